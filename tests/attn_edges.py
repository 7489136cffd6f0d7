"""Edge-probe inputs, an fp64 oracle and a strict comparison rule for the attention kernels.

Plain helper functions for tests/test_attn_edges_{cpu,gpu}.py (no fixtures, no pytest settings).

Why: with randn q / k / v a row that attends over ~1000 keys has an output of size ~0.05, the size of the suite's
absolute tolerance, and one wrong row is fewer elements than the suite's 0.1 % allowance: a mask edge that is off by
one key passes.  Here every probed query row r gets a last visible key e that dominates its softmax and carries a
large value (K[e] = 2 q_r, V[e] = +-8), and the first masked key e + 1 is an even better match with other values
(K[e+1] = 3 q_r, V[e+1] = -+8).  A correct kernel returns ~V[e] for the row, a leak of one key ~V[e+1], a dropped key
~the row mean; every element is compared, none may be wrong.

The bound is |o - o64| <= C * a_abs + 1e-4 with a_abs = softmax(...) |v| (the kernels round P and a pre-scaled Q to
bf16; that error scales with sum p |v|, not with the cancelled result).  C is not tuned on the kernels: it is four
times the largest |emu - o64| / a_abs of a CPU emulation of the kernels' documented rounding (``emulate_all``) over the
committed cases (``CASES``), rounded up to two digits; the factor 4 covers the accumulation order and the hardware
exp2, which the emulation does not model.  tests/test_attn_edges_cpu.py re-measures the floor and holds C to it.
"""
import math
from types import SimpleNamespace

import torch

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn
LOG2E = 1.4426950408889634

# Measured emulation floor (largest |emu - o64| / a_abs over a case, worst rounding variant; the pre-scaled bf16 Q
# dominates): 0.0077 - 0.0151 for the dense cases (largest: f64x2_causal 0.01511, then knob_d64 0.0143, f128_causal
# 0.0133), 0.0111 for paged prefill, 0.0015 - 0.0100 for decode.
FLOOR = 0.01511
C = 0.061          # 4 * FLOOR = 0.0604, rounded up to two digits; stays <= 1 / 16 (mutants reach |err| / a_abs >= 1)
ABS = 1e-4
PAD = 64           # poison rows behind S in the dense K / V buffers
EDGE_KEYS = (63, 255, 511, 128, 320, 1024)   # last / first key of tiles of 32, 64, 128 and 256 keys


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(BF16)


def _pm8(g, *shape):
    return ((torch.randint(0, 2, shape, generator=g) * 2 - 1) * 8).to(BF16)


def probe_rows(kv_len, q_len, off):
    """Causal probes [(row, e)]: e = row + off is the row's last visible key.  The row that ends at kv_len - 1 and
    rows of the last query tile come first, then the tile-edge keys; last visible keys stay >= 2 apart (one row's
    poison key is not the next row's valid key)."""
    want = [kv_len - 1, off + q_len - 1, off + q_len - 4, off + (q_len - 1) // 256 * 256 + 1,
            off + (q_len - 1) // 128 * 128 + 3] + list(EDGE_KEYS)
    got = []
    for e in want:
        r = e - off
        if 0 <= r < q_len and 0 <= e < kv_len and all(abs(e - x) >= 2 for _, x in got):
            got.append((r, e))
    return got


# ----------------------------------------------------------------------------- dense cases
def dense_case(B, Sq, Skv, Hq, Hkv, D, causal=False, causal_offset=0, kv_lens=None, q_lens=None, q_batch_mod=0,
               bias_scale=0.0, seed=0, device="cpu"):
    """q [B or q_batch_mod, Sq, Hq, D]; k / v are the first Skv rows of [B, Skv + PAD, Hkv, D] buffers whose rows from
    kv_len on are poison.  GQA probes align with the first q head of each KV group.  Without causal masking every row
    of a batch ends at kv_len - 1, so each KV head probes another query row."""
    g = _gen(seed)
    Bq = q_batch_mod or B
    G = Hq // Hkv
    q = _randn(g, Bq, Sq, Hq, D)
    kbuf, vbuf = _randn(g, B, Skv + PAD, Hkv, D), _randn(g, B, Skv + PAD, Hkv, D)
    probes = []   # (batch, row, e, kv head or -1 for all)
    for b in range(B):
        kl = kv_lens[b] if kv_lens is not None else Skv
        ql = q_lens[b] if q_lens is not None else Sq
        off = kl - ql if q_lens is not None else causal_offset
        qh = q[b % Bq, :, ::G].float()   # [Sq, Hkv, D]
        if causal:
            rows = probe_rows(kl, ql, off)
            assert rows, "no probe row"
            for r, e in rows:
                kbuf[b, e], vbuf[b, e] = (2 * qh[r]).to(BF16), _pm8(g, Hkv, D)
                if e + 1 < kl:
                    kbuf[b, e + 1], vbuf[b, e + 1] = (3 * qh[r]).to(BF16), _pm8(g, Hkv, D)
                probes.append((b, r, e, -1))
            r_last = max(rows, key=lambda t: t[1])[0]
            kbuf[b, kl:], vbuf[b, kl:] = (3 * qh[r_last]).to(BF16), _pm8(g, Hkv, D)
        else:
            cand = []
            for r in (ql - 1, 0, ql // 2, 127, 128, 255, 256):
                if 0 <= r < ql and r not in cand:
                    cand.append(r)
            for h in range(Hkv):
                r = cand[(b + h) % len(cand)]
                kbuf[b, kl - 1, h], vbuf[b, kl - 1, h] = (2 * qh[r, h]).to(BF16), _pm8(g, D)
                kbuf[b, kl:, h], vbuf[b, kl:, h] = (3 * qh[r, h]).to(BF16), _pm8(g, D)
                probes.append((b, r, kl - 1, h))
    bias = None
    if bias_scale:
        bias = torch.randn(Hq, Sq, Skv, generator=g)
        bias = ((bias - bias.mean(-1, keepdim=True)) * bias_scale).to(BF16)
    i32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device=device)
    kbuf, vbuf = kbuf.to(device), vbuf.to(device)
    return SimpleNamespace(kind="dense", q=q.to(device), k=kbuf[:, :Skv], v=vbuf[:, :Skv], kbuf=kbuf, vbuf=vbuf,
                           causal=causal, causal_offset=causal_offset, kv_lens=i32(kv_lens), q_lens=i32(q_lens),
                           kv_list=kv_lens, q_list=q_lens, q_batch_mod=q_batch_mod,
                           bias=None if bias is None else bias.to(device), scale=1.0 / math.sqrt(D), probes=probes,
                           B=B, Sq=Sq, Skv=Skv)


def dense_vis(c, b):
    """Number of visible keys of every query row of batch b ([Sq] int64): keys 0 .. vis - 1."""
    kl = c.kv_list[b] if c.kv_list is not None else c.Skv
    ql = c.q_list[b] if c.q_list is not None else c.Sq
    off = kl - ql if c.q_list is not None else c.causal_offset
    r = torch.arange(c.Sq, device=c.q.device)
    if not c.causal:
        return torch.full_like(r, kl)
    return (r + off + 1).clamp(0, kl)


def dense_valid(c, b):
    return c.q_list[b] if c.q_list is not None else c.Sq


# ----------------------------------------------------------------------------- paged cases (prefill, varlen, decode)
def paged_case(D, Hq, Hkv, kv_lens, q_lens, fp8=False, k_scale=0.5, v_scale=2.0, seed=0, device="cpu"):
    """Causal attention over a paged cache (64-token blocks, offset kv_len - q_len): q [B, max q_len, Hq, D] (rows past
    q_len unspecified).  The slots behind kv_len in a sequence's last block hold poison, and every unused block-table
    entry (there is at least one per sequence) points at the sequence's own poison block.  fp8: the caches are
    quantised by the cache rule after the probes are planted."""
    g = _gen(seed)
    B, G = len(kv_lens), Hq // Hkv
    need = [(c + 63) // 64 for c in kv_lens]
    maxb = max(need) + 1
    nblocks = sum(need) + B + 3
    kc, vc = _randn(g, nblocks, Hkv, 64, D), _randn(g, nblocks, Hkv, 64, D)
    perm = torch.randperm(nblocks, generator=g)
    q = _randn(g, B, max(q_lens), Hq, D)
    bt = torch.zeros(B, maxb, dtype=torch.int32)
    probes, i = [], 0
    for b, (kl, ql) in enumerate(zip(kv_lens, q_lens)):
        blocks, poison = perm[i:i + need[b]], int(perm[i + need[b]])
        i += need[b] + 1
        bt[b, :need[b]], bt[b, need[b]:] = blocks.int(), poison
        qh = q[b, :, ::G].float()
        off = kl - ql
        for r, e in probe_rows(kl, ql, off):
            blk, s = int(blocks[e // 64]), e % 64
            kc[blk, :, s], vc[blk, :, s] = (2 * qh[r]).to(BF16), _pm8(g, Hkv, D)
            if e + 1 < kl:
                blk, s = int(blocks[(e + 1) // 64]), (e + 1) % 64
                kc[blk, :, s], vc[blk, :, s] = (3 * qh[r]).to(BF16), _pm8(g, Hkv, D)
            probes.append((b, r, e, -1))
        pk, pv = (3 * qh[ql - 1]).to(BF16)[:, None], _pm8(g, Hkv, D)[:, None]   # the last row ends at kv_len - 1
        kc[poison], vc[poison] = pk, pv
        if kl % 64:
            kc[int(blocks[-1]), :, kl % 64:], vc[int(blocks[-1]), :, kl % 64:] = pk, pv
    if fp8:
        from shai_amd.ops import reference as ref
        kc, vc = ref.quantize_kv_fp8(kc, k_scale), ref.quantize_kv_fp8(vc, v_scale)
    else:
        k_scale = v_scale = 1.0
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=device)
    return SimpleNamespace(kind="paged", q=q.to(device), kc=kc.to(device), vc=vc.to(device), bt=bt.to(device),
                           kv_lens=i32(kv_lens), q_lens=i32(q_lens), kv_list=list(kv_lens), q_list=list(q_lens),
                           k_scale=k_scale, v_scale=v_scale, scale=1.0 / math.sqrt(D), probes=probes, B=B, fp8=fp8)


def paged_vis(c, b):
    kl, ql = c.kv_list[b], c.q_list[b]
    return (torch.arange(ql, device=c.q.device) + kl - ql + 1).clamp(0, kl)


def paged_linear(cache, bt_row, scale):
    """Every block of a block-table row as [blocks * 64, Hkv, D] float (an fp8 cache dequantised as ops.reference
    does: float(code) * scale in fp32)."""
    blocks = cache[bt_row.long()]
    if cache.dtype == F8:
        blocks = blocks.float() * torch.tensor(float(scale), dtype=torch.float32, device=cache.device)
    return blocks.permute(0, 2, 1, 3).reshape(-1, cache.shape[1], cache.shape[3])


def packed(c):
    """The packed varlen layout of a paged case: q [T, Hq, D], q_start [B] int32."""
    q = torch.cat([c.q[b, :ql] for b, ql in enumerate(c.q_list)])
    starts = [sum(c.q_list[:b]) for b in range(c.B)]
    return q, torch.tensor(starts, dtype=torch.int32, device=c.q.device)


# ----------------------------------------------------------------------------- fp64 oracle and the rounding emulation
def _head_chunks(q, k, v, bias):
    """(q head slice, q, k, v, bias) in groups of about 8 q heads: bounds the [heads, Sq, L] score buffer."""
    Hq, Hkv = q.shape[1], k.shape[1]
    G = Hq // Hkv
    step = max(1, 8 // G)
    for k0 in range(0, Hkv, step):
        k1 = min(Hkv, k0 + step)
        hs = slice(k0 * G, k1 * G)
        yield hs, q[:, hs], k[:, k0:k1], v[:, k0:k1], None if bias is None else bias[hs]


def _masked_scores(q, k, vis, scale, dt, L):
    """q [Sq, H, D] x k [L', Hkv, D] -> scores [H, Sq, L] * scale and the mask [1, Sq, L] of hidden keys."""
    Hq, Hkv = q.shape[1], k.shape[1]
    kd = k[:L].to(dt).permute(1, 0, 2).repeat_interleave(Hq // Hkv, 0)   # [Hq, L, D]
    s = torch.matmul(q.to(dt).permute(1, 0, 2), kd.transpose(1, 2)) * scale
    mask = torch.arange(L, device=q.device)[None, :] >= vis[:, None]
    return s, mask[None]


def attend64(q, k, v, vis, scale, bias=None):
    """fp64 softmax(mask(q k^T * scale + bias)) v and softmax(...) |v| for one sequence: q [Sq, Hq, D], k / v [L, Hkv,
    D] linear memory (values as the kernel reads them), row i sees keys 0 .. vis[i] - 1 (vis may reach past the
    kernel's kv_len: that is how the mutants leak).  A row with no visible key returns 0."""
    L = max(1, min(k.shape[0], int(vis.max())))
    o = torch.empty(q.shape, dtype=torch.float64, device=q.device)
    a = torch.empty_like(o)
    for hs, qq, kk, vv, bb in _head_chunks(q, k, v, bias):
        s, mask = _masked_scores(qq, kk, vis, scale, torch.float64, L)
        if bb is not None:
            w = min(L, bb.shape[-1])
            s[..., :w] += bb[..., :w].double()
        p = torch.nan_to_num(torch.softmax(s.masked_fill(mask, float("-inf")), -1), nan=0.0)
        vd = vv[:L].double().permute(1, 0, 2).repeat_interleave(qq.shape[1] // kk.shape[1], 0)
        o[:, hs] = torch.matmul(p, vd).permute(1, 0, 2)
        a[:, hs] = torch.matmul(p, vd.abs()).permute(1, 0, 2)
    return o, a


def _bf16_trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


# (Q * scale * log2(e) rounded to bf16 before QK^T, P truncated instead of rounded, row sum over the rounded P)
EMU_VARIANTS = [(pre, trunc, rsum) for pre in (True, False) for trunc in (False, True) for rsum in (False, True)]


def emulate_all(q, k, v, vis, scale, bias=None):
    """The kernels' documented rounding, on the CPU, every variant of EMU_VARIANTS -> fp32 [Sq, Hq, D]: scores in the
    exp2 domain from bf16 operands (optionally with Q pre-multiplied by scale * log2(e) and rounded to bf16: flash64 /
    flash2), fp32 accumulation, P = exp2(s - max) rounded (or truncated) to bf16 for P.V, the row sum in fp32 over the
    unrounded P (flash kernels) or over the rounded P (decode kernels), output rounded to bf16."""
    L = max(1, min(k.shape[0], int(vis.max())))
    sl2 = scale * LOG2E
    outs = {var: torch.empty(q.shape, dtype=torch.float32, device=q.device) for var in EMU_VARIANTS}
    for hs, qq, kk, vv, bb in _head_chunks(q, k, v, bias):
        vd = vv[:L].float().permute(1, 0, 2).repeat_interleave(qq.shape[1] // kk.shape[1], 0)
        for pre in (True, False):
            if pre:
                s, mask = _masked_scores((qq.float() * sl2).to(BF16), kk, vis, 1.0, torch.float32, L)
            else:
                s, mask = _masked_scores(qq, kk, vis, sl2, torch.float32, L)
            if bb is not None:
                w = min(L, bb.shape[-1])
                s[..., :w] += bb[..., :w].float() * LOG2E
            s = s.masked_fill(mask, float("-inf"))
            p = torch.nan_to_num(torch.exp2(s - s.amax(-1, keepdim=True)), nan=0.0)
            lsum = p.sum(-1, keepdim=True)
            for trunc in (False, True):
                pb = _bf16_trunc(p) if trunc else p.to(BF16).float()
                pv = torch.matmul(pb, vd)
                for rsum in (False, True):
                    l = pb.sum(-1, keepdim=True) if rsum else lsum
                    outs[(pre, trunc, rsum)][:, hs] = (pv / l.clamp_min(1e-30)).permute(1, 0, 2)
    return {var: o.to(BF16).float() for var, o in outs.items()}


def sequences(c):
    """Yield (index into the output, q [n, Hq, D], k, v linear memory, vis [n], bias) per sequence of a case; the
    output index selects the compared rows (rows past q_len are unspecified)."""
    if c.kind == "dense":
        for b in range(c.B):
            n = dense_valid(c, b)
            bq = b % c.q_batch_mod if c.q_batch_mod else b
            yield (b, slice(0, n)), c.q[bq, :n], c.kbuf[b], c.vbuf[b], dense_vis(c, b)[:n], (
                None if c.bias is None else c.bias[:, :n])
    else:
        for b in range(c.B):
            n = c.q_list[b]
            yield (b, slice(0, n)), c.q[b, :n], paged_linear(c.kc, c.bt[b], c.k_scale), paged_linear(
                c.vc, c.bt[b], c.v_scale), paged_vis(c, b), None


def oracle(c, mutate=None):
    """[(output index, o64, a_abs)] per sequence.  mutate(b, vis, kv_len) -> vis' moves the mask edge (test mutants)."""
    out = []
    for (b, rows), q, k, v, vis, bias in sequences(c):
        if mutate is not None:
            vis = mutate(b, vis, c.kv_list[b] if c.kv_list is not None else c.Skv).clamp(0, k.shape[0])
        o, a = attend64(q, k, v, vis, c.scale, bias)
        out.append(((b, rows), o, a))
    return out


def floor_of(c):
    """Largest |emu - o64| / a_abs of the worst emulation variant over a case (the rounding floor)."""
    worst = 0.0
    for _, q, k, v, vis, bias in sequences(c):
        o, a = attend64(q, k, v, vis, c.scale, bias)
        for e in emulate_all(q, k, v, vis, c.scale, bias).values():
            worst = max(worst, float(((e.double() - o).abs() / (a + ABS)).max()))
    return worst


# ----------------------------------------------------------------------------- the strict rule
def assert_edges_close(o, o64, a_abs, c=C, what=""):
    """Every element finite and |o - o64| <= c * a_abs + 1e-4: no share of elements left out.  Returns the largest
    |o - o64| / (c * a_abs + 1e-4) (<= 1)."""
    o = o.double()
    assert o.shape == o64.shape, f"{what}: shape {tuple(o.shape)} vs {tuple(o64.shape)}"
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    ratio = (o - o64).abs() / (c * a_abs + ABS)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        idx = [int(i) for i in (ratio == ratio.max()).nonzero()[0]]
        n = int((ratio > 1.0).sum())
        raise AssertionError(
            f"{what}: {n} of {ratio.numel()} elements out of bound; worst at {idx}: got {float(o[tuple(idx)]):.5g}, "
            f"want {float(o64[tuple(idx)]):.5g}, a_abs {float(a_abs[tuple(idx)]):.4g} "
            f"(|err| / a_abs = {worst * c:.4g}, bound {c})")
    return worst


def check(c, out, ref=None, what=""):
    """Compare a kernel's output (indexed as the case's q: [B, S, Hq, D]) with the case's oracle, sequence by
    sequence; the probed rows must also have landed on their planted value (the probe really dominates)."""
    ref = ref if ref is not None else oracle(c)
    worst = 0.0
    for (b, rows), o64, a in ref:
        worst = max(worst, assert_edges_close(out[b, rows], o64, a, what=f"{what} sequence {b}"))
    return worst


def probes_dominate(c, ref):
    """Share of probed (row, head) pairs whose oracle output is within 1 of the planted +-8 in every dimension."""
    by_b = {b: o for (b, _), o, _ in ref}
    hit = tot = 0
    for b, r, e, h in c.probes:
        o = by_b[b][r]
        G = o.shape[0] // (c.kbuf.shape[2] if c.kind == "dense" else c.kc.shape[1])
        heads = range(0, o.shape[0], G) if h < 0 else [h * G]
        for hq in heads:
            tot += 1
            hit += int(bool(((o[hq].abs() - 8).abs() < 1).all()))
    return hit / max(tot, 1)


# ----------------------------------------------------------------------------- the committed cases
# name -> (builder, kwargs); each test names the kernel its case lands on.
def _d(**kw):
    return ("dense", kw)


def _p(**kw):
    return ("paged", kw)


PREFILL_PAIRS = [(64, 64), (65, 65), (128, 37), (300, 300), (129, 1)]   # (kv_len, q_len)
DECODE_CTX = [1, 2, 63, 64, 65, 128, 129, 300, 1000]
X2_LENS = [1100, 1090, 1024, 777, 300, 1100, 65, 1000]

CASES = {
    # v1 (flash_fwd_kernel<128>): Sq, Skv < 512
    "v1_d128": _d(B=2, Sq=333, Skv=333, Hq=8, Hkv=2, D=128, kv_lens=[333, 65], seed=1),
    "v1_d128_causal": _d(B=2, Sq=333, Skv=333, Hq=8, Hkv=2, D=128, causal=True, kv_lens=[333, 65], seed=2),
    "v1_d128_causal_qlens": _d(B=2, Sq=333, Skv=333, Hq=8, Hkv=2, D=128, causal=True, kv_lens=[333, 65],
                               q_lens=[200, 40], seed=3),
    # v1 (flash_fwd_kernel<64>): a bias keeps D = 64 off flash64
    "v1_d64_bias": _d(B=2, Sq=150, Skv=150, Hq=4, Hkv=4, D=64, kv_lens=[150, 77], bias_scale=0.5, seed=4),
    # flash64-DMA
    "f64dma": _d(B=3, Sq=700, Skv=700, Hq=8, Hkv=2, D=64, kv_lens=[700, 600, 65], seed=5),
    "f64dma_causal": _d(B=3, Sq=700, Skv=700, Hq=8, Hkv=2, D=64, causal=True, kv_lens=[700, 600, 65],
                        q_lens=[700, 600, 65], seed=6),
    "f64dma_cross": _d(B=2, Sq=600, Skv=77, Hq=8, Hkv=2, D=64, kv_lens=[77, 33], seed=7),
    "f64dma_shared_q": _d(B=2, Sq=700, Skv=700, Hq=8, Hkv=2, D=64, kv_lens=[700, 590], q_batch_mod=1, seed=8),
    # flash64x2: ceil(1100 / 256) * 32 * 8 = 1280 >= 1024 workgroups, Skv >= 512
    "f64x2": _d(B=8, Sq=1100, Skv=1100, Hq=32, Hkv=8, D=64, kv_lens=X2_LENS, seed=9),
    "f64x2_causal": _d(B=8, Sq=1100, Skv=1100, Hq=32, Hkv=8, D=64, causal=True, kv_lens=X2_LENS, q_lens=X2_LENS,
                       seed=10),
    # flash2<128> (and flash128x2 under set_flash128x2(1)): Sq, Skv >= 512
    "f128": _d(B=2, Sq=1100, Skv=1100, Hq=4, Hkv=2, D=128, kv_lens=[1100, 1090], seed=11),
    "f128_causal": _d(B=2, Sq=1100, Skv=1100, Hq=4, Hkv=2, D=128, causal=True, kv_lens=[1100, 1090],
                      q_lens=[1100, 1090], seed=12),
    "f128_chunk": _d(B=1, Sq=600, Skv=1500, Hq=4, Hkv=2, D=128, causal=True, causal_offset=900, seed=13),
    # attn512: one head, no masks; the key tail ends at the buffer's poison rows
    "a512_1000": _d(B=2, Sq=1000, Skv=1000, Hq=1, Hkv=1, D=512, seed=14),
    "a512_1024": _d(B=2, Sq=1024, Skv=1024, Hq=1, Hkv=1, D=512, seed=15),
    # paged prefill (v1 body, paged K/V), padded and packed
    "paged_prefill": _p(D=128, Hq=8, Hkv=2, kv_lens=[p[0] for p in PREFILL_PAIRS],
                        q_lens=[p[1] for p in PREFILL_PAIRS], seed=16),
    # decode
    "decode_d128_g4": _p(D=128, Hq=8, Hkv=2, kv_lens=DECODE_CTX, q_lens=[1] * 9, seed=17),
    "decode_d64_g1": _p(D=64, Hq=4, Hkv=4, kv_lens=DECODE_CTX, q_lens=[1] * 9, seed=18),
    "decode_d64_g4": _p(D=64, Hq=8, Hkv=2, kv_lens=DECODE_CTX, q_lens=[1] * 9, seed=19),
    "decode_d128_g4_fp8": _p(D=128, Hq=8, Hkv=2, kv_lens=DECODE_CTX, q_lens=[1] * 9, fp8=True, seed=20),
    "decode_d64_g1_fp8": _p(D=64, Hq=4, Hkv=4, kv_lens=DECODE_CTX, q_lens=[1] * 9, fp8=True, seed=21),
    "decode_d64_g4_fp8": _p(D=64, Hq=8, Hkv=2, kv_lens=DECODE_CTX, q_lens=[1] * 9, fp8=True, seed=22),
    # the kernels only an environment knob reaches (tests/attn_edges_worker.py)
    "knob_d64": _d(B=2, Sq=2200, Skv=2200, Hq=4, Hkv=2, D=64, causal=True, kv_lens=[2200, 2090],
                   q_lens=[2200, 2090], seed=23),
    "knob_d128": _d(B=2, Sq=1100, Skv=1100, Hq=4, Hkv=2, D=128, causal=True, kv_lens=[1100, 1090],
                    q_lens=[1100, 1090], seed=24),
}


def make(name, device="cpu", **over):
    kind, kw = CASES[name]
    kw = dict(kw, **over)
    return (dense_case if kind == "dense" else paged_case)(device=device, **kw)
