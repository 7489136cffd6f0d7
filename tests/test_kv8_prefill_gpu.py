"""Native fp8 paged prefill attention (``kv_prefill="native"``): the paged flash kernel reads the e4m3fn cache codes
itself and widens them to bf16 while staging a K/V tile.

Oracle.  After staging, the native route and the widen route (``kv_dequant_blocks`` into a bf16 scratch + the bf16
paged kernel) run the same code on the same kind of bf16 LDS tiles; widening a code to bf16 is exact, and with
power-of-two scales every folded scale (k_scale into the score scale, v_scale into the final normalisation) commutes
exactly with the roundings.  So at scales (1, 1) and (0.5, 2.0) native must equal widen bit for bit.  At (0.3, 1.7)
the widen route rounds code * scale to bf16 and native does not: there, and at the power-of-two scales too, the
check is tests/test_kv8_gpu.py's ``close`` rule (atol 2e-2, rtol 2e-2, fewer than 1e-3 of the elements outside)
against ``ref.paged_attention*`` over the fp32-dequantised cache."""
import math

import pytest
import torch

import shai_amd.ops as ops
from shai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
POW2 = [(1.0, 1.0), (0.5, 2.0)]
SCALES = POW2 + [(0.3, 1.7)]
NAN_CODE = 0x7F   # e4m3fn has no infinities; S.1111.111 is its NaN


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(torch.bfloat16)


def close(a, b, atol=2e-2, rtol=2e-2):   # tests/test_kv8_gpu.py's rule
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    print(f"max err {err.max().item():.4g}, {bad * 100:.4f}% outside")
    assert torch.isfinite(a).all(), "non-finite output"
    assert bad < 1e-3, f"{bad*100:.3f}% elements out of tolerance; max err {err.max().item():.4g}"


def _u8(t):
    return t.view(torch.uint8)


def _caches(nblocks, Hkv, D, ks, vs):
    return (ops.quantize_kv_fp8(rnd(nblocks, Hkv, 64, D), ks), ops.quantize_kv_fp8(rnd(nblocks, Hkv, 64, D), vs))


def _table(ctx, nblocks):
    """Block tables drawn from a random permutation of the whole pool."""
    need = [(c + 63) // 64 for c in ctx]
    assert sum(need) <= nblocks
    perm = torch.randperm(nblocks).tolist()
    bt = torch.zeros(len(ctx), max(need), dtype=torch.int32)
    i = 0
    for b, n in enumerate(need):
        bt[b, :n] = torch.tensor(perm[i:i + n], dtype=torch.int32)
        i += n
    return bt.cuda()


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _padded_case(D, Hq, Hkv, ctx, q_lens, ks, vs):
    """One padded-layout step by both routes and the fp32 reference; only rows below q_len are defined."""
    B, S = len(ctx), max(q_lens)
    nblocks = sum((c + 63) // 64 for c in ctx) + 5
    kc, vc = _caches(nblocks, Hkv, D, ks, vs)
    bt = _table(ctx, nblocks)
    q = rnd(B, S, Hq, D)
    kl, ql = _i32(ctx), _i32(q_lens)
    want = ref.paged_attention(q.float(), ops.dequant_kv_fp8(kc, ks, torch.float32),
                               ops.dequant_kv_fp8(vc, vs, torch.float32), bt, kl, ql, 1 / math.sqrt(D))
    nat = ops.paged_attention(q, kc, vc, bt, kl, ql, k_scale=ks, v_scale=vs, kv_prefill="native")
    wid = ops.paged_attention(q, kc, vc, bt, kl, ql, k_scale=ks, v_scale=vs, kv_prefill="widen")
    rows = lambda o: torch.cat([o[b, :n].reshape(-1) for b, n in enumerate(q_lens)])
    return rows(nat), rows(wid), rows(want)


def _check(nat, wid, want, ks, vs):
    close(nat, want)
    if (ks, vs) in POW2:
        print(f"scales {ks}, {vs}: {int((nat != wid).sum())} of {nat.numel()} elements differ from the widen route")
        assert torch.equal(nat, wid)


@pytest.mark.parametrize("ks,vs", SCALES)
@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (64, 4, 4), (64, 8, 1)])
def test_padded_two_query_tiles_and_tail_block(cuda, D, Hq, Hkv, ks, vs):
    """Contexts [100, 300], q_lens [37, 300]: full 128-row query tiles and a partial last one, a chunk on top of
    cached tokens (causal offset 63), partial tail blocks."""
    torch.manual_seed(13)
    _check(*_padded_case(D, Hq, Hkv, [100, 300], [37, 300], ks, vs), ks, vs)


@pytest.mark.parametrize("ks,vs", SCALES)
@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (64, 4, 4), (64, 8, 1)])
@pytest.mark.parametrize("full", [False, True])
def test_padded_block_edges(cuda, D, Hq, Hkv, ks, vs, full):
    """Contexts around the 64-token block edge, as decode rows (q_len 1) and as whole fresh prompts (q_len = ctx)."""
    torch.manual_seed(17)
    ctx = [1, 63, 64, 65, 129]
    _check(*_padded_case(D, Hq, Hkv, ctx, ctx if full else [1] * len(ctx), ks, vs), ks, vs)


def _packed_inputs(D, Hq, Hkv, n_cached, n_new, ks, vs, extra=4):
    ctx = [c + n for c, n in zip(n_cached, n_new)]
    nblocks = sum((c + 63) // 64 for c in ctx) + extra
    kc, vc = _caches(nblocks, Hkv, D, ks, vs)
    bt = _table(ctx, nblocks)
    q = rnd(sum(n_new), Hq, D)
    q_start = _i32([sum(n_new[:i]) for i in range(len(n_new))])
    return q, kc, vc, bt, _i32(ctx), _i32(n_new), q_start


def _varlen(route, q, kc, vc, bt, kl, ql, qs, max_q, ks, vs):
    return ops.paged_attention_varlen(q, kc, vc, bt, kl, ql, qs, max_q, k_scale=ks, v_scale=vs, kv_prefill=route)


N_CACHED = [0, 130, 0, 300, 63]
N_NEW = [64, 1, 200, 70, 1]


@pytest.mark.parametrize("ks,vs", SCALES)
@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (64, 4, 4), (64, 8, 1)])
def test_packed_mixed_step(cuda, D, Hq, Hkv, ks, vs):
    """Fresh prompts, decode rows, a chunk on top of cached tokens and a decode row that opens a new block (63
    cached + 1), packed back to back."""
    torch.manual_seed(0)
    q, kc, vc, bt, kl, ql, qs = _packed_inputs(D, Hq, Hkv, N_CACHED, N_NEW, ks, vs)
    want = ref.paged_attention_varlen(q.float(), ops.dequant_kv_fp8(kc, ks, torch.float32),
                                      ops.dequant_kv_fp8(vc, vs, torch.float32), bt, kl, ql, qs, 1 / math.sqrt(D), True)
    nat = _varlen("native", q, kc, vc, bt, kl, ql, qs, max(N_NEW), ks, vs)
    wid = _varlen("widen", q, kc, vc, bt, kl, ql, qs, max(N_NEW), ks, vs)
    _check(nat, wid, want, ks, vs)
    # launch groups (the engine's split of a mixed step) partition the sequences and change no row
    grouped = ops.paged_attention_varlen(q, kc, vc, bt, kl, ql, qs, max(N_NEW), k_scale=ks, v_scale=vs,
                                         kv_prefill="native", q_groups=[(0, 1, 64), (1, 0, 1), (1, 3, 200), (4, 1, 1)])
    assert torch.equal(grouped, nat)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (64, 4, 4)])
def test_poisoned_slots_are_never_read(cuda, D, Hq, Hkv):
    """Every cache slot at or beyond a sequence's kv_len and every block no table names holds the e4m3fn NaN code:
    the output is finite and bit-equal to the widen route over a copy with zeros there (P = 0 times NaN would be
    NaN, so the kernel must not let those codes into its tiles)."""
    torch.manual_seed(3)
    ks, vs = 0.5, 2.0
    q, kc, vc, bt, kl, ql, qs = _packed_inputs(D, Hq, Hkv, N_CACHED, N_NEW, ks, vs)
    live = torch.zeros(kc.shape[0], 64, dtype=torch.bool, device="cuda")   # [block, token]
    for b, L in enumerate(kl.tolist()):
        for i in range((L + 63) // 64):
            live[int(bt[b, i]), :min(64, L - 64 * i)] = True
    dead = ~live[:, None, :, None].expand(-1, Hkv, -1, D)
    assert int(dead.sum()) > 4 * Hkv * 64 * D   # the spare blocks and the tails
    kp, vp, kz, vz = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    for poisoned, zeroed in ((kp, kz), (vp, vz)):
        _u8(poisoned)[dead] = NAN_CODE
        _u8(zeroed)[dead] = 0
    assert torch.isnan(kp.float()).any() and not torch.isnan(kz.float()).any()
    nat = _varlen("native", q, kp, vp, bt, kl, ql, qs, max(N_NEW), ks, vs)
    wid = _varlen("widen", q, kz, vz, bt, kl, ql, qs, max(N_NEW), ks, vs)
    assert torch.isfinite(nat.float()).all()
    assert torch.equal(nat, wid)


def test_blocks_beyond_two_gib(cuda):
    """A pool of 33,000 blocks at Hkv 8, D 128 is 2.16e9 bytes per cache: blocks above 32,768 start beyond 2^31
    bytes, so the cache offsets must be 64-bit.  Only the used blocks are written; the output equals the same
    blocks placed at the bottom of a small pool, bit for bit."""
    torch.manual_seed(5)
    D, Hq, Hkv, ks, vs = 128, 16, 8, 0.5, 2.0
    n_cached, n_new = [130, 0], [70, 65]
    q, kc, vc, bt, kl, ql, qs = _packed_inputs(D, Hq, Hkv, n_cached, n_new, ks, vs, extra=0)
    low = _varlen("native", q, kc, vc, bt, kl, ql, qs, max(n_new), ks, vs)
    nb, big = kc.shape[0], 33000
    assert big * Hkv * 64 * D > 2 ** 31
    kbig = torch.empty(big, Hkv, 64, D, dtype=torch.uint8, device="cuda").view(F8)
    vbig = torch.empty(big, Hkv, 64, D, dtype=torch.uint8, device="cuda").view(F8)
    far = torch.arange(big - 1, big - 1 - 3 * nb, -3, device="cuda")   # block i of the small pool -> far[i]
    assert int(far.min()) > 32768
    _u8(kbig)[far] = _u8(kc)
    _u8(vbig)[far] = _u8(vc)
    bt_far = far[bt.long()].to(torch.int32).contiguous()
    high = _varlen("native", q, kbig, vbig, bt_far, kl, ql, qs, max(n_new), ks, vs)
    assert torch.isfinite(high.float()).all()
    assert torch.equal(high, low)


def test_native_call_captures_in_a_graph(cuda):
    """The native route reads no device tensor on the host, so one call captures in a HIP graph (one stream); a
    replay after the cache codes were overwritten in place attends the new contents."""
    torch.manual_seed(7)
    D, Hq, Hkv, ks, vs = 128, 8, 2, 0.5, 2.0
    q, kc, vc, bt, kl, ql, qs = _packed_inputs(D, Hq, Hkv, N_CACHED, N_NEW, ks, vs)
    first = _varlen("native", q, kc, vc, bt, kl, ql, qs, max(N_NEW), ks, vs)   # (also loads the kernel)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _varlen("native", q, kc, vc, bt, kl, ql, qs, max(N_NEW), ks, vs)
    k2, v2 = _caches(kc.shape[0], Hkv, D, ks, vs)
    kc.copy_(k2)
    vc.copy_(v2)
    g.replay()
    torch.cuda.synchronize()
    eager = _varlen("native", q, k2, v2, bt, kl, ql, qs, max(N_NEW), ks, vs)
    assert torch.equal(out, eager) and not torch.equal(out, first)


def _run_engine(eng, monkeypatch=None):
    """Two short sequences start decoding, a 200-token prompt joins them (64-token chunks in mixed steps), then a
    request repeats the long prompt's first blocks (prefix-cache hit).  Returns every step's logits and the tokens."""
    from shai_amd.engines.llm import SamplingParams
    rec = []
    fwd = eng.model.forward
    eng.model.forward = lambda *a, **k: (lambda y: (rec.append(y.float().clone()), y)[1])(fwd(*a, **k))
    p = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    long_prompt = [(7 * i) % 200 + 10 for i in range(200)]
    seqs = [eng.add_request([9, 8, 7, 6], p), eng.add_request([1, 2, 3], p)]
    eng.step()
    seqs.append(eng.add_request(long_prompt, p))
    while not all(s.finished for s in seqs):
        eng.step()
    hits = eng.stats["prefix_hit_tokens"]
    seqs.append(eng.add_request(long_prompt[:150] + [5, 4, 3], p))
    while not seqs[-1].finished:
        eng.step()
    assert eng.stats["prefix_hit_tokens"] >= hits + 128   # two full blocks of the long prompt were reused
    return rec, [s.output for s in seqs]


def test_engine_native_equals_widen(cuda, monkeypatch):
    """Tiny Llama, eager, same seed and weights, fp8 cache at the default scales (1, 1): every step's logits of the
    native engine equal the widen engine's bit for bit.  The native engine holds no scratch and never widens."""
    from shai_amd.engines.llm import LLMEngine
    from shai_amd.models.llama import LlamaConfig
    c = LlamaConfig.tiny()
    kw = dict(device=cuda, max_num_seqs=4, max_model_len=256, seed=1, enable_prefix_caching=True, prefill_chunk=64,
              kv_cache_dtype="fp8", use_graphs=False, async_decode=False)
    ew = LLMEngine(c, kv_prefill="widen", **kw)
    assert ew.kv_scratch is not None and ew.kv_scratch_blocks > 0
    want_logits, want_toks = _run_engine(ew)
    en = LLMEngine(c, kv_prefill="native", **kw)
    assert en.kv_prefill == "native" and en.kv_scratch is None
    assert en.kv_scratch_blocks == 0 and en.kv_scratch_bytes == 0

    def never(*a, **k):
        raise AssertionError("the native route widened cache blocks")
    monkeypatch.setattr(ops, "kv_dequant_blocks", never)
    planned = []
    att = en._attach_kv_rounds
    groups = []
    en._attach_kv_rounds = lambda batch, *a: (att(batch, *a), groups.append(batch.q_groups), planned.append(
        (batch.kv_prefill, batch.kv_rounds, batch.kv_scratch)))[0]
    got_logits, got_toks = _run_engine(en)
    assert len(planned) >= 5 and all(p == ("native", None, None) for p in planned), planned
    assert [(0, 1, 64), (1, 2, 1)] in groups, groups   # a chunk of the long prompt with the two decode rows behind it
    assert got_toks == want_toks and len(got_logits) == len(want_logits)
    for i, (g, w) in enumerate(zip(got_logits, want_logits)):
        assert torch.equal(g, w), (i, (g - w).abs().max().item())
    assert en.bm.num_free == en.num_kv_blocks and ew.bm.num_free == ew.num_kv_blocks


def test_binding_checks(cuda):
    D, Hq, Hkv = 128, 4, 2
    kc, vc = _caches(3, Hkv, D, 1.0, 1.0)
    q = rnd(1, 5, Hq, D)
    bt = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    kl, ql = _i32([5]), _i32([5])
    with pytest.raises((RuntimeError, ValueError), match="differ"):   # an fp8 K with a bf16 V
        ops.paged_attention(q, kc, vc.to(torch.bfloat16), bt, kl, ql, kv_prefill="native")
    K = ops._K()
    with pytest.raises(RuntimeError, match="differ"):
        K.flash_attn(q, kc, vc.to(torch.bfloat16), torch.empty_like(q), 0.1, True, 0, kl, ql, None, bt, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="block_table"):   # an fp8 cache is paged: no dense form
        K.flash_attn(q, kc, vc, torch.empty_like(q), 0.1, True, 0, kl, ql, None, None, 1.0, 1.0)
    for ks, vs in ((0.0, 1.0), (1.0, -2.0), (float("inf"), 1.0)):
        with pytest.raises(RuntimeError, match="positive and finite"):
            ops.paged_attention(q, kc, vc, bt, kl, ql, k_scale=ks, v_scale=vs, kv_prefill="native")
        with pytest.raises(RuntimeError, match="positive and finite"):
            ops.paged_attention_varlen(q[0], kc, vc, bt, kl, ql, _i32([0]), 5, k_scale=ks, v_scale=vs,
                                       kv_prefill="native")
    with pytest.raises(ValueError, match="kv_prefill"):
        ops.paged_attention(q, kc, vc, bt, kl, ql, kv_prefill="scratchless")
    # the argument is ignored for a bf16 cache
    kb, vb = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    assert torch.equal(ops.paged_attention(q, kb, vb, bt, kl, ql, kv_prefill="native"),
                       ops.paged_attention(q, kb, vb, bt, kl, ql))
