"""FP8 (OCP e4m3fn) KV cache on the GPU: the writers are bit-exact against the quantisation rule, the fp8 split
decode kernel (unfused, fused, QKV partial slabs) and the prefill-through-scratch path meet the bf16 kernels'
tolerance against the fp32 reference over the dequantised cache (both sides share the quantisation), and an fp8-KV
engine tracks a CPU fp8-KV engine."""
import math

import pytest
import torch

import shai_amd.ops as ops
from shai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn


def rnd(*shape, scale=1.0, device="cuda"):
    return (torch.randn(*shape, device=device) * scale).to(torch.bfloat16)


def close(a, b, atol, rtol=2e-2):   # tests/test_kernels_gpu.py's rule
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    assert torch.isfinite(a).all(), "non-finite output"
    assert bad < 1e-3, f"{bad*100:.3f}% elements out of tolerance; max err {err.max().item():.4g}"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


def _u8(t):
    return t.view(torch.uint8)


def _wide(*shape):
    """bf16 values with some above +-448 (clamped) and some below 2^-9 (flushed to the zero code)."""
    x = torch.randn(*shape, device="cuda") * 40
    m = torch.rand(*shape, device="cuda")
    x = torch.where(m < 0.05, x * 30, x)           # |x| up to a few thousand
    x = torch.where(m > 0.9, x * 1e-5, x)          # far below the smallest subnormal
    return x.to(torch.bfloat16)


def _code_steps(a, b):
    """Distance in fp8 code steps (codes ordered by value: sign-magnitude -> signed integer)."""
    def order(c):
        c = _u8(c).int()
        return torch.where(c >= 128, -(c - 128), c)
    return (order(a) - order(b)).abs()


def _check_codes(got, want, scale):
    if scale in (1.0, 0.25):
        assert torch.equal(_u8(got), _u8(want))
    else:   # 1 / scale is not a power of two: x * (1 / scale) rounds once more; a code step at most, and rarely
        d = _code_steps(got, want)
        print(f"scale {scale}: {(d > 0).float().mean().item() * 100:.4f}% of codes differ, max {int(d.max())} step(s)")
        assert int(d.max()) <= 1


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("scale", [1.0, 0.25, 0.3])
def test_kv_write_fp8_bit_exact(cuda, D, scale):
    torch.manual_seed(14)
    T, H = 70, 8
    k, v = _wide(T, H, D), _wide(T, H, D)
    assert (k.float().abs() > 448).any() and ((k.float().abs() < 2 ** -9) & (k != 0)).any()
    kc = torch.zeros(4, H, 64, D, dtype=F8, device="cuda")
    vc = torch.zeros_like(kc)
    slots = torch.randperm(256, device="cuda")[:T].to(torch.int32)
    kr, vr = kc.clone().cpu(), vc.clone().cpu()
    ops.kv_write(k, v, kc, vc, slots, scale, 2 * scale)
    ref.kv_write(k.cpu(), v.cpu(), kr, vr, slots.cpu(), scale, 2 * scale)
    assert _u8(kc).any()
    _check_codes(kc.cpu(), kr, scale)
    _check_codes(vc.cpu(), vr, scale)


@pytest.mark.parametrize("D,H,Hk", [(128, 8, 2), (64, 4, 4)])
@pytest.mark.parametrize("scale", [1.0, 0.25, 0.3])
def test_rope_qkv_cache_fp8_bit_exact(cuda, D, H, Hk, scale):
    """K: NeoX rope in fp32, rounded to bf16 (what the bf16 cache would hold), then the rule; V: the rule.  q is
    roped in place as bf16 (checked as tests/test_skinny_gpu.py checks the bf16-cache kernel); slot -1 writes
    nothing."""
    torch.manual_seed(5)
    T, nb = 33, 6
    qkv = _wide(T, (H + 2 * Hk) * D)
    pos = torch.randint(0, 300, (T,), device="cuda", dtype=torch.int32)
    ang = torch.rand(512, D // 2, device="cuda") * 3
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    slots = torch.randperm(nb * 64, device="cuda")[:T].int()
    slots[3] = -1
    kc = torch.zeros(nb, Hk, 64, D, dtype=F8, device="cuda")
    vc = torch.zeros_like(kc)
    kc2, vc2, qkv2 = kc.clone().cpu(), vc.clone().cpu(), qkv.clone().cpu()
    orig = qkv.clone()
    ops.rope_qkv_cache(qkv, pos, cos, sin, kc, vc, slots, H, Hk, scale, 2 * scale)
    k = qkv2[:, H * D:(H + Hk) * D].view(T, Hk, D)
    v = qkv2[:, (H + Hk) * D:].view(T, Hk, D)
    ref.rope(k, pos.cpu(), cos.cpu(), sin.cpu(), D, True)        # in place, rounded to bf16
    ref.kv_write(k, v, kc2, vc2, slots.cpu(), scale, 2 * scale)  # quantize_kv_fp8 into the fp8 cache
    _check_codes(kc.cpu(), kc2, scale)
    _check_codes(vc.cpu(), vc2, scale)
    # q roped in place; the k / v columns of qkv untouched
    q = qkv2[:, :H * D].view(T, H, D)
    ref.rope(q, pos.cpu(), cos.cpu(), sin.cpu(), D, True)
    assert _rel(qkv[:, :H * D], qkv2[:, :H * D]) < 1e-2
    assert torch.equal(qkv[:, H * D:], orig[:, H * D:])
    s3 = int(slots[2])
    assert _u8(kc)[s3 // 64, :, s3 % 64].any() and int(_u8(kc).ne(0).any(-1).sum()) == (T - 1) * Hk


def _paged_setup8(B, Hkv, D, ctx, nblocks, ks, vs):
    kc = ops.quantize_kv_fp8(rnd(nblocks, Hkv, 64, D), ks)
    vc = ops.quantize_kv_fp8(rnd(nblocks, Hkv, 64, D), vs)
    maxb = max((c + 63) // 64 for c in ctx)
    perm = torch.randperm(nblocks, device="cuda").to(torch.int32)
    bt = torch.zeros(B, maxb, dtype=torch.int32, device="cuda")
    i = 0
    for b, c in enumerate(ctx):
        nb = (c + 63) // 64
        bt[b, :nb] = perm[i:i + nb]
        i += nb
    return kc, vc, bt


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 32, 8), (64, 8, 8), (128, 64, 8), (128, 16, 8), (64, 16, 4)])
@pytest.mark.parametrize("long_ctx", [False, True])
def test_decode_attn_fp8(cuda, D, Hq, Hkv, long_ctx):
    """tests/test_kernels_gpu.py::test_decode_attn's grid over fp8 caches (k_scale 0.5, v_scale 2.0)."""
    torch.manual_seed(12)
    ks, vs = 0.5, 2.0
    ctx = [1, 64, 300, 1000] + ([4100, 5000] if long_ctx else [])
    B = len(ctx)
    kc, vc, bt = _paged_setup8(B, Hkv, D, ctx, sum((c + 63) // 64 for c in ctx) + 8, ks, vs)
    q = rnd(B, Hq, D)
    lens = torch.tensor(ctx, dtype=torch.int32, device="cuda")
    want = ref.decode_attention(q, ops.dequant_kv_fp8(kc, ks, torch.float32), ops.dequant_kv_fp8(vc, vs, torch.float32),
                                bt, lens, 1 / math.sqrt(D))
    for splits in (1, 3):
        o = ops.decode_attention(q, kc, vc, bt, lens, num_splits=splits, k_scale=ks, v_scale=vs)
        close(o, want, 2e-2)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 8), (128, 16, 8), (128, 32, 8), (128, 64, 8), (64, 8, 8), (64, 16, 4)])
def test_split_decode_formats_agree(cuda, D, Hq, Hkv):
    """The split kernel is one body for both cache formats: over a bf16 cache whose every value is an e4m3 value and
    its fp8 twin (scales 1.0) the two formats do the same arithmetic in the same order -- widening a code to bf16 is
    exact -- so the outputs are equal bit for bit, and both meet the fp32 reference.  Every GQA group at D = 128 and
    two at D = 64; contexts around the 64-token block edge and up to 10 blocks (1 to 3 splits per sequence); 9
    splits at Hkv = 8 are 576 items, more than two per CU: the persistent walk with split rotation."""
    torch.manual_seed(23)
    ctx = [1, 63, 64, 65, 300, 520, 580, 600]
    B = len(ctx)
    k8, v8, bt = _paged_setup8(B, Hkv, D, ctx, sum((c + 63) // 64 for c in ctx) + 8, 1.0, 1.0)
    kb, vb = ops.dequant_kv_fp8(k8, 1.0, torch.bfloat16), ops.dequant_kv_fp8(v8, 1.0, torch.bfloat16)
    assert torch.equal(_u8(ops.quantize_kv_fp8(kb, 1.0)), _u8(k8))   # the bf16 cache holds the codes' values exactly
    q = rnd(B, Hq, D)
    lens = torch.tensor(ctx, dtype=torch.int32, device="cuda")
    want = ref.decode_attention(q, kb.float(), vb.float(), bt, lens, 1 / math.sqrt(D))
    prev = ops.set_decode_wb(-1)
    try:
        ops.set_decode_wb(0)   # D 128, group 4, one split: the bf16 cache takes the split kernel too
        for splits in (1, 3, 9):
            o8 = ops.decode_attention(q, k8, v8, bt, lens, num_splits=splits, k_scale=1.0, v_scale=1.0)
            ob = ops.decode_attention(q, kb, vb, bt, lens, num_splits=splits)
            close(o8, want, 2e-2)
            close(ob, want, 2e-2)
            diff = (o8.float() - ob.float()).abs()
            print(f"splits {splits}: fp8 vs bf16 cache: {int((o8 != ob).sum())} of {o8.numel()} elements differ, "
                  f"max |diff| {diff.max().item():.3g}")
            assert torch.equal(o8, ob)
    finally:
        ops.set_decode_wb(prev)


def test_decode_attention_rejects_unsupported_gqa_group(cuda):
    """The split kernel has instantiations for GQA groups 1, 2, 4 and 8; any other group (here 24 / 8 = 3) is
    rejected by the binding before a launch, for both cache formats."""
    D, Hq, Hkv = 128, 24, 8
    q = rnd(1, Hq, D)
    bt = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    lens = torch.ones(1, dtype=torch.int32, device="cuda")
    for dtype in (torch.bfloat16, F8):
        kc = torch.zeros(2, Hkv, 64, D, dtype=dtype, device="cuda")
        with pytest.raises(RuntimeError, match="1, 2, 4 and 8"):
            ops.decode_attention(q, kc, torch.zeros_like(kc), bt, lens)


@pytest.mark.parametrize("wb", [0, 1])
@pytest.mark.parametrize("source", ["qkv_rows", "partial_slabs"])
def test_decode_attn_fp8_fused(cuda, wb, source):
    """Fused step over fp8 caches at the shape of test_decode_attn_wave_per_block_matches_split_kernel (an fp8 cache
    takes the split kernel in both wave-per-block modes): the caches afterwards equal the fp8 rope_qkv_cache result
    bit for bit, the outputs meet the fp32 reference over the updated dequantised cache.  partial_slabs: q / k / v
    come from the skinny GEMM's split-K partials at K = 256, the smallest whole-step K (four 64-wide K steps) the
    skinny kernel splits."""
    torch.manual_seed(31)
    D, Hq, Hkv = 128, 32, 8
    ks, vs = 0.5, 2.0
    ctx = [1, 63, 64, 65, 256, 257, 17000, 5]
    B = len(ctx)
    kc, vc, bt = _paged_setup8(B, Hkv, D, ctx, sum((c + 63) // 64 for c in ctx) + 8, ks, vs)
    lens = torch.tensor(ctx, dtype=torch.int32, device="cuda")
    ang = torch.rand(max(ctx) + 1, D // 2, device="cuda") * 3
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    pos = lens - 1
    slots = torch.stack([bt[b, (c - 1) // 64] * 64 + (c - 1) % 64 for b, c in enumerate(ctx)]).int()
    slots[-1] = -1
    N = (Hq + 2 * Hkv) * D
    prev = ops.set_decode_wb(-1)
    try:
        ops.set_decode_wb(wb)
        k2, v2 = kc.clone(), vc.clone()
        if source == "qkv_rows":
            qkv = rnd(B, N)
            o = ops.decode_attention_rope(qkv.clone(), k2, v2, bt, lens, pos, cos, sin, slots, Hq, Hkv,
                                          num_splits=1, k_scale=ks, v_scale=vs)
        else:
            K, eps = 256, 1e-5
            x = rnd(B, K)
            w = rnd(N, K, scale=1 / math.sqrt(K))
            o = ops.decode_attention_rope_qkv(x, w, eps, k2, v2, bt, lens, pos, cos, sin, slots, Hq, Hkv,
                                              num_splits=1, k_scale=ks, v_scale=vs)
            # the same partials folded by the GEMM's own fold launch: the rows the kernel attended
            part = ops.gemm_partials(x, w, eps)
            kg = part.numel() // (B * (N + 1))
            assert kg >= 2
            qkv = torch.empty(B, N, device="cuda", dtype=torch.bfloat16)
            ops.gemm_into(x, w, qkv, force_cfg=1000 + kg, rms_eps=eps)
    finally:
        ops.set_decode_wb(prev)
    q2, k3, v3 = qkv.clone(), kc.clone(), vc.clone()
    ops.rope_qkv_cache(q2, pos, cos, sin, k3, v3, slots, Hq, Hkv, ks, vs)
    assert torch.equal(_u8(k2), _u8(k3)) and torch.equal(_u8(v2), _u8(v3))
    assert not torch.equal(_u8(k2), _u8(kc))   # the new tokens were written
    want = ref.decode_attention(q2[:, :Hq * D].reshape(B, Hq, D), ops.dequant_kv_fp8(k3, ks, torch.float32),
                                ops.dequant_kv_fp8(v3, vs, torch.float32), bt, lens, 1 / math.sqrt(D))
    close(o[:-1], want.reshape(B, Hq * D)[:-1], 2e-2)


def test_kv_dequant_blocks_and_binding_checks(cuda):
    torch.manual_seed(2)
    Hkv, D = 2, 128
    kc = ops.quantize_kv_fp8(rnd(9, Hkv, 64, D, scale=3), 0.3)
    vc = ops.quantize_kv_fp8(rnd(9, Hkv, 64, D, scale=3), 1.7)
    phys = torch.tensor([7, 0, 3], dtype=torch.int32, device="cuda")
    ko = torch.full((4, Hkv, 64, D), 9.0, dtype=torch.bfloat16, device="cuda")
    vo = ko.clone()
    ops.kv_dequant_blocks(kc, vc, phys, ko, vo, 0.3, 1.7)
    assert torch.equal(ko[:3], ops.dequant_kv_fp8(kc[phys.long()], 0.3, torch.bfloat16))
    assert torch.equal(vo[:3], ops.dequant_kv_fp8(vc[phys.long()], 1.7, torch.bfloat16))
    assert bool((ko[3] == 9).all())       # blocks past the list are untouched
    q = rnd(1, 4, D)
    bt = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    lens = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises((RuntimeError, ValueError), match="differ"):
        ops.decode_attention(q, kc, ko, bt, lens)
    wide = torch.zeros(2, 9, Hkv, 64, 2 * D, dtype=F8, device="cuda")
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.decode_attention(q, wide[0, ..., :D], wide[1, ..., :D], bt, lens)
    with pytest.raises(RuntimeError, match="D % 16"):
        ops.kv_write(rnd(1, Hkv, 8), rnd(1, Hkv, 8), torch.zeros(2, Hkv, 64, 8, dtype=F8, device="cuda"),
                     torch.zeros(2, Hkv, 64, 8, dtype=F8, device="cuda"), lens)
    with pytest.raises(RuntimeError, match="scratch capacity"):
        ops.kv_dequant_blocks(kc, vc, torch.arange(5, dtype=torch.int32, device="cuda"), ko, vo, 1.0, 1.0)


def test_paged_prefill_attn_fp8_through_scratch(cuda):
    """test_paged_prefill_attn's shapes over fp8 caches, once with the scratch sized by the op (one round) and once
    with a scratch of 5 blocks (sequence 0 needs 2, sequence 1 needs 5: two rounds)."""
    torch.manual_seed(13)
    D, Hq, Hkv = 128, 8, 2
    ks, vs = 0.5, 2.0
    ctx = [100, 300]
    q_lens = [37, 300]
    kc, vc, bt = _paged_setup8(2, Hkv, D, ctx, 64, ks, vs)
    q = rnd(2, 300, Hq, D)
    kl = torch.tensor(ctx, dtype=torch.int32, device="cuda")
    ql = torch.tensor(q_lens, dtype=torch.int32, device="cuda")
    orf = ref.paged_attention(q, ops.dequant_kv_fp8(kc, ks, torch.float32), ops.dequant_kv_fp8(vc, vs, torch.float32),
                              bt, kl, ql, 1 / math.sqrt(D))
    small = (torch.empty(5, Hkv, 64, D, dtype=torch.bfloat16, device="cuda"),
             torch.empty(5, Hkv, 64, D, dtype=torch.bfloat16, device="cuda"))
    assert len(ops.plan_kv_scratch([2, 5], 5)) == 2
    for scratch in (None, small):
        o = ops.paged_attention(q, kc, vc, bt, kl, ql, k_scale=ks, v_scale=vs, scratch=scratch)
        close(o[0, :37], orf[0, :37], 2e-2)
        close(o[1], orf[1], 2e-2)


def test_paged_attention_varlen_fp8_through_scratch(cuda):
    """tests/test_varlen_gpu.py's packed step (prefill chunks and decode rows, D 128) over fp8 caches; the second
    pass forces three rounds with a scratch just large enough for the longest sequence."""
    torch.manual_seed(0)
    D, Hq, Hkv = 128, 8, 2
    ks, vs = 0.5, 2.0
    n_cached = [0, 130, 0, 5000, 63]
    n_new = [64, 1, 8192, 700, 1]
    blocks_per = [(c + n + 63) // 64 for c, n in zip(n_cached, n_new)]
    nblk = sum(blocks_per) + 4
    kc = ops.quantize_kv_fp8(rnd(nblk, Hkv, 64, D, scale=0.5), ks)
    vc = ops.quantize_kv_fp8(rnd(nblk, Hkv, 64, D), vs)
    perm = torch.randperm(nblk).tolist()
    bt = torch.zeros(len(n_new), max(blocks_per), dtype=torch.int32)
    o = 0
    for i, nb in enumerate(blocks_per):
        bt[i, :nb] = torch.tensor(perm[o:o + nb])
        o += nb
    bt = bt.cuda()
    T = sum(n_new)
    q = rnd(T, Hq, D)
    q_start = torch.tensor([sum(n_new[:i]) for i in range(len(n_new))], dtype=torch.int32, device="cuda")
    kv_lens = torch.tensor([c + n for c, n in zip(n_cached, n_new)], dtype=torch.int32, device="cuda")
    q_lens = torch.tensor(n_new, dtype=torch.int32, device="cuda")
    want = ref.paged_attention_varlen(q.float(), ops.dequant_kv_fp8(kc, ks, torch.float32),
                                      ops.dequant_kv_fp8(vc, vs, torch.float32), bt, kv_lens, q_lens, q_start,
                                      1.0 / D ** 0.5, True)
    cap = max(blocks_per)
    small = (torch.empty(cap, Hkv, 64, D, dtype=torch.bfloat16, device="cuda"),
             torch.empty(cap, Hkv, 64, D, dtype=torch.bfloat16, device="cuda"))
    assert len(ops.plan_kv_scratch(blocks_per, cap)) == 3
    for scratch in (None, small):
        got = ops.paged_attention_varlen(q, kc, vc, bt, kv_lens, q_lens, q_start, max(n_new), k_scale=ks, v_scale=vs,
                                         scratch=scratch)
        close(got, want, 2e-2)


def _run_engine(eng, prompts, n_dec, forced=None):
    """tests/test_mxfp4_gpu.py's pattern: greedy generation recording every step's logits; ``forced`` replaces each
    step's appended tokens, so both engines see the same sequences."""
    from shai_amd.engines.llm import SamplingParams
    rec = []
    fwd = eng.model.forward
    eng.model.forward = lambda *a, **k: (lambda y: (rec.append(y.float().clone()), y)[1])(fwd(*a, **k))
    p = SamplingParams(max_tokens=n_dec, temperature=0.0, ignore_eos=True)
    seqs = [eng.add_request(pr, p) for pr in prompts]
    row = {id(s): i for i, s in enumerate(seqs)}
    if forced is not None:
        app = eng._append
        eng._append = lambda ss, toks: app(ss, [forced[row[id(q)]][len(q.output)] for q in ss])
    while not all(q.finished for q in seqs):
        eng.step()
    return rec, [q.output for q in seqs]


def test_fp8_kv_llm_engine(cuda):
    """Eager GPU fp8-KV engine against a CPU fp8-KV engine (same weights, forced tokens): per-step logit rel below
    3e-2, the quantised-engine bound of tests/test_mxfp4_gpu.py; then the default engine (graphs, look-ahead) on its
    greedy tokens, a chunked prefill with mixed steps through a scratch too small for one round, and the block pool
    back to full.  Measured: fp8 KV 0.020 - 0.030 per step (largest 0.0299), bf16 KV 0.0085 - 0.0105 for the same
    GPU-vs-CPU comparison (printed for context) -- an element that differs by a bf16 ulp between the two engines
    can land on the neighbouring e4m3 code, a 2^-3 relative step."""
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    c = LlamaConfig.tiny()
    kw = dict(max_num_seqs=4, max_model_len=256, seed=1, enable_prefix_caching=False)
    prompts = [[3, 17, 99, 250, 7], [5, 6, 7, 8, 9, 10, 11]]
    n_dec = 8   # prefill + 7 decode steps
    figs = {}
    for kvd in ("fp8", "auto"):
        eg = LLMEngine(c, device=cuda, kv_cache_dtype=kvd, use_graphs=False, async_decode=False, **kw)
        ec = LLMEngine(c, device="cpu", kv_cache_dtype=kvd, **kw)
        ec.model.load_state_dict({k: v.cpu() for k, v in eg.model.state_dict().items()})
        ec.model._folded = True   # the GPU engine's weights are already folded
        assert eg.kv_buf.dtype == ec.kv_buf.dtype == (torch.float8_e4m3fn if kvd == "fp8" else torch.bfloat16)
        ref_logits, ref_toks = _run_engine(ec, prompts, n_dec)
        got_logits, got_toks = _run_engine(eg, prompts, n_dec, forced=ref_toks)
        assert got_toks == ref_toks and len(got_logits) == len(ref_logits) == n_dec
        figs[kvd] = [_rel(g, r) for g, r in zip(got_logits, ref_logits)]
        print(f"kv {kvd}: per-step GPU-vs-CPU logits rel", [round(x, 5) for x in figs[kvd]])
        assert eg.bm.num_free == eg.num_kv_blocks
        if kvd == "fp8":
            fp8_ref = (ref_logits, ref_toks)
    for i, rel in enumerate(figs["fp8"]):
        assert rel < 3e-2, (i, rel)
    ref_logits, ref_toks = fp8_ref
    # defaults: HIP-graph decode and async look-ahead.  Free-running greedy tokens follow the reference's; a step may
    # differ only where the reference's own margin between the two tokens is inside the logit tolerance above
    # (2 x 3e-2 of the row's largest logit), and the comparison ends there (the sequences differ from then on).
    ed = LLMEngine(c, device=cuda, kv_cache_dtype="fp8", **kw)
    assert ed.use_graphs and ed.async_decode and ed.kv_buf.dtype == torch.float8_e4m3fn
    out = [s.output for s in ed.generate(prompts, SamplingParams(max_tokens=n_dec, temperature=0.0, ignore_eos=True))]
    assert all(len(o) == n_dec and all(0 <= t < c.vocab_size for t in o) for o in out)
    for b, (o, want) in enumerate(zip(out, ref_toks)):
        for t in range(n_dec):
            if o[t] == want[t]:
                continue
            rowl = ref_logits[t][b]
            margin = (rowl[want[t]] - rowl[o[t]]).item()
            assert margin <= 2 * 3e-2 * rowl.abs().max().item(), (b, t, o, want, margin)
            break
    assert ed.bm.num_free == ed.num_kv_blocks
    # a prompt longer than prefill_chunk beside a running sequence: chunked prefill and mixed steps, with a scratch
    # too small for the step's blocks in one round
    ex = LLMEngine(c, device=cuda, kv_cache_dtype="fp8", prefill_chunk=64, kv_scratch_blocks=5, **kw)
    assert ex.kv_scratch_blocks == 5
    p = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    first, second = ex.add_request([9, 8, 7, 6], p), ex.add_request([1, 2, 3], p)
    ex.step()
    long_ = ex.add_request([(7 * i) % 200 + 10 for i in range(200)], p)
    kinds = []
    pre = ex._prefill
    ex._prefill = lambda seqs, rows=(): (kinds.append((len(seqs), len(list(rows)))), pre(seqs, rows))[1]
    att, nrounds = ex._attach_kv_rounds, []
    ex._attach_kv_rounds = lambda batch, *a: (att(batch, *a), nrounds.append(len(batch.kv_rounds)))[0]
    while not (first.finished and second.finished and long_.finished):
        ex.step()
    assert len(kinds) >= 4 and any(r > 0 for _, r in kinds), kinds   # 200 tokens in 64-token chunks; mixed steps
    assert max(nrounds) >= 2, nrounds   # 4 + 1 + 1 blocks do not fit the 5-block scratch in one round
    assert len(first.output) == len(second.output) == len(long_.output) == 6
    assert ex.bm.num_free == ex.num_kv_blocks
