"""NF4 tile GEMM (csrc/kernels/gemm_nf4.hip): nf4 weights above 64 activation rows without a dequantise pass, behind
``ops.NF4_PREFILL = "fused"``.  References are the CPU table decode and fp64, never the kernel under test."""
import pytest
import torch

from shai_amd import ops
from gemm_exact import act64, assert_smooth, to_bf16_exact
from nf4_cases import nf4_case, random_packed, random_quantised, rel, run_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fused(monkeypatch):
    monkeypatch.setattr(ops, "NF4_PREFILL", "fused")


@pytest.mark.parametrize("cfg", [-1, 1301, 1333, 1302])
def test_widening_is_the_oracle(cuda, cfg):
    """X = rows of the identity: output row m is column k_m of the dequantised weights, bit for bit (one product per
    output, exact under any split).  K = 320 = 2.5 steps of 128; the 96 k cover both nibbles, the ends of blocks and
    steps, and the half-filled last step."""
    M, N, K = 96, 160, 320
    ks = [0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 254, 255, 256, 257, 318, 319]
    ks += [k for k in range(2, K, 3) if k not in ks][:M - len(ks)]
    assert len(set(ks)) == M
    wq, am, wd = random_packed(N, K, seed=9)   # absmax with all 24 significant bits
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), torch.tensor(ks)] = 1.0
    y = ops.linear(x.to(cuda), wq.to(cuda), w_scale=am.to(cuda), force_cfg=cfg)
    assert torch.equal(y.cpu(), wd[:, ks].t())


EXACT = [(m, n, k, cfg) for (m, n, k) in [(65, 96, 64), (130, 320, 1088), (257, 200, 2048)]
         for cfg in (1301, 1333, 1302, 1304, 1334) if (cfg - 1300) % 32 <= (k + 127) // 128]   # a K step per K group


@pytest.mark.parametrize("M,N,K,cfg", EXACT)
def test_exact_gemm(cuda, M, N, K, cfg):
    """absmax in {0.5, 1, 2} and x in {-1, 0, 1}: every weight is a multiple of 2^-12 and every sum of |terms| below
    2^24 of that unit, so the fp32 accumulation is exact in any order and the output must be bf16(fp64 result)."""
    g = torch.Generator().manual_seed(M + N + K)
    absmax = 2.0 ** torch.randint(-1, 2, (N, K // 64), generator=g).float()
    codes, absmax, w = nf4_case(N, K, seed=M + N, absmax=absmax)
    wq, am = ops.quantize_nf4(w)
    assert torch.equal(ops.nf4_unpack(wq, am)[0], codes)
    x = torch.randint(-1, 2, (M, K), generator=g).bfloat16()
    b = torch.randint(-4, 5, (N,), generator=g).bfloat16()
    r = torch.randint(-8, 9, (M, N), generator=g).bfloat16()
    wd = ops.dequant_nf4(wq, am).double()
    assert float((x.double().abs() @ wd.abs().t() + b.double().abs() + r.double().abs()).max()) < 4096
    want = to_bf16_exact(x.double() @ wd.t() + b.double() + r.double())
    y = ops.linear(x.to(cuda), wq.to(cuda), b.to(cuda), residual=r.to(cuda), w_scale=am.to(cuda), force_cfg=cfg)
    bad = (y.cpu() != want).nonzero()
    assert bad.numel() == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("cfg", [-1, 1333, 1302])
def test_glu_rms_silu(cuda, cfg):
    """The rule and terms of test_skinny_glu_rms_silu: rstd is applied in fp32 in the tile kernel's epilogue (an
    explicit row-norm pass would round the normalised activations to bf16 and miss this bound: 1.33 ulp measured).
    The route's choice, the 256-row tile, and a split whose row sums of squares go through the fold."""
    M = 200
    wq, am, wd = random_quantised(2 * 192, 1024, seed=11)
    x = (torch.randn(M, 1024, generator=torch.Generator().manual_seed(M)) * 3).bfloat16()
    y = ops.linear(x.to(cuda), wq.to(cuda), act="silu", glu=True, rms_eps=1e-5, w_scale=am.to(cuda), force_cfg=cfg)
    xn = x.double() * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + 1e-5)
    z = xn @ wd.double().t()
    terms = xn.abs() @ wd.double().abs().t()   # sum of |terms| of each pre-activation
    assert_smooth(y, z[:, 0::2] * act64(z[:, 1::2], "silu"), terms[:, 0::2] * terms[:, 1::2].clamp_min(1),
                  f"glu + rms + silu M={M}")


def test_strided_rows_and_column_slice(cuda):
    """x = every second row of a buffer, out and residual column slices of wider buffers (ldc, ldr > N): the result
    is right and the neighbouring columns keep their sentinel."""
    torch.manual_seed(9)
    M, N, K = 150, 200, 320
    wq, am, wd = random_quantised(N, K, seed=9)
    buf = torch.randn(2 * M, K).bfloat16()
    b = torch.randn(N).bfloat16()
    rwide = torch.randn(M, N + 24).bfloat16()
    want = buf[::2].float() @ wd.float().t() + b.float() + rwide[:, 8:8 + N].float()
    x = buf.to(cuda)[::2]
    res = rwide.to(cuda)[:, 8:8 + N]
    wide = torch.full((M, N + 64), 777.0, device=cuda, dtype=torch.bfloat16)
    out = wide[:, 32:32 + N]
    assert x.stride(0) == 2 * K and out.stride(0) == N + 64
    ops.gemm_into(x, wq.to(cuda), out, b.to(cuda), residual=res, w_scale=am.to(cuda))
    err = rel(out, want)
    print("nf4 tile strided rel", err)
    assert err < 1e-2
    assert bool((wide[:, :32] == 777.0).all()) and bool((wide[:, 32 + N:] == 777.0).all())


def _no_dequant(*a, **k):
    raise AssertionError("ops.dequant_nf4 called: the GEMM fell back to the dequantise route")


def test_route(cuda, monkeypatch):
    wq, am, wd = random_quantised(512, 1024, seed=3)
    wg, sg = wq.to(cuda), am.to(cuda)
    x = torch.randn(300, 1024, generator=torch.Generator().manual_seed(3)).bfloat16()
    xg, want = x.to(cuda), x.double() @ wd.double().t()
    out = torch.empty(300, 512, device=cuda, dtype=torch.bfloat16)
    monkeypatch.setattr(ops, "dequant_nf4", _no_dequant)
    assert rel(ops.linear(xg, wg, w_scale=sg), want) < 1e-2            # above 64 rows: the tile kernel
    y = ops.linear(xg.view(3, 100, 1024), wg, w_scale=sg)              # flattenable leading dims
    assert y.shape == (3, 100, 512) and rel(y.view(300, 512), want) < 1e-2
    with pytest.raises(AssertionError, match="dequantise route"):      # a gate still dequantises
        ops.gemm_into(xg, wg, out, gate=torch.ones(300, 512, device=cuda, dtype=torch.bfloat16), w_scale=sg)
    with pytest.raises(AssertionError, match="dequantise route"):      # a folded LayerNorm still dequantises
        ops.linear(xg, wg, w_scale=sg, row_affine=(torch.zeros(300, 2, device=cuda), torch.zeros(512, device=cuda)))
    with pytest.raises(RuntimeError, match="force_cfg"):               # a skinny number above 64 rows
        ops.gemm_into(xg, wg, out, w_scale=sg, force_cfg=1001)
    with pytest.raises(RuntimeError, match="force_cfg"):               # a tile number at 8 rows
        ops.gemm_into(xg[:8], wg, out[:8], w_scale=sg, force_cfg=1300)
    monkeypatch.undo()                                                 # the switch at its default: dequantise
    assert ops.NF4_PREFILL == "dequant"
    monkeypatch.setattr(ops, "dequant_nf4", _no_dequant)
    with pytest.raises(AssertionError, match="dequantise route"):
        ops.linear(xg, wg, w_scale=sg)
    assert rel(ops.linear(xg[:64], wg, w_scale=sg), want[:64]) < 1e-2  # 64 rows never depend on the switch


def test_engine(cuda, monkeypatch):
    """One packed 95-row prefill, then decode steps with 72 sequences (a 72-row GEMM or its size bucket), eager,
    against a bf16 engine carrying the dequantised weights; then the default graph + async engine."""
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    from shai_amd.parallel.layers import FP8_LAYER_TYPES
    c = LlamaConfig.tiny()
    kw = dict(device=cuda, max_num_seqs=80, max_model_len=256, seed=1, enable_prefix_caching=False)
    e4 = LLMEngine(c, quantization="nf4", use_graphs=False, async_decode=False, **kw)
    e16 = LLMEngine(c, use_graphs=False, async_decode=False, **kw)
    q = {n: m for n, m in e4.model.named_modules() if isinstance(m, FP8_LAYER_TYPES)}
    assert q and all(m.weight.dtype == torch.uint8 for m in q.values())
    for n, m in e16.model.named_modules():
        if isinstance(m, FP8_LAYER_TYPES):
            m.weight.data.copy_(ops.dequant_nf4(q[n].weight, q[n].w_scale))
    monkeypatch.setattr(ops, "dequant_nf4", _no_dequant)
    n_dec = 4
    packed = [[(7 * i + 3) % c.vocab_size for i in range(50)], [(11 * i + 5) % c.vocab_size for i in range(45)]]
    many = [[(5 * b + 13 * i + 1) % c.vocab_size for i in range(3 + b % 4)] for b in range(72)]
    hooks = e16.model.forward, e4.model.forward, e4._append   # run_engine wraps them per call
    for prompts in (packed, many):
        e16.model.forward, e4.model.forward, e4._append = hooks
        ref_logits, ref_toks = run_engine(e16, prompts, n_dec)
        got_logits, got_toks = run_engine(e4, prompts, n_dec, forced=ref_toks)
        assert got_toks == ref_toks and len(got_logits) == len(ref_logits)
        for i, (g, r) in enumerate(zip(got_logits, ref_logits)):
            err = rel(g, r)
            print("nf4 tile engine", len(prompts), "step", i, "logits rel", err)
            assert g.shape == r.shape and err < 3e-2, i
    # defaults (HIP-graph decode, async look-ahead) on the 72 prompts: greedy tokens follow the reference's; a step may
    # differ only where the reference's own margin between the two tokens is inside the logit tolerance above
    ed = LLMEngine(c, quantization="nf4", **kw)
    assert ed.use_graphs and ed.async_decode
    out = [s.output for s in ed.generate(many, SamplingParams(max_tokens=n_dec, temperature=0.0, ignore_eos=True))]
    dec_logits = ref_logits[-n_dec:]
    for b, (o, want) in enumerate(zip(out, ref_toks)):
        assert len(o) == n_dec
        for t in range(n_dec):
            if o[t] != want[t]:
                rowl = dec_logits[t][b]
                assert (rowl[want[t]] - rowl[o[t]]).item() <= 2 * 3e-2 * rowl.abs().max().item(), (b, t, o, want)
                break
