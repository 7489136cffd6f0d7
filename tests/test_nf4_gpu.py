"""NF4 weight-only path on the GPU: the dequantise kernel and the widening inside the skinny decode GEMM
(csrc/kernels/gemv_nf4.hip) bit-equal to the CPU table decode, an exact GEMM over every forced split-K form, the
GLU + folded RMSNorm + SiLU epilogue against fp64, the dequantise route above 64 rows, and an NF4 LLM engine against a
bf16 engine carrying the dequantised weights."""
import pytest
import torch

from shai_amd import ops
from gemm_exact import act64, assert_smooth, to_bf16_exact
from nf4_cases import nf4_case, random_packed, random_quantised, rel, run_engine

pytestmark = pytest.mark.gpu


def test_dequant_kernel_is_the_table_decode(cuda):
    # every code under absmax 0, random fp32 values, and values that put TABLE[c] * absmax next to a bf16 rounding tie
    table = torch.tensor(ops.NF4_TABLE, dtype=torch.float32)
    tie = torch.tensor(1.00390625)   # 1 + 2^-8: halfway between the bf16 numbers 1 and 1 + 2^-7
    near = torch.stack([torch.nextafter(tie / table[c].abs(), torch.tensor(d)) for c in (1, 6, 8, 14)
                        for d in (0.0, 4.0)] + [tie, tie * 2])
    g = torch.Generator().manual_seed(0)
    absmax = torch.cat([torch.zeros(2), near, torch.rand(12, generator=g) * 3 + 1e-3,
                        torch.rand(8, generator=g) * 1e-3 + 1e-6]).view(4, 8)
    codes = (torch.arange(4 * 512) % 16).to(torch.uint8).view(4, 512)
    wq, am = ops.nf4_pack(codes, absmax)
    got = ops.dequant_nf4(wq.to(cuda), am.to(cuda))
    assert got.dtype == torch.bfloat16 and got.is_cuda
    assert torch.equal(got.cpu(), ops.dequant_nf4(wq, am))
    wq, am, want = random_quantised(256, 512, seed=4)
    assert torch.equal(ops.dequant_nf4(wq.to(cuda), am.to(cuda)).cpu(), want)


def test_skinny_widening_is_the_oracle(cuda):
    """X = rows of the identity: output row m is column k_m of the dequantised weights, bit for bit.  K = 320 = 2.5
    steps of 128; the 64 k cover both nibbles, the ends of blocks and steps, and the half-filled last step."""
    M, N, K = 64, 160, 64 * 5
    ks = [0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 254, 255, 256, 257, 318, 319]
    ks += [k for k in range(2, K, 5) if k not in ks][:M - len(ks)]
    assert len(set(ks)) == M
    wq, am, wd = random_packed(N, K, seed=9)   # absmax with all 24 significant bits
    assert bool(((ops.nf4_unpack(wq, am)[1].view(torch.int32) & 0xffff) != 0).float().mean() > 0.9)   # not bf16 numbers
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), torch.tensor(ks)] = 1.0
    y = ops.linear(x.to(cuda), wq.to(cuda), w_scale=am.to(cuda))
    assert torch.equal(y.cpu(), wd[:, ks].t())


EXACT = [(m, n, k, cfg) for (m, n, k) in [(1, 128, 256), (5, 96, 64), (33, 320, 2048), (64, 200, 1088)]
         for cfg in (-1, 1001, 1004, 1104) if cfg < 0 or cfg % 100 <= max(1, k // 128)]   # a K step per K group


@pytest.mark.parametrize("M,N,K,cfg", EXACT)
def test_skinny_exact_gemm(cuda, M, N, K, cfg):
    """absmax in {0.5, 1, 2} and x in {-1, 0, 1}: every weight is a multiple of 2^-12 and every partial sum below
    2^24 of that unit, so the fp32 accumulation is exact in any order and the output must be bf16(fp64 result)."""
    g = torch.Generator().manual_seed(M + N + K)
    absmax = 2.0 ** torch.randint(-1, 2, (N, K // 64), generator=g).float()
    codes, absmax, w = nf4_case(N, K, seed=M + N, absmax=absmax)
    wq, am = ops.quantize_nf4(w)
    assert torch.equal(ops.nf4_unpack(wq, am)[0], codes)
    x = torch.randint(-1, 2, (M, K), generator=g).bfloat16()
    b = torch.randint(-4, 5, (N,), generator=g).bfloat16()
    r = torch.randint(-8, 9, (M, N), generator=g).bfloat16()
    want = to_bf16_exact(x.double() @ ops.dequant_nf4(wq, am).double().t() + b.double() + r.double())
    y = ops.linear(x.to(cuda), wq.to(cuda), b.to(cuda), residual=r.to(cuda), w_scale=am.to(cuda), force_cfg=cfg)
    bad = (y.cpu() != want).nonzero()
    assert bad.numel() == 0, (len(bad), bad[:5].tolist())


@pytest.fixture(scope="module")
def glu_weights():
    return random_quantised(2 * 192, 1024, seed=11)


@pytest.mark.parametrize("M", [1, 17, 64])
def test_skinny_glu_rms_silu(cuda, glu_weights, M):
    wq, am, wd = glu_weights
    x = (torch.randn(M, 1024, generator=torch.Generator().manual_seed(M)) * 3).bfloat16()
    y = ops.linear(x.to(cuda), wq.to(cuda), act="silu", glu=True, rms_eps=1e-5, w_scale=am.to(cuda))
    xn = x.double() * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + 1e-5)
    z = xn @ wd.double().t()
    terms = xn.abs() @ wd.double().abs().t()   # sum of |terms| of each pre-activation
    assert_smooth(y, z[:, 0::2] * act64(z[:, 1::2], "silu"), terms[:, 0::2] * terms[:, 1::2].clamp_min(1),
                  f"glu + rms + silu M={M}")


def test_route_above_64_rows_dequantises(cuda):
    wq, am, wd = random_quantised(512, 1024, seed=3)
    x = torch.randn(80, 1024, generator=torch.Generator().manual_seed(3)).bfloat16()
    y = ops.linear(x.to(cuda), wq.to(cuda), w_scale=am.to(cuda))
    err = rel(y, x.double() @ wd.double().t())
    print("route above 64 rows rel", err)
    assert err < 1e-2


def test_nf4_llm_engine(cuda):
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    from shai_amd.parallel.layers import FP8_LAYER_TYPES
    c = LlamaConfig.tiny()
    kw = dict(device=cuda, max_num_seqs=4, max_model_len=256, seed=1, enable_prefix_caching=False)
    prompts = [[3, 17, 99, 250, 7], [5, 6, 7, 8, 9, 10, 11]]
    n_dec = 8   # prefill + 7 decode steps
    e4 = LLMEngine(c, quantization="bitsandbytes", use_graphs=False, async_decode=False, **kw)
    gu = e4.model.layers[0].mlp.gate_up_proj
    assert e4.quantization == "nf4" and gu.weight.dtype == torch.uint8
    assert e4.model.embed_tokens.weight.dtype == torch.bfloat16 and e4.model.lm_head.weight.dtype == torch.bfloat16
    e16 = LLMEngine(c, use_graphs=False, async_decode=False, **kw)
    q = {n: m for n, m in e4.model.named_modules() if isinstance(m, FP8_LAYER_TYPES)}
    for n, m in e16.model.named_modules():
        if isinstance(m, FP8_LAYER_TYPES):
            m.weight.data.copy_(ops.dequant_nf4(q[n].weight, q[n].w_scale))
    ref_logits, ref_toks = run_engine(e16, prompts, n_dec)
    got_logits, got_toks = run_engine(e4, prompts, n_dec, forced=ref_toks)
    assert got_toks == ref_toks and len(got_logits) == len(ref_logits) == n_dec
    for i, (g, r) in enumerate(zip(got_logits, ref_logits)):
        err = rel(g, r)
        print("engine step", i, "logits rel", err)
        assert g.shape == r.shape and err < 3e-2, i
    # defaults (HIP-graph decode, async look-ahead): greedy tokens follow the reference's; a step may differ only where
    # the reference's own margin between the two tokens is inside the logit tolerance above, and the comparison ends
    ed = LLMEngine(c, quantization="nf4", **kw)
    assert ed.use_graphs and ed.async_decode
    out = [s.output for s in ed.generate(prompts, SamplingParams(max_tokens=n_dec, temperature=0.0, ignore_eos=True))]
    for b, (o, want) in enumerate(zip(out, ref_toks)):
        assert len(o) == n_dec
        for t in range(n_dec):
            if o[t] != want[t]:
                rowl = ref_logits[t][b]
                assert (rowl[want[t]] - rowl[o[t]]).item() <= 2 * 3e-2 * rowl.abs().max().item(), (b, t, o, want)
                break
