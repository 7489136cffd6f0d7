"""MXFP4 weight-only quantisation on the CPU: the quantiser's scale rule and rounding, the exact decode table, the
dequantise route of ``ops.linear``, model quantisation and a CPU engine against its dequantised weights."""
import pytest
import torch

from shai_amd import ops
from shai_amd.ops import reference as ref

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def group_scaled_weights(n, k, seed, device="cpu"):
    """randn / sqrt(K) with every 32-group multiplied by 2^randint(-6, 7): a wrong group or row index in a scale
    fetch cannot hide."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k // 32, 32, generator=g) / k ** 0.5
    e = torch.randint(-6, 7, (n, k // 32, 1), generator=g)
    return torch.ldexp(w, e).reshape(n, k).bfloat16().to(device)


def all_codes_case():
    """Packed bytes holding all 256 values (every code in both nibbles), 16 rows x 32 bytes = 2 groups per row, with
    group scales at exponents -20, -1, 0, 3 and 15; returns (wq, scales, expected fp32 [16, 64])."""
    codes = torch.arange(256, dtype=torch.uint8).reshape(16, 16).repeat(1, 2)          # [16, 32] bytes, K = 64
    exps = torch.tensor([-20, -1, 0, 3, 15], dtype=torch.int32)
    e = exps[(torch.arange(16)[:, None] * 2 + torch.arange(2)[None, :]) % 5]          # [16, 2]
    wq, scales = ops.mxfp4_pack(codes, (e + 127).to(torch.uint8))
    want = torch.empty(16, 64, dtype=torch.float32)
    for n in range(16):
        for kb in range(32):
            b = int(codes[n, kb])
            for h, code in enumerate((b & 15, b >> 4)):                               # even k: low nibble
                mag = E2M1[code & 7] * 2.0 ** int(e[n, (2 * kb + h) // 32])
                want[n, 2 * kb + h] = -mag if code & 8 else mag
    return wq, scales, want


def test_round_trip_error():
    torch.manual_seed(0)
    w = (torch.randn(512, 4096) / 64).bfloat16()
    wq, s = ops.quantize_mxfp4(w)
    assert wq.dtype == torch.float4_e2m1fn_x2 and wq.shape == (512, 2048)
    assert s.dtype == torch.float8_e8m0fnu and s.numel() == 512 * 4096 // 32
    d = ops.dequant_mxfp4(wq, s)
    assert d.dtype == torch.bfloat16 and d.shape == w.shape
    rel = ((d.float() - w.float()).norm() / w.float().norm()).item()
    print("round-trip rel", rel)
    assert rel < 0.13


def test_requantise_is_idempotent():
    w = group_scaled_weights(96, 512, seed=1)
    w[5, 64:96] = 0          # an all-zero group
    w[7] = 0                 # an all-zero row
    wq, s = ops.quantize_mxfp4(w)
    d = ops.dequant_mxfp4(wq, s)
    assert not d[5, 64:96].any() and not d[7].any()
    wq2, s2 = ops.quantize_mxfp4(d)
    torch.testing.assert_close(ops.dequant_mxfp4(wq2, s2).float(), d.float(), atol=0, rtol=0)
    assert torch.equal(wq2.view(torch.uint8), wq.view(torch.uint8))
    # and the dequantised values are exact in bf16: fp32 and bf16 decodes agree
    torch.testing.assert_close(ops.dequant_mxfp4(wq, s, dtype=torch.float32), d.float(), atol=0, rtol=0)


def test_exact_decode_table():
    wq, scales, want = all_codes_case()
    got = ops.dequant_mxfp4(wq, scales, dtype=torch.float32)
    torch.testing.assert_close(got, want, atol=0, rtol=0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))                  # -0 codes keep their sign
    b16 = ops.dequant_mxfp4(wq, scales)
    assert torch.equal(b16.view(torch.int16), want.bfloat16().view(torch.int16))
    torch.testing.assert_close(b16.float(), want, atol=0, rtol=0)                      # every value is exact in bf16
    codes, sb = ops.mxfp4_unpack(wq, scales)                                           # the layout helper inverts
    assert torch.equal(codes[:, :16].reshape(-1), torch.arange(256, dtype=torch.uint8)) and sb.shape == (16, 2)


def test_rounding_ties_to_even_and_clamp():
    # one group: amax 6 -> e = 0; midpoints go to the even mantissa (0, 1, 2, 4), values past 6 cannot occur
    vals = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, -0.25, -0.75, -2.5, -5.0, 0.26, 0.74, 5.25, 0.0]
    w = torch.tensor(vals + [0.0] * 16).reshape(1, 32).bfloat16()
    d = ops.dequant_mxfp4(*ops.quantize_mxfp4(w)).float()[0, :16]
    want = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0, 0.0, -1.0, -2.0, -4.0, 0.5, 0.5, 6.0, 0.0])
    torch.testing.assert_close(d, want, atol=0, rtol=0)
    # amax 7.5 = 1.875 * 2^2 -> e = 0 as well: clamped to 6
    w2 = torch.tensor([7.5, -7.0] + [0.0] * 30).reshape(1, 32).bfloat16()
    d2 = ops.dequant_mxfp4(*ops.quantize_mxfp4(w2)).float()[0, :2]
    torch.testing.assert_close(d2, torch.tensor([6.0, -6.0]), atol=0, rtol=0)


@pytest.mark.parametrize("M", [80, 5])
def test_cpu_linear_is_the_dequantised_linear(M):
    w = group_scaled_weights(64, 256, seed=2)
    wq, s = ops.quantize_mxfp4(w)
    x = torch.randn(M, 256, generator=torch.Generator().manual_seed(M)).bfloat16()
    b = torch.randn(64, generator=torch.Generator().manual_seed(3)).bfloat16()
    got = ops.linear(x, wq, b, act="silu", glu=True, w_scale=s)
    want = ref.linear(x, ops.dequant_mxfp4(wq, s), b, "silu", glu=True)
    torch.testing.assert_close(got.float(), want.float(), atol=0, rtol=0)
    out = torch.empty(M, 64, dtype=torch.bfloat16)
    ops.gemm_into(x, wq, out, w_scale=s)
    torch.testing.assert_close(out.float(), ref.linear(x, ops.dequant_mxfp4(wq, s)).float(), atol=0, rtol=0)


def test_model_quantisation():
    from shai_amd.models.layers import init_random_
    from shai_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from shai_amd.parallel.layers import FP8_LAYER_TYPES, quantize_mxfp4_
    m = LlamaForCausalLM(LlamaConfig.tiny())
    init_random_(m, 0)
    m.layers[1].mlp.no_fp8 = True
    skipped = {id(c) for c in m.layers[1].mlp.modules()}
    lin = [l for l in m.modules() if isinstance(l, FP8_LAYER_TYPES)]
    shapes = {id(l): tuple(l.weight.shape) for l in lin}
    n = quantize_mxfp4_(m)
    assert n == len(lin) - sum(id(l) in skipped for l in lin) and n > 0
    for l in lin:
        if id(l) in skipped:
            assert l.weight.dtype == torch.bfloat16 and l.w_scale is None
        else:
            N, K = shapes[id(l)]
            assert l.weight.dtype == torch.float4_e2m1fn_x2 and tuple(l.weight.shape) == (N, K // 2)
            assert l.w_scale is not None and l.w_scale.numel() >= N * K // 32
    assert m.embed_tokens.weight.dtype == torch.bfloat16 and m.lm_head.weight.dtype == torch.bfloat16
    before = [l.weight.view(torch.uint8).clone() for l in lin if id(l) not in skipped]
    quantize_mxfp4_(m)   # a second call is a no-op
    after = [l.weight.view(torch.uint8) for l in lin if id(l) not in skipped]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    with pytest.raises(RuntimeError, match="MXFP4"):
        m.fold_norms()


def test_row_parallel_shard_must_hold_whole_groups():
    from shai_amd.parallel.layers import RowParallelLinear
    l = RowParallelLinear(48, 64, bias=False)
    l.weight.data.normal_()
    with pytest.raises(ValueError, match="multiple of the MXFP4 group size 32"):
        l.quantize_mxfp4_()


def test_engine_rejects_unknown_quantization_and_names_mxfp4():
    from shai_amd.engines.llm import LLMEngine
    from shai_amd.models.llama import LlamaConfig
    with pytest.raises(ValueError, match="mxfp4"):
        LLMEngine(LlamaConfig.tiny(), device="cpu", max_num_seqs=2, max_model_len=128, quantization="int3")


def test_cpu_engine_matches_dequantised_weights():
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    from shai_amd.parallel.layers import FP8_LAYER_TYPES
    c = LlamaConfig.tiny()
    kw = dict(device="cpu", max_num_seqs=2, max_model_len=256, seed=1, enable_prefix_caching=False)
    e4 = LLMEngine(c, quantization="mxfp4", **kw)
    e16 = LLMEngine(c, **kw)
    assert e4.quantization == "mxfp4"
    q = {n: m for n, m in e4.model.named_modules() if isinstance(m, FP8_LAYER_TYPES)}
    assert q and all(m.weight.dtype == torch.float4_e2m1fn_x2 for m in q.values())
    for n, m in e16.model.named_modules():
        if isinstance(m, FP8_LAYER_TYPES):
            m.weight.data.copy_(ops.dequant_mxfp4(q[n].weight, q[n].w_scale))
    prompts = [[3, 17, 99, 250, 7], [5, 6, 7, 8, 9, 10, 11]]
    p = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    o4 = [s.output for s in e4.generate(prompts, p)]
    o16 = [s.output for s in e16.generate(prompts, p)]
    assert all(len(o) == 8 for o in o4) and o4 == o16
