"""NF4 (bitsandbytes 4-bit) weight-only format on the CPU: quantiser / table decode / layout helpers of
ops/reference.py, and the ``quantization: nf4`` / ``bitsandbytes`` switch of the LLM engine."""
import pytest
import torch

from shai_amd import ops
from nf4_cases import nf4_case


@pytest.mark.parametrize("n,k", [(3, 64), (16, 320), (5, 1024)])
def test_quantise_dequantise_round_trip(n, k):
    codes, absmax, w = nf4_case(n, k, seed=n + k)
    wq, am = ops.quantize_nf4(w)
    assert wq.dtype == torch.uint8 and tuple(wq.shape) == (n, k // 2) and ops.is_nf4(wq)
    assert am.dtype == torch.float32 and tuple(am.shape) == ((k + 127) // 128, n, 2)
    c2, a2 = ops.nf4_unpack(wq, am)
    assert torch.equal(c2, codes) and torch.equal(a2, absmax)
    assert torch.equal(ops.dequant_nf4(wq, am), w)
    # the layout helpers invert each other
    wq2, am2 = ops.nf4_pack(codes, absmax)
    assert torch.equal(wq2, wq) and torch.equal(am2, am)


def test_zero_block_and_ties():
    w = torch.zeros(2, 128, dtype=torch.bfloat16)
    w[1, 64:] = 0.5
    wq, am = ops.quantize_nf4(w)
    codes, absmax = ops.nf4_unpack(wq, am)
    assert torch.equal(absmax, torch.tensor([[0.0, 0.0], [0.0, 0.5]]))
    assert bool((codes[0] == 7).all()) and bool((codes[1, :64] == 7).all()) and bool((codes[1, 64:] == 15).all())
    assert torch.equal(ops.dequant_nf4(wq, am), w)
    # half of table entry 8 (exact in fp32) is the midpoint of entries 7 (= 0) and 8: a tie takes the lower index
    t = torch.zeros(1, 64)
    t[0, 0], t[0, 1] = 1.0, torch.tensor(ops.NF4_TABLE[8], dtype=torch.float32) / 2
    assert ops.nf4_unpack(*ops.quantize_nf4(t))[0][0, :3].tolist() == [15, 7, 7]


def test_k_must_hold_whole_blocks():
    from shai_amd.parallel.layers import RowParallelLinear
    with pytest.raises(ValueError, match="K % 64 == 0"):
        ops.quantize_nf4(torch.zeros(4, 96))
    lin = RowParallelLinear(96, 64, bias=False)
    lin.weight.data.normal_()
    with pytest.raises(ValueError, match="multiple of the NF4 block size 64"):
        lin.quantize_nf4_()


@pytest.mark.parametrize("M", [80, 5])
def test_cpu_linear_is_the_dequantised_linear(M):
    from shai_amd.ops import reference as ref
    wq, am = ops.quantize_nf4(nf4_case(64, 256, seed=2)[2])
    x = torch.randn(M, 256, generator=torch.Generator().manual_seed(M)).bfloat16()
    got = ops.linear(x, wq, act="silu", glu=True, w_scale=am)
    assert torch.equal(got, ref.linear(x, ops.dequant_nf4(wq, am), None, "silu", glu=True))
    out = torch.empty(M, 64, dtype=torch.bfloat16)
    ops.gemm_into(x, wq, out, w_scale=am)
    assert torch.equal(out, ref.linear(x, ops.dequant_nf4(wq, am)))


def test_cpu_engine_matches_dequantised_weights():
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    from shai_amd.parallel.layers import FP8_LAYER_TYPES
    c = LlamaConfig.tiny()
    kw = dict(device="cpu", max_num_seqs=2, max_model_len=256, seed=1, enable_prefix_caching=False)
    e4 = LLMEngine(c, quantization="nf4", **kw)
    e16 = LLMEngine(c, **kw)
    assert e4.quantization == "nf4"
    q = {n: m for n, m in e4.model.named_modules() if isinstance(m, FP8_LAYER_TYPES)}
    assert q and all(m.weight.dtype == torch.uint8 and m.w_scale.dtype == torch.float32 for m in q.values())
    assert e4.model.embed_tokens.weight.dtype == torch.bfloat16 and e4.model.lm_head.weight.dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="NF4"):
        e4.model.fold_norms()
    for n, m in e16.model.named_modules():
        if isinstance(m, FP8_LAYER_TYPES):
            m.weight.data.copy_(ops.dequant_nf4(q[n].weight, q[n].w_scale))
    logits = {}
    for name, eng in (("nf4", e4), ("bf16", e16)):
        fwd, rec = eng.model.forward, logits.setdefault(name, [])
        eng.model.forward = lambda *a, _f=fwd, _r=rec, **k: (lambda y: (_r.append(y.float().clone()), y)[1])(_f(*a, **k))
        eng.generate([[3, 17, 99, 250, 7], [5, 6, 7, 8, 9, 10, 11]],
                     SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))
    assert len(logits["nf4"]) == len(logits["bf16"]) >= 6
    assert all(torch.equal(a, b) for a, b in zip(logits["nf4"], logits["bf16"]))


def test_vllm_config_bitsandbytes_reaches_the_engine():
    from shai_amd.serving import llm_api
    from shai_amd.serving.common import ServerEnv
    env = ServerEnv(app="mistral", pod_name="pod0", nodepool="mi355x", model_id="m", device="cpu", config="tiny",
                    num_inference_steps=2, max_new_tokens=4, max_seq_len=16, height=64, width=64)
    eng = llm_api.build_engine(env, {"max_num_seqs": 2, "max_model_len": 128, "quantization": "bitsandbytes"})
    assert eng.quantization == "nf4" and eng.model.layers[0].mlp.gate_up_proj.weight.dtype == torch.uint8
