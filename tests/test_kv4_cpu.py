"""MXFP4 KV cache on the CPU: the oracle's rule on hand-written rows, the option's three sources, a tiny engine and
the rejections."""
import pytest
import torch

import shai_amd.ops as ops
from shai_amd.ops import reference as ref


def test_rule_on_hand_written_row_and_round_trip():
    """Groups: all zero (scale 124, codes 0); amax exactly 4 = 2^2 (e = 0, scale 127: 4 -> code 6, ties 2.5 -> 2,
    3.5 -> 4, -0.25 -> 0 with no sign bit, -0.75 -> -1.0); amax 96 (e = 4, scale 131: 96 / 16 = 6 -> code 7,
    -100 would saturate but 96 is the amax; 8 / 16 = 0.5 -> code 1)."""
    x = torch.zeros(1, 96)
    x[0, 32:40] = torch.tensor([4.0, 2.5, 3.5, -0.25, -0.75, 1.0, 0.0, -4.0])
    x[0, 64:68] = torch.tensor([96.0, 8.0, -96.0, 52.0])   # 52 / 16 = 3.25 -> 3.0 (code 5)
    codes, sb = ops.quantize_kv_mxfp4(x.bfloat16())
    assert sb.tolist() == [[124, 127, 131]]
    assert codes[0, :16].eq(0).all() and codes[0, 20:32].eq(0).all() and codes[0, 34:].eq(0).all()
    assert codes[0, 16:20].tolist() == [6 | (4 << 4), 6 | (0 << 4), 10 | (2 << 4), 0 | (14 << 4)]
    assert codes[0, 32:34].tolist() == [7 | (1 << 4), 15 | (5 << 4)]
    d = ops.dequant_kv_mxfp4(codes, sb, torch.float32)
    assert d[0, 32:40].tolist() == [4.0, 2.0, 4.0, 0.0, -1.0, 1.0, 0.0, -4.0]
    assert d[0, 64:68].tolist() == [96.0, 8.0, -96.0, 48.0]
    y = torch.zeros(1, 32)
    y[0, 0] = 7.5   # above 6 * scale (e = 0): saturates
    assert ops.dequant_kv_mxfp4(*ops.quantize_kv_mxfp4(y), torch.float32)[0, 0] == 6.0
    torch.manual_seed(0)
    r = (torch.randn(5, 3, 128) * 4).bfloat16()
    once = ops.dequant_kv_mxfp4(*ops.quantize_kv_mxfp4(r))
    assert once.dtype == torch.bfloat16 and torch.isfinite(once).all()
    assert torch.equal(ops.dequant_kv_mxfp4(*ops.quantize_kv_mxfp4(once)), once)
    assert torch.equal(ref.dequant_mxfp4(*ref.quantize_mxfp4(r.reshape(15, 128))), once.reshape(15, 128))   # one rule


@pytest.mark.parametrize("D", [64, 128])
def test_reference_paths_over_an_mxfp4_cache(D):
    """kv_write fills code and scale planes of the region layout; decode and the widener read them back."""
    torch.manual_seed(1)
    H, nb = 2, 3
    kc = torch.zeros(nb, H, 64, D // 2 + D // 32, dtype=torch.uint8)
    vc = torch.zeros_like(kc)
    k, v = torch.randn(70, H, D).bfloat16(), torch.randn(70, H, D).bfloat16()
    slots = torch.arange(70, dtype=torch.int32) + 64   # blocks 1 and 2
    ops.kv_write(k, v, kc, vc, slots)
    codes, sb = ops.quantize_kv_mxfp4(k)
    flat = kc.reshape(nb, H, -1)
    assert torch.equal(flat[1, :, :32 * D].reshape(H, 64, D // 2), codes[:64].transpose(0, 1))
    assert torch.equal(flat[2, :, 32 * D:].reshape(H, 64, D // 32)[:, :6], sb[64:].transpose(0, 1)) and not flat[0].any()
    kd, vd = ops.dequant_kv_mxfp4(codes, sb, torch.float32), ops.dequant_kv_mxfp4(*ops.quantize_kv_mxfp4(v), torch.float32)
    bt = torch.tensor([[1, 2]], dtype=torch.int32)
    lens = torch.tensor([70], dtype=torch.int32)
    q = torch.randn(1, 4, D).bfloat16()
    want = ref.attention(q[:, None], kd[None], vd[None], scale=D ** -0.5)[0, 0]
    assert torch.equal(ops.decode_attention(q, kc, vc, bt, lens), want[None])
    ko, vo = torch.zeros(2, H, 64, D).bfloat16(), torch.zeros(2, H, 64, D).bfloat16()
    ops.kv_dequant_blocks(kc, vc, torch.tensor([2, 1], dtype=torch.int32), ko, vo)
    assert torch.equal(ko[1].transpose(0, 1), kd[:64].bfloat16()) and torch.equal(vo[0, :, :6].transpose(0, 1),
                                                                                 vd[64:].bfloat16())
    for exc, call in ((ValueError, lambda: ops.decode_attention(q, kc, vc.view(torch.float8_e4m3fn), bt, lens)),
                      (ValueError, lambda: ops.kv_write(k, v, kc, vc, slots, k_scale=0.5)),
                      (NotImplementedError, lambda: ops.paged_attention(q[:, None], kc, vc, bt, lens, None,
                                                                        kv_prefill="native"))):
        with pytest.raises(exc):
            call()


def test_option_sources_engine_and_rejections(tmp_path, monkeypatch):
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig, kv_bytes_per_block
    from shai_amd.models.mllama import MllamaConfig
    from shai_amd.serving import llm_api
    from shai_amd.serving.common import ServerEnv
    c = LlamaConfig.tiny()
    kw = dict(device="cpu", max_num_seqs=2, max_model_len=256, seed=1)
    eng = LLMEngine(c, kv_cache_dtype="mxfp4", **kw)
    D, hk = c.head_dim, eng.model.kv_heads_local
    assert eng.kv_cache_dtype == "mxfp4" and eng.kv_buf.dtype == torch.uint8 and eng.kv_prefill == "widen"
    assert eng.kv_buf.shape[-2:] == (64, D // 2 + D // 32) and eng.kv_scratch_blocks >= eng.max_blocks + 1
    assert kv_bytes_per_block(c, hk, torch.uint8) * 64 == kv_bytes_per_block(c, hk, torch.bfloat16) * 17
    assert LLMEngine(c, kv_cache_dtype="fp4", **kw).kv_cache_dtype == "mxfp4"
    prompts = [[3, 17, 99, 250, 7], list(range(5, 75))]
    out = eng.generate(prompts, SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))
    assert all(len(s.output) == 6 and all(0 <= t < c.vocab_size for t in s.output) for s in out) and eng.kv_buf.any()
    for bad, exc in ((dict(k_scale=0.5), ValueError), (dict(v_scale=2.0), ValueError),
                     (dict(kv_prefill="native"), NotImplementedError),
                     (dict(speculative={"method": "ngram", "num_speculative_tokens": 2}), NotImplementedError)):
        with pytest.raises(exc):
            LLMEngine(c, kv_cache_dtype="mxfp4", **bad, **kw)
    with pytest.raises(NotImplementedError, match="mllama"):
        LLMEngine(MllamaConfig.tiny(), kv_cache_dtype="mxfp4", **kw)
    for name in ("int4", "fp8_e5m2"):
        with pytest.raises(ValueError, match="kv_cache_dtype.*fp8_e4m3"):
            LLMEngine(c, kv_cache_dtype=name, **kw)
    monkeypatch.setenv("SHAI_KV_CACHE_DTYPE", "mxfp4")
    assert LLMEngine(c, **kw).kv_buf.dtype == torch.uint8
    assert LLMEngine(c, kv_cache_dtype="auto", **kw).kv_buf.dtype == torch.bfloat16   # the argument wins
    monkeypatch.delenv("SHAI_KV_CACHE_DTYPE")
    cfgf = tmp_path / "vllm_config.yaml"
    cfgf.write_text("max_num_seqs: 2\nmax_model_len: 128\nkv_cache_dtype: mxfp4\n")
    monkeypatch.setenv("VLLM_CONFIG", str(cfgf))
    env = ServerEnv(app="mistral", pod_name="pod0", nodepool="mi355x", model_id="m", device="cpu", config="tiny",
                    num_inference_steps=2, max_new_tokens=4, max_seq_len=16, height=64, width=64)
    assert llm_api.build_engine(env).kv_cache_dtype == "mxfp4"
