"""``kv_prefill``: the route of the prefill attention over an fp8 KV cache ("native": the paged kernel reads the
codes, no bf16 scratch; "widen": the scratch route, the default) -- argument and environment resolution, the engine's
scratch, the serving config key, and a CPU engine on either route."""
import pytest
import torch

import shai_amd.ops as ops
from shai_amd.engines.llm import LLMEngine, SamplingParams
from shai_amd.models.llama import LlamaConfig

F8 = torch.float8_e4m3fn
KW = dict(device="cpu", max_num_seqs=4, max_model_len=256, seed=1)


def test_resolve_kv_prefill(monkeypatch):
    monkeypatch.delenv("SHAI_KV8_PREFILL", raising=False)
    assert ops.resolve_kv_prefill(None) == "widen"           # the default stays the scratch route
    assert ops.resolve_kv_prefill("native") == "native" and ops.resolve_kv_prefill(" Widen ") == "widen"
    monkeypatch.setenv("SHAI_KV8_PREFILL", "native")
    assert ops.resolve_kv_prefill(None) == "native"
    assert ops.resolve_kv_prefill("widen") == "widen"        # the argument wins over the environment
    monkeypatch.setenv("SHAI_KV8_PREFILL", "")
    assert ops.resolve_kv_prefill(None) == "widen"
    for bad in ("scratch", "fp8", "0"):
        with pytest.raises(ValueError, match="kv_prefill"):
            ops.resolve_kv_prefill(bad)
    monkeypatch.setenv("SHAI_KV8_PREFILL", "direct")
    with pytest.raises(ValueError, match="kv_prefill"):
        ops.resolve_kv_prefill(None)


def test_ops_accept_kv_prefill_on_the_cpu(monkeypatch):
    """On the CPU both routes run the reference; an unknown route is still an error with an fp8 cache, and the
    argument is ignored with a bf16 cache."""
    monkeypatch.delenv("SHAI_KV8_PREFILL", raising=False)
    torch.manual_seed(0)
    D, Hq, Hkv = 64, 4, 2
    kc = ops.quantize_kv_fp8(torch.randn(4, Hkv, 64, D).to(torch.bfloat16), 0.5)
    vc = ops.quantize_kv_fp8(torch.randn(4, Hkv, 64, D).to(torch.bfloat16), 2.0)
    bt = torch.tensor([[2, 0], [3, 0]], dtype=torch.int32)
    kl, ql = torch.tensor([70, 9], dtype=torch.int32), torch.tensor([6, 9], dtype=torch.int32)
    q = torch.randn(2, 9, Hq, D).to(torch.bfloat16)
    outs = [ops.paged_attention(q, kc, vc, bt, kl, ql, k_scale=0.5, v_scale=2.0, kv_prefill=r)
            for r in (None, "widen", "native")]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    qp = torch.cat([q[0, :6], q[1, :9]])
    qs = torch.tensor([0, 6], dtype=torch.int32)
    vo = [ops.paged_attention_varlen(qp, kc, vc, bt, kl, ql, qs, 9, k_scale=0.5, v_scale=2.0, kv_prefill=r)
          for r in ("widen", "native")]
    assert torch.equal(vo[0], vo[1]) and torch.equal(vo[0][:6], outs[0][0, :6]) and torch.equal(vo[0][6:], outs[0][1])
    with pytest.raises(ValueError, match="kv_prefill"):
        ops.paged_attention(q, kc, vc, bt, kl, ql, kv_prefill="scratch")
    with pytest.raises(ValueError, match="kv_prefill"):
        ops.paged_attention_varlen(qp, kc, vc, bt, kl, ql, qs, 9, kv_prefill="scratch")
    kb, vb = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    assert torch.equal(ops.paged_attention(q, kb, vb, bt, kl, ql, kv_prefill="scratch"),
                       ops.paged_attention(q, kb, vb, bt, kl, ql))


def test_engine_argument_and_environment(monkeypatch):
    monkeypatch.delenv("SHAI_KV8_PREFILL", raising=False)
    c = LlamaConfig.tiny()
    e = LLMEngine(c, kv_cache_dtype="fp8", **KW)
    assert e.kv_prefill == "widen" and e.kv_scratch is not None and e.kv_scratch_blocks > 0 and e.kv_scratch_bytes > 0
    n = LLMEngine(c, kv_cache_dtype="fp8", kv_prefill="native", **KW)
    assert n.kv_prefill == "native" and n.kv_buf.dtype == F8
    assert n.kv_scratch is None and n.kv_scratch_blocks == 0 and n.kv_scratch_bytes == 0
    monkeypatch.setenv("SHAI_KV8_PREFILL", "native")
    assert LLMEngine(c, kv_cache_dtype="fp8", **KW).kv_scratch is None
    w = LLMEngine(c, kv_cache_dtype="fp8", kv_prefill="widen", **KW)      # the argument wins
    assert w.kv_prefill == "widen" and w.kv_scratch is not None
    b = LLMEngine(c, kv_prefill="native", **KW)                           # bf16 cache: nothing to choose
    assert b.kv_buf.dtype == torch.bfloat16 and b.kv_scratch is None
    monkeypatch.delenv("SHAI_KV8_PREFILL")
    with pytest.raises(ValueError, match="kv_prefill"):
        LLMEngine(c, kv_cache_dtype="fp8", kv_prefill="scratch", **KW)
    with pytest.raises(ValueError, match="kv_scratch_blocks"):
        LLMEngine(c, kv_cache_dtype="fp8", kv_prefill="native", kv_scratch_blocks=8, **KW)
    assert LLMEngine(c, kv_cache_dtype="fp8", kv_prefill="widen", kv_scratch_blocks=8, **KW).kv_scratch_blocks == 8


def test_mllama_stays_rejected_with_an_fp8_cache():
    from shai_amd.models.mllama import MllamaConfig
    with pytest.raises(NotImplementedError, match="mllama"):
        LLMEngine(MllamaConfig.tiny(), kv_cache_dtype="fp8", kv_prefill="native", **KW)


def test_vllm_config_kv_prefill_reaches_the_engine(tmp_path, monkeypatch):
    from shai_amd.serving import llm_api
    from shai_amd.serving.common import ServerEnv
    monkeypatch.delenv("SHAI_KV8_PREFILL", raising=False)
    env = ServerEnv(app="mistral", pod_name="pod0", nodepool="mi355x", model_id="m", device="cpu", config="tiny",
                    num_inference_steps=2, max_new_tokens=4, max_seq_len=16, height=64, width=64)
    cfgf = tmp_path / "vllm_config.yaml"
    monkeypatch.setenv("VLLM_CONFIG", str(cfgf))
    cfgf.write_text("max_num_seqs: 2\nmax_model_len: 128\nkv_cache_dtype: fp8\nkv_prefill: native\n")
    eng = llm_api.build_engine(env)
    assert eng.kv_cache_dtype == "fp8" and eng.kv_prefill == "native" and eng.kv_scratch is None
    cfgf.write_text("max_num_seqs: 2\nmax_model_len: 128\nkv_cache_dtype: fp8\n")
    eng = llm_api.build_engine(env)
    assert eng.kv_prefill == "widen" and eng.kv_scratch is not None
    cfgf.write_text("max_num_seqs: 2\nmax_model_len: 128\nkv_cache_dtype: fp8\nkv_prefill: bf16\n")
    with pytest.raises(ValueError, match="kv_prefill"):
        llm_api.build_engine(env)


def _generate(eng):
    """Two running sequences, a 200-token prompt in 64-token chunks beside them, then a prefix-cache hit."""
    p = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
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
    assert eng.stats["prefix_hit_tokens"] >= hits + 128
    return [s.output for s in seqs]


def test_cpu_native_engine_generates_the_widen_engines_tokens(monkeypatch):
    monkeypatch.delenv("SHAI_KV8_PREFILL", raising=False)
    c = LlamaConfig.tiny()
    kw = dict(KW, kv_cache_dtype="fp8", prefill_chunk=64, enable_prefix_caching=True)
    ew, en = LLMEngine(c, kv_prefill="widen", **kw), LLMEngine(c, kv_prefill="native", **kw)
    assert en.kv_scratch is None and ew.kv_scratch is not None
    att, seen = en._attach_kv_rounds, []
    en._attach_kv_rounds = lambda batch, *a: (att(batch, *a), seen.append(
        (batch.kv_prefill, batch.kv_rounds, batch.kv_scratch, batch.q_groups)))[0]
    want, got = _generate(ew), _generate(en)
    assert got == want and all(len(o) == 6 for o in got)
    assert len(seen) >= 5 and all(s[:3] == ("native", None, None) for s in seen)   # nothing is planned
    # a 64-token chunk of the long prompt with the two decode rows behind it: two launch groups
    assert ("native", None, None, [(0, 1, 64), (1, 2, 1)]) in seen, seen
    assert en.bm.num_free == en.num_kv_blocks
