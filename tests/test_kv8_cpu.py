"""FP8 (OCP e4m3fn) KV cache on the CPU: the quantisation rule (the oracle of the GPU writers), the fp32 reference
over an fp8 cache, the engine argument, the scratch-grouping planner and the serving config key."""
import math

import numpy as np
import pytest
import torch

import shai_amd.ops as ops
from shai_amd.ops import reference as ref


def test_quantisation_rule_vector_and_round_trip():
    x = torch.tensor([1000, -1000, 448, 464, 465, 9e-4, 2 ** -9, 0.3, 17.3, -0.0])
    want = [126, 254, 126, 126, 126, 0, 1, 42, 89, 128]
    for q in (ref.quantize_kv_fp8, ops.quantize_kv_fp8):
        c = q(x, 1.0)
        assert c.dtype == torch.float8_e4m3fn
        assert c.view(torch.uint8).tolist() == want
    # bf16 input (what the cache writers see) gives the same codes where bf16 holds the value
    assert ops.quantize_kv_fp8(x[:5].bfloat16(), 1.0).view(torch.uint8).tolist() == want[:5]
    # every finite code survives scale * code -> quantise at power-of-two scales
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7f) != 0x7f].view(torch.float8_e4m3fn)   # 0x7f / 0xff are NaN
    for scale in (0.5, 2.0):
        vals = ops.dequant_kv_fp8(codes, scale, torch.float32)
        assert torch.equal(vals, codes.float() * scale)
        back = ops.quantize_kv_fp8(vals, scale)
        assert torch.equal(back.view(torch.uint8), codes.view(torch.uint8))
    assert ops.dequant_kv_fp8(codes, 2.0).dtype == torch.bfloat16


def test_reference_decode_over_fp8_cache_equals_dequantised_cache():
    torch.manual_seed(0)
    Hq, Hkv, D, nb = 8, 2, 64, 6
    ctx = [1, 64, 130]
    ks, vs = 0.5, 2.0
    T = sum(ctx)
    k = (torch.randn(T, Hkv, D) * 3).bfloat16()
    v = (torch.randn(T, Hkv, D) * 3).bfloat16()
    k[0, 0, 0], v[1, 1, 1] = 900.0, -2000.0    # clamped
    bt = torch.zeros(len(ctx), 3, dtype=torch.int32)
    perm = torch.randperm(nb).int()
    slots, i = [], 0
    for b, c in enumerate(ctx):
        n = (c + 63) // 64
        bt[b, :n] = perm[i:i + n]
        i += n
        slots += [int(bt[b, t // 64]) * 64 + t % 64 for t in range(c)]
    slots = torch.tensor(slots, dtype=torch.int32)
    kc = torch.zeros(nb, Hkv, 64, D, dtype=torch.float8_e4m3fn)
    vc = torch.zeros_like(kc)
    ops.kv_write(k, v, kc, vc, slots, ks, vs)          # CPU: ref.kv_write
    assert kc.dtype == torch.float8_e4m3fn
    t0 = int(slots[0])
    assert torch.equal(kc[t0 // 64, :, t0 % 64].view(torch.uint8), ref.quantize_kv_fp8(k[0], ks).view(torch.uint8))
    assert kc[t0 // 64, 0, t0 % 64, 0].float().item() == 448.0
    q = torch.randn(len(ctx), Hq, D).bfloat16()
    lens = torch.tensor(ctx, dtype=torch.int32)
    sc = 1 / math.sqrt(D)
    got = ref.decode_attention(q, kc, vc, bt, lens, sc, ks, vs)
    want = ref.decode_attention(q, ref.dequant_kv_fp8(kc, ks), ref.dequant_kv_fp8(vc, vs), bt, lens, sc)
    assert torch.equal(got, want)
    assert torch.equal(ops.decode_attention(q, kc, vc, bt, lens, sc, k_scale=ks, v_scale=vs), want)
    # the prefill references dequantise the same way
    ql = torch.tensor([1, 5, 7], dtype=torch.int32)
    qs = torch.tensor([0, 1, 6], dtype=torch.int32)
    qp = torch.randn(13, Hq, D).bfloat16()
    got = ops.paged_attention_varlen(qp, kc, vc, bt, lens, ql, qs, 7, sc, k_scale=ks, v_scale=vs)
    want = ref.paged_attention_varlen(qp, ref.dequant_kv_fp8(kc, ks), ref.dequant_kv_fp8(vc, vs), bt, lens, ql, qs, sc)
    assert torch.equal(got, want)
    # mixed cache dtypes are an error, not a silent cast
    with pytest.raises(ValueError, match="dtypes differ"):
        ref.decode_attention(q, kc, vc.float().bfloat16(), bt, lens, sc)
    # the block widener's reference
    ko = torch.zeros(4, Hkv, 64, D, dtype=torch.bfloat16)
    vo = torch.zeros_like(ko)
    phys = torch.tensor([3, 1], dtype=torch.int32)
    ops.kv_dequant_blocks(kc, vc, phys, ko, vo, ks, vs)
    assert torch.equal(ko[1], ref.dequant_kv_fp8(kc[1], ks, torch.bfloat16)) and torch.equal(
        vo[0], ref.dequant_kv_fp8(vc[3], vs, torch.bfloat16))


def test_tiny_cpu_engine_with_fp8_kv():
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig, kv_bytes_per_block
    from shai_amd.models.mllama import MllamaConfig
    c = LlamaConfig.tiny()
    kw = dict(device="cpu", max_num_seqs=2, max_model_len=256, seed=1)
    eng = LLMEngine(c, kv_cache_dtype="fp8", k_scale=0.5, v_scale=2.0, **kw)
    assert eng.kv_cache_dtype == "fp8" and eng.kv_buf.dtype == torch.float8_e4m3fn
    assert eng.kv[0][0].dtype == torch.float8_e4m3fn
    assert eng.k_scales == [0.5] * c.num_hidden_layers and eng.model.layers[-1].self_attn.v_scale == 2.0
    assert eng.kv_scratch_blocks >= eng.max_blocks + 1
    hk = eng.model.kv_heads_local
    assert 2 * kv_bytes_per_block(c, hk, torch.float8_e4m3fn) == kv_bytes_per_block(c, hk, torch.bfloat16)
    assert kv_bytes_per_block(c, hk) == kv_bytes_per_block(c, hk, torch.bfloat16)
    prompts = [[3, 17, 99, 250, 7], list(range(5, 75))]
    out = eng.generate(prompts, SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))
    assert all(len(s.output) == 6 and all(0 <= t < c.vocab_size for t in s.output) for s in out)
    assert eng.kv_buf.view(torch.uint8).any()            # codes were written
    assert eng.bm.num_free == eng.num_kv_blocks
    # default and aliases: bf16 cache, exactly as before
    for name in (None, "auto", "bf16"):
        e = LLMEngine(c, kv_cache_dtype=name, **kw)
        assert e.kv_buf.dtype == torch.bfloat16 and e.kv_scratch is None and e.kv_cache_dtype == "auto"
    assert LLMEngine(c, kv_cache_dtype="fp8_e4m3", **kw).kv_buf.dtype == torch.float8_e4m3fn
    with pytest.raises(ValueError, match="fp8_e4m3"):
        LLMEngine(c, kv_cache_dtype="fp8_e5m2", **kw)
    with pytest.raises(NotImplementedError, match="not supported yet"):
        LLMEngine(MllamaConfig.tiny(), kv_cache_dtype="fp8", **kw)


def test_engine_reads_kv_cache_dtype_from_environment(monkeypatch):
    from shai_amd.engines.llm import LLMEngine
    from shai_amd.models.llama import LlamaConfig
    kw = dict(device="cpu", max_num_seqs=2, max_model_len=128)
    monkeypatch.setenv("SHAI_KV_CACHE_DTYPE", "fp8")
    assert LLMEngine(LlamaConfig.tiny(), **kw).kv_buf.dtype == torch.float8_e4m3fn
    assert LLMEngine(LlamaConfig.tiny(), kv_cache_dtype="auto", **kw).kv_buf.dtype == torch.bfloat16   # argument wins
    monkeypatch.delenv("SHAI_KV_CACHE_DTYPE")
    assert LLMEngine(LlamaConfig.tiny(), **kw).kv_buf.dtype == torch.bfloat16


def test_scratch_planner_covers_each_sequence_once_within_capacity():
    rng = np.random.default_rng(0)
    for cap in (5, 8, 17):
        need = rng.integers(0, cap + 1, 40).tolist()
        groups = ops.plan_kv_scratch(need, cap)
        assert sorted(i for g in groups for i in g) == list(range(len(need)))
        assert all(sum(need[i] for i in g) <= cap for g in groups)
        assert len(groups) > 1
    assert ops.plan_kv_scratch([3, 2], 5) == [[0, 1]]
    with pytest.raises(ValueError, match="scratch"):
        ops.plan_kv_scratch([2, 6], 5)
    # the rounds: remapped tables address the round's own scratch blocks, in the order the blocks are widened
    bt = np.arange(40, dtype=np.int32).reshape(4, 10) + 100
    kv = np.array([65, 10, 200, 64], np.int32)
    ql = np.array([5, 10, 3, 1], np.int32)
    qs = np.array([0, 5, 15, 18], np.int32)
    rounds = ops.build_kv_rounds(bt, kv, ql, qs, 5, "cpu")
    assert [r.sel.tolist() for r in rounds] == [[0, 1], [2, 3]]
    seen = []
    for r in rounds:
        assert r.phys.numel() == r.n_blocks <= 5
        for row, b in enumerate(r.sel.tolist()):
            n = (int(kv[b]) + 63) // 64
            assert r.phys[r.block_table[row, :n].long()].tolist() == bt[b, :n].tolist()
            seen.append(b)
        assert r.kv_lens.tolist() == kv[r.sel.numpy()].tolist() and r.q_start.tolist() == qs[r.sel.numpy()].tolist()
        assert r.max_q == int(ql[r.sel.numpy()].max())
    assert seen == [0, 1, 2, 3]
    one = ops.build_kv_rounds(bt, kv, ql, qs, 64, "cpu")
    assert len(one) == 1 and one[0].sel is None


def test_vllm_config_kv_cache_dtype_reaches_the_engine(tmp_path, monkeypatch):
    from shai_amd.serving import llm_api
    from shai_amd.serving.common import ServerEnv

    def env(**kw):   # as tests/test_api_cpu.py
        base = dict(app="t", pod_name="pod0", nodepool="mi355x", model_id="m", device="cpu", config="tiny",
                    num_inference_steps=2, max_new_tokens=4, max_seq_len=16, height=64, width=64)
        base.update(kw)
        return ServerEnv(**base)
    cfgf = tmp_path / "vllm_config.yaml"
    cfgf.write_text("max_num_seqs: 2\nmax_model_len: 128\nkv_cache_dtype: fp8\n")
    monkeypatch.setenv("VLLM_CONFIG", str(cfgf))
    eng = llm_api.build_engine(env(app="mistral"))
    assert eng.kv_cache_dtype == "fp8" and eng.kv_buf.dtype == torch.float8_e4m3fn and eng.max_num_seqs == 2
    cfgf.write_text("max_num_seqs: 2\nmax_model_len: 128\n")
    assert llm_api.build_engine(env(app="mistral")).kv_buf.dtype == torch.bfloat16
    cfgf.write_text("max_num_seqs: 2\nmax_model_len: 128\nkv_cache_dtype: int4\n")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        llm_api.build_engine(env(app="mistral"))
