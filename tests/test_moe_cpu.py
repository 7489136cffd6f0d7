"""Mixtral sparse-MoE on the CPU (fp32 reference ops): transformers parity through both checkpoint key layouts, the
routing contract of ops.reference, and the engine's scope limits."""
import pytest
import torch

from shai_amd.engines.llm import LLMEngine, SamplingParams
from shai_amd.models.llama import LlamaConfig
from shai_amd.ops import reference as ref
from shai_amd.weights import load_into


def _hf_tiny_moe():
    transformers = pytest.importorskip("transformers")
    c = LlamaConfig.tiny_moe()
    hc = transformers.MixtralConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size,
                                    intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                                    num_attention_heads=c.num_attention_heads,
                                    num_key_value_heads=c.num_key_value_heads, head_dim=c.head_dim,
                                    rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta,
                                    max_position_embeddings=c.max_position_embeddings, tie_word_embeddings=False,
                                    num_local_experts=c.num_local_experts, num_experts_per_tok=c.num_experts_per_tok,
                                    sliding_window=None)
    torch.manual_seed(0)
    m = transformers.MixtralForCausalLM(hc).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())  # bf16-representable weights
    return c, m


def _hub_layout(sd, cfg):
    """The installed transformers' fused expert tensors rewritten as the hub checkpoints name them."""
    out, I = {}, cfg.intermediate_size
    for k, v in sd.items():
        if k.endswith("mlp.gate.weight"):
            out[k.replace("mlp.gate.weight", "block_sparse_moe.gate.weight")] = v
        elif k.endswith("mlp.experts.gate_up_proj"):
            for e in range(cfg.num_local_experts):
                p = k.replace("mlp.experts.gate_up_proj", f"block_sparse_moe.experts.{e}.")
                out[p + "w1.weight"], out[p + "w3.weight"] = v[e, :I].clone(), v[e, I:].clone()
        elif k.endswith("mlp.experts.down_proj"):
            for e in range(cfg.num_local_experts):
                out[k.replace("mlp.experts.down_proj", f"block_sparse_moe.experts.{e}.w2.weight")] = v[e].clone()
        else:
            out[k] = v
    return out


@pytest.mark.parametrize("layout", ["fused", "hub"])
def test_mixtral_matches_transformers(layout):
    c, hf = _hf_tiny_moe()
    sd = {k: v.clone() for k, v in hf.state_dict().items()}
    if layout == "hub":
        if not any(k.endswith("mlp.experts.gate_up_proj") for k in sd):
            pytest.skip("this transformers already uses the hub layout: covered by the other case")
        sd = _hub_layout(sd, c)
    eng = LLMEngine(c, device="cpu", max_num_seqs=2, max_model_len=256, enable_prefix_caching=False)
    load_into(eng.model, sd, eng.model.convert_hf_state_dict, strict=True)
    prompt = [3, 17, 99, 250, 7, 7, 400, 12]
    with torch.no_grad():
        want = hf(torch.tensor([prompt])).logits[0, -1].float()
        g = hf.generate(torch.tensor([prompt]), max_new_tokens=6, do_sample=False)[0, len(prompt):].tolist()
    seq = eng.add_request(prompt, SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    eng.step()
    assert seq.finished and seq.output[0] == int(want.argmax())
    out = eng.generate([prompt], SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))[0].output
    assert out[:3] == g[:3]   # (the compared length of test_llama_matches_transformers)


@pytest.mark.parametrize("k", [1, 2])
def test_reference_routing_ties_and_weights(k):
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    x[:, 0] = 1.0
    wg = torch.zeros(8, 64)
    wg[:, 0] = torch.tensor([1.0, 3.0, 3.0, 0.0, 3.0, 2.0, 0.0, 0.0])   # experts 1, 2 and 4 tie at the top
    for eps in (None, 1e-5):
        ids, w, rstd = ref.moe_route(x, wg, k, eps)
        assert ids.dtype == torch.int32 and ids.tolist() == [[1, 2][:k]] * 4
        assert torch.allclose(w.sum(1), torch.ones(4)) and bool((w > 0).all())
        if k == 2:
            assert torch.equal(w[:, 0], w[:, 1])
        assert torch.allclose(rstd, torch.full((4,), 8.0 if eps else 1.0), rtol=1e-3)


@pytest.mark.parametrize("kw", [dict(quantization="fp8"), dict(quantization="mxfp4"), dict(quantization="nf4"),
                                dict(quantization="bitsandbytes"), dict(tp=2)])
def test_engine_rejects_moe_outside_scope(kw, monkeypatch):
    if "tp" in kw:
        import shai_amd.engines.llm as llm
        st = type("St", (), {"size": kw["tp"], "rank": 0})()
        monkeypatch.setattr(llm, "tp", lambda: st)
        kw = {}
    with pytest.raises(NotImplementedError, match="mixture-of-experts"):
        LLMEngine(LlamaConfig.tiny_moe(), device="cpu", max_num_seqs=2, max_model_len=128, **kw)
