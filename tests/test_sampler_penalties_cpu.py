"""Sampler penalties, min_p and logprobs without a GPU: the oracle against transformers, the exact cases against
the oracle and its mutants, and the engine-level properties on the CPU engine (which keeps the same state table as a
CPU tensor and samples through the oracle)."""
import base64

import pytest
import torch

import sampler_cases as sc
from shai_amd import ops
from shai_amd.engines.llm import LLMEngine, SamplingParams
from shai_amd.models.llama import LlamaConfig
from shai_amd.ops import reference as ref

TINY = LlamaConfig.tiny()
PROMPTS = [[3, 17, 99, 250, 7, 7, 400, 12], [5, 6, 7], [9, 9, 9, 9, 41], list(range(20, 90))]


def _engine(**kw):
    kw.setdefault("max_num_seqs", 4)
    kw.setdefault("max_model_len", 256)
    return LLMEngine(TINY, device="cpu", **kw)


def _mixed_params():
    return [SamplingParams(max_tokens=9, temperature=0.0, ignore_eos=True, repetition_penalty=1.3, logprobs=3),
            SamplingParams(max_tokens=12, temperature=0.8, seed=11, frequency_penalty=0.5, presence_penalty=0.25,
                           min_p=0.05, stop_token_ids=[272, 159, 238, 81], ignore_eos=True),
            SamplingParams(max_tokens=7, temperature=0.7, ignore_eos=True, logprobs=0, seed=5),
            SamplingParams(max_tokens=8, temperature=0.9, top_k=0, ignore_eos=True, min_p=0.1, seed=2,
                           repetition_penalty=0.8, logprobs=20)]


# ---------------------------------------------------------------------- the rule
def test_oracle_matches_transformers_processors():
    tr = pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(0)
    B, V = 5, 777
    scores = torch.randn(B, V, generator=g) * 4
    ids = torch.randint(0, V, (B, 40), generator=g)
    for r in (1.3, 0.7, 2.0):
        want = tr.RepetitionPenaltyLogitsProcessor(penalty=r)(ids, scores.clone())
        words = torch.stack([sc.recount(row.tolist(), 25, V) for row in ids])     # 25 "prompt" + 15 "output" tokens
        got = ref.penalize_logits(scores, words, torch.full((B,), r), torch.zeros(B), torch.zeros(B))
        assert torch.equal(got, want)
    for mp in (0.05, 0.3):
        want = tr.MinPLogitsWarper(min_p=mp)(ids, scores.clone())                 # -inf where dropped
        _, kept = ref.sample_candidates(scores, torch.ones(B), torch.zeros(B, dtype=torch.long), torch.ones(B),
                                        torch.full((B,), mp), torch.zeros(B), return_kept=True)
        assert torch.equal(kept, torch.isfinite(want))


@pytest.mark.parametrize("V", sc.VOCABS[:2])
def test_exact_cases_oracle_fp32_equals_fp64(V):
    case = sc.exact_batch(V)
    toks, st = sc.run_calls(case)
    assert torch.equal(toks, case.tokens)
    assert torch.equal(st, case.states[-1])
    # rows without a state row, and the canaries either side, were not touched
    for r in [0, case.B + 1] + [b + 1 for b in range(case.B) if case.rows[b] < 0]:
        assert torch.equal(st[r], case.states[0][r])
    # every row's state is its initial words plus a recount of what it sampled
    for b in range(case.B):
        if case.rows[b] >= 0:
            assert torch.equal(st[b + 1] - case.states[0][b + 1], sc.recount(case.tokens[:, b].tolist(), 0, V))


@pytest.mark.parametrize("mutant", ["output_only", "mul_positive", "presence_by_count", "minp_after_nucleus",
                                    "no_state_update"])
def test_mutants_fail_the_exact_cases(mutant):
    case = sc.exact_batch(1000)
    kw = {"output_only": dict(penalize=sc.mutant_output_only), "mul_positive": dict(penalize=sc.mutant_mul_positive),
          "presence_by_count": dict(penalize=sc.mutant_presence_by_count),
          "minp_after_nucleus": dict(candidates=sc.mutant_minp_after_nucleus),
          "no_state_update": dict(update=False)}[mutant]
    toks, _ = sc.run_calls(case, **kw)
    assert not torch.equal(toks, case.tokens)


def test_penalty_state_init_reference():
    V = 50
    st = torch.full((3, V), 7, dtype=torch.int32)
    toks = [4, 4, 9, -1, 50, 49, 4, 9, 1000000, 0]
    ops.penalty_state_init(st, 1, toks, 4)
    assert torch.equal(st[1], sc.recount(toks, 4, V))
    assert bool((st[0] == 7).all()) and bool((st[2] == 7).all())
    ops.penalty_state_init(st, 1, [3, 3], 2)       # empty output: flags only, the old row is gone
    assert torch.equal(st[1], sc.recount([3, 3], 2, V))
    ops.penalty_state_init(st, 2, [], 0)
    assert int(st[2].abs().sum()) == 0


def test_logprobs_reference():
    case = sc.logprob_case(1000)
    vals, ids = ops.token_logprobs(case.logits, case.tokens, case.N, case.row_n)
    assert torch.equal(ids, case.ids)
    ok = torch.isfinite(case.vals)
    assert torch.equal(ok, torch.isfinite(vals))
    assert float((vals[ok].double() - case.vals[ok]).abs().max()) <= 1e-4
    assert ids[0, 1:].tolist() == torch.sort(case.logits[0], descending=True, stable=True).indices[:5].tolist()
    assert ids[1, 0] == case.tokens[1] and ids[1, 1:].tolist() == [-1] * 5 and ids[2].tolist() == [-1] * 6


# ---------------------------------------------------------------------- engine
def test_greedy_repetition_penalty_matches_hf_generate():
    tr = pytest.importorskip("transformers")
    from shai_amd.weights import load_into
    c = TINY
    hc = tr.LlamaConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                        num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                        num_key_value_heads=c.num_key_value_heads, head_dim=c.head_dim, rms_norm_eps=c.rms_norm_eps,
                        rope_theta=c.rope_theta, max_position_embeddings=c.max_position_embeddings,
                        tie_word_embeddings=False)
    torch.manual_seed(0)
    hf = tr.LlamaForCausalLM(hc).eval()
    with torch.no_grad():
        for p in hf.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    eng = _engine(enable_prefix_caching=False)
    load_into(eng.model, {k: v.clone() for k, v in hf.state_dict().items()}, eng.model.convert_hf_state_dict,
              strict=True)
    prompt = PROMPTS[0]
    with torch.no_grad():
        want = hf.generate(torch.tensor([prompt]), max_new_tokens=8, do_sample=False, repetition_penalty=1.3,
                           eos_token_id=None, pad_token_id=0)[0, len(prompt):].tolist()
        plain = hf.generate(torch.tensor([prompt]), max_new_tokens=8, do_sample=False, eos_token_id=None,
                            pad_token_id=0)[0, len(prompt):].tolist()
    got = eng.generate([prompt], SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True,
                                                repetition_penalty=1.3))[0].output
    assert got == want
    assert want != plain or len(set(plain)) == len(plain)   # (the penalty matters unless greedy never repeats)


def _run(eng, params, prompts=PROMPTS):
    seqs = [eng.add_request(p, q) for p, q in zip(prompts, params)]
    while eng.has_work():
        eng.step()
    return seqs


def test_async_equals_sync_mixed_batch():
    out = {}
    for a in (True, False):
        eng = _engine(async_decode=a)
        seqs = _run(eng, _mixed_params())
        out[a] = [(s.output, s.logprobs, s.finish_reason) for s in seqs]
        for s in seqs:
            n = s.params.logprobs
            assert len(s.logprobs) == (0 if n is None else len(s.output))
            for tok, e in zip(s.output, s.logprobs):
                assert e["token"] == tok and len(e["top_ids"]) == n == len(e["top_logprobs"])
                assert e["top_logprobs"] == sorted(e["top_logprobs"], reverse=True)
                assert n == 0 or e["logprob"] <= e["top_logprobs"][0]
        assert eng.bm.num_free == eng.num_kv_blocks and sorted(eng._pen_free) == list(range(4))
    assert out[True] == out[False]
    assert out[True][1][2] == "stop" or len(out[True][1][0]) == 12


def test_neutral_engine_allocates_nothing_and_keeps_its_graph_keys():
    eng = _engine()
    p = [SamplingParams(max_tokens=4, temperature=t, ignore_eos=True) for t in (0.0, 0.7, 0.7, 0.0)]
    seqs = _run(eng, p)
    assert eng.pen_state is None and eng._lp_host is None
    assert all(s.pen_row == -1 and s.logprobs == [] for s in seqs)
    assert all(len(k) == 4 and k[:3] == (k[0], False, False) for k in eng._graphs)     # (Bc, cross, greedy, splits)
    assert all(g.NF == 9 for g in eng._graphs.values())
    # a plain greedy sequence batched with a penalised one produces the tokens it produces alone.  (Sampled plain
    # rows are compared on the GPU, where both batches run the kernel: the CPU engine's plain path orders equal
    # logits as torch.topk happens to, the oracle by ascending index, and the tiny model's logits do tie.)
    alone = [s.output for s in seqs]
    eng2 = _engine()
    q = list(p)
    q[0] = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True, repetition_penalty=1.5, logprobs=1)
    both = _run(eng2, q)
    assert both[3].output == alone[3] and all(len(s.output) == 4 for s in both)
    assert eng2.pen_state is not None and tuple(eng2.pen_state.shape) == (4, TINY.vocab_size)
    assert any(len(k) == 5 and k[4] == ("pen", 2, "logprobs", True) for k in eng2._graphs)


def test_state_row_is_a_recount_of_the_tokens():
    eng = _engine(async_decode=False)
    s = eng.add_request(PROMPTS[2], SamplingParams(max_tokens=12, temperature=0.9, seed=4, ignore_eos=True,
                                                   repetition_penalty=1.2, frequency_penalty=0.3))
    other = eng.add_request(PROMPTS[1], SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True))
    while len(s.output) < 7:
        eng.step()
    assert s.pen_row >= 0 and other.pen_row == -1 and s.n_prompt0 == len(PROMPTS[2])
    V = TINY.vocab_size
    assert torch.equal(eng.pen_state[s.pen_row], sc.recount(s.tokens, s.n_prompt0, V))
    # rebuilt mid-generation from the host-known tokens, split at the original prompt length: the live row
    fresh = torch.full((2, V), -1, dtype=torch.int32)
    ops.penalty_state_init(fresh, 1, s.tokens, s.n_prompt0)
    assert torch.equal(fresh[1], eng.pen_state[s.pen_row])
    while eng.has_work():
        eng.step()
    assert s.pen_row == -1 and sorted(eng._pen_free) == list(range(4))


def test_preempted_sequence_keeps_its_penalties():
    """Preemption moves the output into the prompt; the state rebuilt on re-admission still flags only the
    original prompt and counts the rest, so generation continues as if nothing had happened."""
    p = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.4)
    want = _run(_engine(async_decode=False), [p], [PROMPTS[0]])[0].output
    eng = _engine(async_decode=False)
    s = eng.add_request(PROMPTS[0], p)
    while len(s.output) < 5:
        eng.step()
    # what _decode does to a sequence it cannot give a block
    eng._free(s)
    s.n_cached, s.prefill_started = 0, False
    s.prompt, s.output = s.prompt + s.output, []
    eng.running.remove(s)
    eng.waiting.insert(0, s)
    assert s.pen_row == -1
    while eng.has_work():
        eng.step()
    # (the re-admitted sequence counts max_tokens anew, as it always has: compare what both runs generated)
    assert s.n_prompt0 == len(PROMPTS[0]) and s.tokens[s.n_prompt0:][:len(want)] == want


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                                dict(presence_penalty=2.5), dict(frequency_penalty=-2.01), dict(min_p=1.5),
                                dict(min_p=-0.1), dict(logprobs=21), dict(logprobs=-1), dict(logprobs=1.5),
                                dict(repetition_penalty=float("nan"))])
def test_validation_errors(kw):
    eng = _engine()
    with pytest.raises(ValueError):
        eng.add_request([1, 2, 3], SamplingParams(**kw))
    assert not eng.waiting and eng.pen_state is None
    eng.add_request([1, 2, 3], SamplingParams(repetition_penalty=2.0, presence_penalty=-2.0, frequency_penalty=2.0,
                                              min_p=1.0, logprobs=20))


def test_failed_state_allocation_fails_the_request_only(monkeypatch):
    eng = _engine()
    real = torch.zeros

    def zeros(*a, **k):
        if k.get("dtype") == torch.int32 and len(a) == 2 and a[1] == TINY.vocab_size:
            raise torch.OutOfMemoryError("out of memory")
        return real(*a, **k)
    monkeypatch.setattr(torch, "zeros", zeros)
    with pytest.raises(MemoryError, match="penalty-state"):
        eng.add_request([1, 2, 3], SamplingParams(repetition_penalty=1.2))
    assert eng.pen_state is None and not eng.waiting
    s = eng.generate([[1, 2, 3]], SamplingParams(max_tokens=3, temperature=0.0, ignore_eos=True))[0]
    assert len(s.output) == 3


# ---------------------------------------------------------------------- API
def test_api_round_trip():
    from fastapi.testclient import TestClient
    from shai_amd.serving import llm_api
    from shai_amd.serving.common import ServerEnv
    env = ServerEnv(app="mistral", pod_name="pod0", nodepool="mi355x", model_id="m", device="cpu", config="tiny",
                    num_inference_steps=2, max_new_tokens=4, max_seq_len=16, height=64, width=64)
    c = TestClient(llm_api.create_app(env=env))
    r = c.post("/generate", json={"prompt": "What model are you?", "max_new_tokens": 5})
    assert r.status_code == 200 and set(r.json()) == {"text", "execution_time"}      # the default response, unchanged
    req = {"prompt": "What model are you?", "max_new_tokens": 5, "temperature": 0.0, "repetition_penalty": 1.3,
           "presence_penalty": 0.5, "frequency_penalty": 0.5, "min_p": 0.05, "top_k": 40, "top_p": 0.95, "seed": 1,
           "logprobs": 2}
    a, b = c.post("/generate", json=req).json(), c.post("/generate", json=req).json()
    assert set(a) == {"text", "execution_time", "logprobs"} and a["text"] == b["text"]
    assert a["logprobs"] == b["logprobs"] and 1 <= len(a["logprobs"]) <= 5
    assert all(len(e["top_ids"]) == 2 and e["logprob"] <= 0 for e in a["logprobs"])
    base64.b64decode(a["text"]).decode()
    for bad in ({"repetition_penalty": 0}, {"presence_penalty": 3}, {"frequency_penalty": -3}, {"min_p": 2},
                {"logprobs": 21}, {"logprobs": -1}, {"temperature": -1}, {"top_p": 0}):
        assert c.post("/generate", json={"prompt": "x", "max_new_tokens": 2, **bad}).status_code == 422, bad
    assert c.post("/generate", json={"prompt": "x", "max_new_tokens": 2}).status_code == 200
