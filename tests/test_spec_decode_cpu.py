"""Speculative decoding on the CPU: the n-gram proposer, the acceptance rule, the engine's verify step against the
plain engine token for token, the fall-back to the plain path, the mask of ops.spec_attention's reference route and
the configuration surface.

The engine comparisons run fp32 models.  The CPU reference GEMM is an fp32 library call whose summation order depends
on how many rows the call has (1, a few, 16 or more), and with bf16 activations such a last-bit difference moves a
logit by a bf16 step often enough to reorder near-tied candidates; in fp32 the two engines' logits agree to ~1e-6 and
the sampler sees the same candidates.  (On the GPU the GEMMs are row-deterministic: tests/test_spec_decode_gpu.py.)"""
import base64

import pytest
import torch

import attn_edges as ae
import shai_amd.ops as ops
from shai_amd.engines.llm import LLMEngine, NgramProposer, SamplingParams, accept_drafts
from shai_amd.models.llama import LlamaConfig
from spec_cases import SPEC_CASES, Replay, Wrong

SPEC = {"method": "ngram", "num_speculative_tokens": 4}


# ----------------------------------------------------------------------------- proposer
def test_ngram_proposer_table():
    p = NgramProposer(4, 1)
    # longest m wins: the 3-gram (1 2 3) occurred before 9, the 1-gram 3 also before 7 (earlier)
    assert p.propose([3, 7, 1, 2, 3, 9, 8, 1, 2, 3], 2) == [9, 8]
    # earliest occurrence wins
    assert p.propose([5, 6, 10, 5, 6, 20, 5, 6], 1) == [10]
    # an overlapping match is allowed (the occurrence shares tokens with the suffix), the suffix itself is not one
    assert p.propose([7, 7, 7, 7, 7, 7], 3) == [7, 7]     # m = 4 at start 0: two tokens are left behind it
    assert p.propose([4, 8, 8, 8], 2) == [8]
    # a match at the very end gives fewer than k tokens
    assert p.propose([1, 2, 9, 1, 2], 4) == [9, 1, 2]
    # no hit
    assert p.propose([1, 2, 3, 4], 4) == []
    assert p.propose([5], 4) == []
    assert p.propose([], 4) == []
    # n > 1 ignores 1-gram hits
    assert NgramProposer(4, 2).propose([1, 5, 2, 5], 2) == []
    assert NgramProposer(4, 1).propose([1, 5, 2, 5], 2) == [2, 5]
    assert NgramProposer(4, 2).propose([1, 5, 2, 1, 5], 2) == [2, 1]
    # never more than k
    assert len(p.propose(list(range(10)) + list(range(10)), 3)) == 3


def test_acceptance_rule():
    # sampled[t]: the token drawn behind row t; draft[t] sat in row t + 1
    assert accept_drafts([10, 11, 12, 13, 14], [20, 21, 22, 23]) == [10]                     # none accepted
    assert accept_drafts([10, 11, 12, 13, 14], [10, 11, 12, 13]) == [10, 11, 12, 13, 14]     # all accepted
    assert accept_drafts([10, 11, 12, 13, 14], [10, 11, 99, 13]) == [10, 11, 12]             # mismatch in the middle
    assert accept_drafts([10, 11, 12, 13, 14], [10, 99, 12, 13]) == [10, 11]
    assert accept_drafts([10, 3, 3, 3, 3], []) == [10]                                       # d_b = 0
    assert accept_drafts([10, 11, 0, 0, 0], [10]) == [10, 11]                                # a cut draft


# ----------------------------------------------------------------------------- engine against the plain engine
PROMPTS = [[1, 5, 9, 200, 5, 9, 200, 5, 9], list(range(3, 90)), [7, 7, 7, 7, 7, 7]]


def _engine(spec=None, **kw):
    kw = dict(dict(max_num_seqs=4, max_model_len=256), **kw)
    eng = LLMEngine(LlamaConfig.tiny(), device="cpu", speculative=spec, **kw)
    eng.model.float()   # see the module docstring
    return eng


def _params(greedy, **kw):
    kw = dict(dict(max_tokens=24, ignore_eos=True), **kw)
    if greedy:
        return SamplingParams(temperature=0.0, **kw)
    return SamplingParams(temperature=0.9, top_k=30, top_p=0.95, seed=5, **kw)


def _gen(eng, prompts, params):
    with torch.inference_mode():
        seqs = eng.generate(prompts, params)
    assert eng.bm.num_free == eng.num_kv_blocks and eng._inflight is None
    return seqs


_plain = {}


def plain(greedy):
    """The plain engine's outputs for PROMPTS (computed once per sampling mode, shared, never modified)."""
    if greedy not in _plain:
        eng = _engine()
        _plain[greedy] = ([list(s.output) for s in _gen(eng, PROMPTS, _params(greedy))], eng.stats["steps"])
    return _plain[greedy]


@pytest.mark.parametrize("proposer", ["ngram", "oracle", "wrong", "two_right"])
@pytest.mark.parametrize("greedy", [True, False])
def test_engine_matches_plain(greedy, proposer):
    want, plain_steps = plain(greedy)
    eng = _engine(SPEC)
    assert isinstance(eng.proposer, NgramProposer)
    if proposer != "ngram":
        eng.proposer = {"oracle": Replay(PROMPTS, want), "wrong": Wrong(),
                        "two_right": Replay(PROMPTS, want, right=2)}[proposer]
    got = [list(s.output) for s in _gen(eng, PROMPTS, _params(greedy))]
    assert got == want
    st = eng.stats
    assert st["spec_steps"] > 0 and st["spec_drafted"] > 0
    if proposer == "oracle":
        assert st["spec_accepted"] == st["spec_drafted"] > 0
        assert st["steps"] < plain_steps
    if proposer == "two_right":
        assert 0 < st["spec_accepted"] < st["spec_drafted"]
    if proposer == "ngram" and greedy:
        assert st["spec_accepted"] > 0     # [7] * 6 and the repeated (5 9 200) give the proposer real hits


def _pair(greedy, params, prompts=PROMPTS, **kw):
    """(plain sequences, speculative sequences, speculative engine) with the oracle proposer fed the plain run."""
    a = _gen(_engine(**kw), prompts, params)
    eng = _engine(SPEC, **kw)
    eng.proposer = Replay(prompts, [s.output for s in a])
    b = _gen(eng, prompts, params)
    return a, b, eng


@pytest.mark.parametrize("greedy", [True, False])
def test_stop_token_inside_accepted_run(greedy):
    want, _ = plain(greedy)
    stop = want[0][6]     # lands in the middle of the second verify step's accepted run
    params = _params(greedy, stop_token_ids=[stop])
    a, b, eng = _pair(greedy, params)
    assert [s.output for s in b] == [s.output for s in a]
    assert b[0].finish_reason == "stop" and b[0].output[-1] == stop and b[0].output.count(stop) == 1
    assert len(b[0].output) <= 7 and eng.stats["spec_accepted"] > 0
    assert [s.finish_reason for s in b] == [s.finish_reason for s in a]


@pytest.mark.parametrize("greedy", [True, False])
def test_max_tokens_inside_run(greedy):
    a, b, eng = _pair(greedy, _params(greedy, max_tokens=8))    # 1 (prefill) + 5 + a run cut to 2
    assert [s.output for s in b] == [s.output for s in a]
    assert all(len(s.output) == 8 and s.finish_reason == "length" for s in b)
    assert eng.stats["spec_accepted"] == eng.stats["spec_drafted"] == 3 * (4 + 1)


def test_max_model_len_reached():
    prompts = [list(range(3, 120))]                                  # 117 tokens, max_model_len 128
    a, b, eng = _pair(True, _params(True, max_tokens=64), prompts, max_model_len=128)
    assert b[0].output == a[0].output and b[0].finish_reason == a[0].finish_reason == "length"
    assert len(b[0].prompt) + len(b[0].output) == 128
    assert eng.stats["spec_accepted"] > 0


@pytest.mark.parametrize("greedy", [True, False])
def test_small_block_pool_preempts(greedy):
    """Five blocks for three sequences that each grow into a second one.  A preempted sequence carries what it had
    generated in ``prompt`` and its ``max_tokens`` count restarts (the engine's existing rule), so how many tokens a
    sequence ends with depends on when it was preempted, which differs between the two engines: the generated tokens
    are compared over the length both have, at least ``max_tokens``."""
    prompts = [list(range(3, 60)), list(range(100, 160)), list(range(200, 262))]
    params = _params(greedy, max_tokens=30)
    full = lambda s: (s.prompt + s.output)[s.n_prompt0:]
    a = _gen(_engine(num_kv_blocks=5), prompts, params)
    eng = _engine(SPEC, num_kv_blocks=5)
    eng.proposer = Replay(prompts, [full(s) for s in a])
    b = _gen(eng, prompts, params)
    for x, y in zip(a, b):
        n = min(len(full(x)), len(full(y)))
        assert n >= 30 and full(y)[:n] == full(x)[:n]
    assert any(len(s.prompt) > s.n_prompt0 for s in b), "no sequence was preempted"
    assert eng.stats["spec_accepted"] > 0


def test_prompt_arrives_mid_decode_mixed_steps():
    """A 300-token prompt joins while two sequences decode, prefill_chunk 64: the chunks run as mixed steps whose
    decode rows are one-token rows; verify steps resume afterwards."""
    long = [(i * 7) % 500 + 3 for i in range(300)]
    params = _params(True, max_tokens=20)

    def run(spec, proposer=None):
        eng = _engine(spec, max_model_len=512, prefill_chunk=64)
        if proposer is not None:
            eng.proposer = proposer
        with torch.inference_mode():
            seqs = [eng.add_request(p, params) for p in PROMPTS[:2]]
            for _ in range(3):
                eng.step()
            seqs.append(eng.add_request(long, params))
            while any(not s.finished for s in seqs):
                eng.step()
            if eng._inflight is not None:
                eng.step()
        assert eng.bm.num_free == eng.num_kv_blocks and eng._inflight is None
        return [list(s.output) for s in seqs], eng

    want, _ = run(None)
    got, eng = run(SPEC, Replay(PROMPTS[:2] + [long], want))
    assert got == want
    assert eng.stats["spec_accepted"] > 0 and eng.stats["prefill_tokens"] >= 300


def test_prefix_caching_and_shared_prefix():
    base = list(range(5, 205))
    prompts2 = [base + [9, 9, 9]]
    params = _params(True, max_tokens=12)
    plain_eng = _engine(max_model_len=512, enable_prefix_caching=True)
    a1 = [list(s.output) for s in _gen(plain_eng, [base], params)]
    a2 = [list(s.output) for s in _gen(plain_eng, prompts2, params)]
    eng = _engine(SPEC, max_model_len=512, enable_prefix_caching=True)
    eng.proposer = Replay([base] + prompts2, a1 + a2)
    b1 = [list(s.output) for s in _gen(eng, [base], params)]
    hits = eng.stats["prefix_hit_tokens"]
    b2 = [list(s.output) for s in _gen(eng, prompts2, params)]
    assert (b1, b2) == (a1, a2)
    assert eng.stats["prefix_hit_tokens"] - hits == 192 and eng.stats["spec_accepted"] > 0


# ----------------------------------------------------------------------------- fall-back to the plain path
def test_penalties_and_logprobs_fall_back():
    prompts = PROMPTS[:2]
    ps = [SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True, repetition_penalty=1.3,
                         presence_penalty=0.5),
          SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True, logprobs=2)]

    def run(spec):
        eng = _engine(spec)
        with torch.inference_mode():
            seqs = [eng.add_request(p, q) for p, q in zip(prompts, ps)]
            while any(not s.finished for s in seqs):
                eng.step()
            if eng._inflight is not None:
                eng.step()
        assert eng.bm.num_free == eng.num_kv_blocks and eng._inflight is None
        return seqs, eng

    a, _ = run(None)
    b, eng = run(SPEC)
    assert [s.output for s in b] == [s.output for s in a]
    assert b[1].logprobs == a[1].logprobs and len(b[1].logprobs) == 10
    assert eng.stats["spec_steps"] == 0 and eng.stats["spec_drafted"] == 0
    # min_p and the full-vocabulary sampler keep a step on the plain path too
    for extra in (dict(min_p=0.1), dict(top_k=0)):
        eng = _engine(SPEC)
        _gen(eng, prompts, SamplingParams(max_tokens=4, temperature=0.8, ignore_eos=True, seed=1, **extra))
        assert eng.stats["spec_steps"] == 0


# ----------------------------------------------------------------------------- the reference route's mask
@pytest.mark.parametrize("name", list(SPEC_CASES))
def test_reference_route_mask(name):
    c = ae.paged_case(seed=7, **SPEC_CASES[name])
    assert ae.floor_of(c) <= ae.FLOOR
    ref = ae.oracle(c)
    assert ae.probes_dominate(c, ref) == 1.0
    o = ops.spec_attention(c.q, c.kc, c.vc, c.bt, c.kv_lens, c.q_lens)
    ae.check(c, o, ref, what=f"reference route {name}")
    # one key more / one key fewer per row must fail the rule
    for what, mut in (("one key more", lambda b, vis, kl: vis + 1), ("one key fewer", lambda b, vis, kl: vis - 1)):
        bad = ae.oracle(c, mutate=mut)
        with pytest.raises(AssertionError):
            ae.check(c, o, bad, what=what)


# ----------------------------------------------------------------------------- validation and configuration
@pytest.mark.parametrize("spec", [dict(SPEC, num_speculative_tokens=0), dict(SPEC, num_speculative_tokens=8),
                                  dict(SPEC, prompt_lookup_max=2, prompt_lookup_min=3),
                                  dict(SPEC, prompt_lookup_min=0), dict(SPEC, method="eagle"),
                                  {"method": "ngram"}, dict(SPEC, draft_model="x")])
def test_bad_configuration_is_rejected(spec):
    with pytest.raises(ValueError):
        LLMEngine(LlamaConfig.tiny(), device="cpu", max_num_seqs=2, max_model_len=128, speculative=spec)


def test_mllama_is_rejected():
    from shai_amd.models.mllama import MllamaConfig
    with pytest.raises(NotImplementedError):
        LLMEngine(MllamaConfig.tiny(), device="cpu", max_num_seqs=2, max_model_len=128, speculative=SPEC)


def test_defaults_and_off_by_default():
    eng = LLMEngine(LlamaConfig.tiny(), device="cpu", max_num_seqs=2, max_model_len=128, speculative=SPEC)
    assert eng.speculative == {"method": "ngram", "num_speculative_tokens": 4, "prompt_lookup_max": 4,
                               "prompt_lookup_min": 1}
    assert (eng.proposer.n_max, eng.proposer.n_min) == (4, 1) and not eng.async_decode
    off = LLMEngine(LlamaConfig.tiny(), device="cpu", max_num_seqs=2, max_model_len=128)
    assert off.speculative is None and off.proposer is None and "spec_steps" not in off.stats


def test_vllm_config_reaches_the_engine_and_api_schema(tmp_path, monkeypatch):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from shai_amd.serving import llm_api
    from shai_amd.serving.common import ServerEnv
    cfgfile = tmp_path / "vllm_config.yaml"
    cfgfile.write_text("max_num_seqs: 2\nmax_model_len: 128\nspeculative_config:\n  method: ngram\n"
                       "  num_speculative_tokens: 3\n  prompt_lookup_max: 3\n")
    monkeypatch.setenv("VLLM_CONFIG", str(cfgfile))
    env = ServerEnv(app="mistral", pod_name="pod0", nodepool="mi355x", model_id="m", device="cpu", config="tiny",
                    num_inference_steps=2, max_new_tokens=4, max_seq_len=16, height=64, width=64)
    app = llm_api.create_app(env=env)
    eng = app.state.service.engine
    assert eng.speculative == {"method": "ngram", "num_speculative_tokens": 3, "prompt_lookup_max": 3,
                               "prompt_lookup_min": 1}
    assert eng.spec_k == 3 and eng.max_num_seqs == 2
    r = TestClient(app).post("/generate", json={"prompt": "hello hello hello hello", "max_new_tokens": 6,
                                                "temperature": 0.0})
    assert r.status_code == 200
    body = r.json()
    assert set(body) == {"text", "execution_time"} and isinstance(body["execution_time"], float)
    base64.b64decode(body["text"]).decode()
    assert eng.stats["spec_steps"] > 0
