"""Constrained sampling without a GPU: the oracle against transformers' logits processors, the exact cases against
the oracle and its mutants, the compiler, and the engine-level properties on the CPU engine (which keeps the same pool
and state words as CPU tensors and samples through the oracle)."""
import base64
import dataclasses
import pickle

import pytest
import torch

import constraint_cases as cc
from shai_amd import ops
from shai_amd.engines import constraints as cn
from shai_amd.engines.llm import LLMEngine, SamplingParams
from shai_amd.models.llama import LlamaConfig
from shai_amd.ops import reference as ref

TINY = LlamaConfig.tiny()
V_TINY = TINY.vocab_size
EOS = TINY.eos_token_id
PROMPTS = [[3, 17, 99, 250, 7, 7, 400, 12], [5, 6, 7], [9, 9, 9, 9, 41], list(range(20, 90))]


def _engine(**kw):
    kw.setdefault("max_num_seqs", 4)
    kw.setdefault("max_model_len", 256)
    return LLMEngine(TINY, device="cpu", **kw)


def _run(eng, params, prompts=PROMPTS):
    seqs = [eng.add_request(p, q) for p, q in zip(prompts, params)]
    while eng.has_work():
        eng.step()
    return seqs


def _mixed_params():
    return [SamplingParams(max_tokens=9, temperature=0.9, seed=3, guided_choice=[[5, 6, 7], [5, 9], [11]]),
            SamplingParams(max_tokens=12, temperature=0.8, seed=11, frequency_penalty=0.5, presence_penalty=0.25,
                           min_p=0.05, ignore_eos=True),
            SamplingParams(max_tokens=10, temperature=0.7, seed=5, min_tokens=6, logit_bias={EOS: 100.0, 17: -100.0},
                           bad_words_ids=[[40], [41, 42]], allowed_token_ids=list(range(0, 200)),
                           repetition_penalty=1.2),
            SamplingParams(max_tokens=8, temperature=0.9, ignore_eos=True, seed=2)]


# ---------------------------------------------------------------------- the rule
def _one_state_rows(p, V, B, stop=(cc.EOS,), state=0):
    prog = cn.compile_program(p, list(stop), V)
    pv = ref.con_view(prog.words, 0, V)
    return prog, [(pv, b, state) for b in range(B)]


def test_oracle_matches_transformers_processors():
    tr = pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(0)
    B, V = 4, 333
    scores = torch.randn(B, V, generator=g) * 4
    ids = torch.randint(0, V, (B, 12), generator=g)
    none = (None, torch.ones(B), torch.zeros(B), torch.zeros(B))
    ban0 = torch.zeros(B, dtype=torch.int32)
    # logit_bias
    bias = {7: 2.5, 100: -100.0, 332: 0.75, 1: -3.0}      # (transformers refuses token id 0 here)
    want = tr.SequenceBiasLogitsProcessor([[[k], v] for k, v in bias.items()])(ids, scores.clone())
    _, rows = _one_state_rows(cc.params_of(logit_bias=bias), V, B)
    assert torch.equal(ref.constrain_logits(scores, *none, rows, ban0), want)
    # bad words: single tokens and sequences, each batch row in the state its own history leads to
    words = [[5], [int(ids[0, -1]), 9], [int(ids[1, -2]), int(ids[1, -1]), 11], [int(ids[1, -1]), 12]]
    want = tr.NoBadWordsLogitsProcessor(words, eos_token_id=cc.EOS)(ids, scores.clone())
    prog = cn.compile_program(cc.params_of(bad_words_ids=words), [cc.EOS], V)
    pv = ref.con_view(prog.words, 0, V)
    rows = [(pv, b, prog.replay(ids[b].tolist())) for b in range(B)]
    got = ref.constrain_logits(scores, *none, rows, ban0)
    assert torch.equal(torch.isfinite(got), torch.isfinite(want)) and torch.equal(got[torch.isfinite(got)],
                                                                                 want[torch.isfinite(want)])
    assert not torch.isfinite(got[0, 9]) and not torch.isfinite(got[1, 11]) and not torch.isfinite(got[1, 12])
    # min_tokens
    _, rows = _one_state_rows(cc.params_of(min_tokens=4, stop_token_ids=[50]), V, B, stop=(cc.EOS, 50))
    for n_new in (0, 3, 4, 9):
        hf = tr.MinNewTokensLengthLogitsProcessor(12 - n_new, 4, [cc.EOS, 50])(ids, scores.clone())
        ban = torch.full((B,), int(ref.ban_stop(n_new, 4)), dtype=torch.int32)
        got = ref.constrain_logits(scores, *none, rows, ban)
        assert torch.equal(got, hf), n_new
    # the trie
    choices = [[5, 6, 7], [5, 9], [11]]
    prog = cn.compile_program(cc.params_of(guided_choice=choices), [cc.EOS], V)
    pv = ref.con_view(prog.words, 0, V)

    def allowed_fn(_, sent):
        sent = sent.tolist()
        nxt = {c[len(sent)] for c in choices if c[:len(sent)] == sent and len(c) > len(sent)}
        return sorted(nxt | ({cc.EOS} if sent in choices else set()))
    for hist in ([], [5], [5, 6], [5, 6, 7], [5, 9], [11]):
        inp = torch.tensor([hist] * B, dtype=torch.long).reshape(B, len(hist))
        hf = tr.PrefixConstrainedLogitsProcessor(allowed_fn, 1)(inp, scores.clone())
        got = ref.constrain_logits(scores, *none, [(pv, b, prog.replay(hist)) for b in range(B)], ban0)
        assert torch.equal(got, hf), hist


@pytest.mark.parametrize("V", cc.VOCABS[:2])
def test_exact_cases_oracle_fp32_equals_fp64(V):
    case = cc.exact_batch(V)
    toks, pst, cst = cc.run_calls(case)
    assert torch.equal(toks, case.tokens)
    assert torch.equal(pst, case.pstates[-1]) and torch.equal(cst, case.cstates[-1])
    # the rows do what their names say
    i, t = case.ids, case.tokens
    assert set(t[:, 1].tolist()) <= set(i.allowed3) and t[0, 1] == i.allowed3[2] and t[0, 7] == i.allowed3[2]
    assert t[0, 2] != V - 1 and t[:, 3].tolist()[0] == i.z
    assert cc.EOS not in t[:2, 4].tolist() and t[2, 4] == cc.EOS
    assert t[:, 5].tolist() == [i.wa, i.wc, i.wb]
    assert t[:2, 6].tolist() == [i.g1, i.g2] and int(t[2, 6]) in i.stop
    # canaries: the even state words, and the word of the row without a program
    final = case.cstates[-1]
    assert torch.equal(final[0::2], case.cstates[0][0::2]) and final[1] == 999
    assert any(not torch.equal(a, b) for a, b in zip(case.cstates[:-1], case.cstates[1:]))


MUTANTS = {"mask_after_topk": dict(topk_first=True), "bias_after_penalties": dict(bias_last=True),
           "state_not_advanced": dict(advance=False), "ban_stop_off_by_one": dict(ban_rule=lambda g, m: g <= m),
           "pad_bits_allowed": dict(pad_allowed=True), "zero_mass_tail_kept": dict(candidates=cc.mutant_tail_kept)}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutants_of_the_rule_change_a_token(name):
    changed = []
    for V in cc.VOCABS[:2]:
        case = cc.exact_batch(V)
        toks = cc.run_calls(case, **MUTANTS[name])[0]
        changed.append(not torch.equal(toks, case.tokens))
    assert all(changed), (name, changed)        # (both sizes have a partial last mask word)


# ---------------------------------------------------------------------- the compiler
def test_aho_corasick_bans_equal_a_brute_force_suffix_check():
    g = torch.Generator().manual_seed(1)
    V = 40
    for trial in range(20):
        n = int(torch.randint(1, 8, (1,), generator=g))
        words = [torch.randint(0, 4, (int(torch.randint(2, 5, (1,), generator=g)),), generator=g).tolist()
                 for _ in range(n)] + [[0, 1, 0], [1, 0], [0, 0, 1, 0, 2]]             # overlapping on purpose
        singles = [[7]]
        prog = cn.compile_program(cc.params_of(bad_words_ids=words + singles), [cc.EOS], V)
        pv = ref.con_view(prog.words, 0, V)
        stream = torch.randint(0, 5, (200,), generator=g).tolist()
        st = 0
        for i in range(len(stream) + 1):
            out = stream[:i]
            banned = {w[-1] for w in words if out[len(out) - (len(w) - 1):] == w[:-1] and len(out) >= len(w) - 1}
            banned.add(7)
            allowed = ref.con_mask_bits(pv.masks[st], V)
            assert set((~allowed).nonzero().reshape(-1).tolist()) == banned, (trial, i)
            if i < len(stream):
                assert ref.con_next(pv, st, stream[i]) == prog.advance(st, stream[i])
                st = prog.advance(st, stream[i])
        # explicit edges never lead to the root, and every default does
        assert all(nx != 0 for e in prog.edges for nx in e.values()) and set(prog.default) == {0}


def test_trie_programs():
    V, stop = 100, [cc.EOS, 50]
    choices = [[5, 6, 7], [5, 9], [11], [5]]
    prog = cn.compile_program(cc.params_of(guided_choice=choices), stop, V)
    pv = ref.con_view(prog.words, 0, V)
    al = lambda hist: set(ref.con_mask_bits(pv.masks[prog.replay(hist)], V).nonzero().reshape(-1).tolist())
    assert al([]) == {5, 11} and al([5]) == {6, 9, 2, 50} and al([5, 6]) == {7}
    assert al([5, 6, 7]) == al([11]) == al([5, 9]) == {2, 50}
    assert prog.S == 6 and set(ref.con_mask_bits(pv.stop, V).nonzero().reshape(-1).tolist()) == {2, 50}
    assert int(pv.masks[:, -1].max()) < 2 ** (V % 32) and int(pv.masks[:, -1].min()) >= 0     # pad bits are zero
    # sharing: equal options give equal keys and equal words
    again = cn.compile_program(cc.params_of(guided_choice=[list(c) for c in choices]), stop, V)
    assert torch.equal(again.words, prog.words)
    assert cn.program_key(cc.params_of(guided_choice=choices), stop, V) == \
        cn.program_key(cc.params_of(guided_choice=[list(c) for c in choices]), list(reversed(stop)), V)


BAD = [dict(logit_bias={V_TINY: 1.0}), dict(logit_bias={-1: 1.0}), dict(logit_bias={3: 101.0}),
       dict(logit_bias={3: float("nan")}), dict(logit_bias={i: 0.5 for i in range(301)}), dict(logit_bias=[1, 2]),
       dict(allowed_token_ids=[]), dict(allowed_token_ids=[V_TINY]), dict(allowed_token_ids=[1.5]),
       dict(bad_words_ids=[[]]), dict(bad_words_ids=[[1, V_TINY]]), dict(bad_words_ids=[3]),
       dict(min_tokens=-1), dict(min_tokens=1.5), dict(min_tokens=9, max_tokens=8),
       dict(guided_choice=[]), dict(guided_choice=[[]]), dict(guided_choice=[[1, V_TINY]]),
       dict(guided_choice=[[5]], ignore_eos=True), dict(guided_choice=[[5]], min_tokens=1),
       dict(guided_choice=[[5]], bad_words_ids=[[7, 8]]), dict(guided_choice=[[5, EOS]]),
       dict(guided_choice=[[5, 6]], bad_words_ids=[[6]]), dict(guided_choice=[[5, 6]], allowed_token_ids=[5, 6]),
       dict(allowed_token_ids=[EOS], min_tokens=2), dict(allowed_token_ids=[7], bad_words_ids=[[7]]),
       dict(bad_words_ids=[list(range(3, 503)), list(range(4, 504)), list(range(5, 505))])]


@pytest.mark.parametrize("kw", BAD, ids=[str(i) for i in range(len(BAD))])
def test_validation_errors(kw):
    eng = _engine(max_model_len=1024)
    with pytest.raises(ValueError):
        eng.add_request([1, 2, 3], SamplingParams(**kw))
    assert not eng.waiting and eng.con_pool is None and eng.con_state is None


def test_state_cap_is_named_and_valid_combinations_pass():
    with pytest.raises(ValueError, match="1024"):
        cn.compile_program(cc.params_of(bad_words_ids=[list(range(3, 603)), list(range(4, 604))]), [EOS], 2000)
    with pytest.raises(ValueError, match="1024"):
        cn.compile_program(cc.params_of(guided_choice=[[i % 500 + 3, j + 3] for i in range(40) for j in range(30)]),
                           [EOS], V_TINY)
    assert cn.compile_program(cc.params_of(bad_words_ids=[list(range(3, 3 + 1024))]), [EOS], 2000).S == 1024   # the cap itself
    eng = _engine()
    eng.add_request([1, 2, 3], SamplingParams(guided_choice=[[5, 6]], bad_words_ids=[[9]], logit_bias={5: -100.0},
                                              allowed_token_ids=[5, 6, EOS], max_tokens=8))
    eng.add_request([1, 2, 3], SamplingParams(min_tokens=8, max_tokens=8, bad_words_ids=[[1, 2], [3]],
                                              logit_bias={0: 100, V_TINY - 1: -100}))


# ---------------------------------------------------------------------- the engine (CPU)
def test_async_equals_sync_mixed_batch():
    out = {}
    for a in (True, False):
        eng = _engine(async_decode=a)
        seqs = _run(eng, _mixed_params())
        out[a] = [(s.output, s.finish_reason) for s in seqs]
        assert eng.bm.num_free == eng.num_kv_blocks and sorted(eng._con_free) == list(range(4))
        assert all(e.refs == 0 for e in eng.con_pool.entries.values()) and len(eng.con_pool.entries) == 2
    assert out[True] == out[False]
    (g_out, g_why), _, (m_out, m_why), _ = out[True]
    assert g_why == "stop" and g_out[:-1] in ([5, 6, 7], [5, 9], [11]) and g_out[-1] == EOS
    assert len(m_out) >= 7 and EOS not in m_out[:6] and all(t < 200 and t not in (17, 40) for t in m_out)
    assert not any(m_out[i:i + 2] == [41, 42] for i in range(len(m_out)))
    assert m_out[6] == EOS and m_why == "stop"       # +100 on EOS: it comes the moment min_tokens lets it


def test_neutral_engine_allocates_nothing_and_a_plain_neighbour_is_unmoved():
    eng = _engine()
    p = [SamplingParams(max_tokens=4, temperature=t, ignore_eos=True) for t in (0.0, 0.7, 0.7, 0.0)]
    seqs = _run(eng, p)
    assert eng.con_pool is None and eng.con_state is None
    assert all(s.con is None and s.con_slot == -1 for s in seqs)
    assert all(len(k) == 4 for k in eng._graphs) and all(g.NF == 9 and not g.con for g in eng._graphs.values())
    # a plain greedy sequence batched with a constrained one produces the tokens it produces alone (sampled plain
    # rows are compared on the GPU: see the same remark in test_sampler_penalties_cpu.py)
    alone = [s.output for s in seqs]
    eng2 = _engine()
    q = list(p)
    q[0] = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True, allowed_token_ids=[7, 8, 9])
    both = _run(eng2, q)
    assert both[3].output == alone[3] and set(both[0].output) <= {7, 8, 9} and len(both[0].output) == 4
    assert eng2.con_pool is not None and eng2.con_state.numel() == 4
    assert all(k[-1] == ("con",) and g.NF == 18 for k, g in eng2._graphs.items())


def test_preempted_sequence_resumes_in_the_right_state():
    p = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True, bad_words_ids=[[7, 7, 7], [400, 12]],
                       logit_bias={7: 100.0})
    want = _run(_engine(async_decode=False), [p], [PROMPTS[0]])[0].output
    assert want[:3] == [7, 7] + [want[2]] and want[2] != 7 and [7, 7, 7] not in [want[i:i + 3] for i in range(10)]
    for cut in (1, 2, 5):
        eng = _engine(async_decode=False)
        s = eng.add_request(PROMPTS[0], p)
        while len(s.output) < cut:
            eng.step()
        eng._free(s)                                   # what _decode does to a sequence it cannot give a block
        s.n_cached, s.prefill_started = 0, False
        s.prompt, s.output = s.prompt + s.output, []
        eng.running.remove(s)
        eng.waiting.insert(0, s)
        assert s.con_slot == -1 and s.con is not None and s.con.refs == 1
        while eng.has_work():
            eng.step()
        assert s.tokens[s.n_prompt0:][:len(want)] == want, cut
        assert s.con is None and sorted(eng._con_free) == list(range(4))


def test_guided_choice_output_is_a_choice_for_20_seeds():
    choices = [[5, 6, 7], [5, 9], [11], [300, 301, 302, 303]]
    eng = _engine(max_num_seqs=8)
    seen = set()
    for lo in (0, 10):
        ps = [SamplingParams(max_tokens=9, temperature=1.0, top_k=0 if seed % 2 else 50, seed=seed,
                             guided_choice=choices) for seed in range(lo, lo + 10)]
        for s in _run(eng, ps[:8], [[1, 2, 3 + i] for i in range(8)]) + _run(eng, ps[8:], [[4, 5], [6]]):
            assert s.finish_reason == "stop" and s.output[-1] == EOS and s.output[:-1] in choices, s.output
            seen.add(tuple(s.output))
    assert len(seen) > 1 and len(eng.con_pool.entries) == 1


def test_min_tokens_holds_an_eos_greedy_model_off():
    for n in (0, 1, 4, 7):
        p = SamplingParams(max_tokens=7, temperature=0.0, logit_bias={EOS: 100.0}, min_tokens=n)
        for a in (True, False):
            s = _run(_engine(async_decode=a), [p], [PROMPTS[1]])[0]
            assert len(s.output) == min(n + 1, 7) and EOS not in s.output[:n], (n, s.output)
            assert s.output[-1] == EOS if n < 7 else s.finish_reason == "length"


def test_failed_pool_allocation_fails_that_request_only(monkeypatch):
    monkeypatch.setenv(cn.POOL_ENV, "0.0004")          # 104 words: one 1-state program of this vocabulary (59), not two
    eng = _engine()
    big = SamplingParams(max_tokens=3, bad_words_ids=[[3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]])
    with pytest.raises(MemoryError, match=cn.POOL_ENV):
        eng.add_request([1, 2, 3], big)
    assert eng.con_pool is None and not eng.waiting
    small = SamplingParams(max_tokens=3, temperature=0.0, ignore_eos=True, allowed_token_ids=[4, 5])
    a = eng.add_request([1, 2, 3], small)
    other = dataclasses.replace(small, allowed_token_ids=[6, 7])
    with pytest.raises(MemoryError, match=cn.POOL_ENV):   # the live program holds the pool: no room, nothing evicted
        eng.add_request([1, 2, 3], other)
    b = eng.add_request([1, 2, 3], SamplingParams(max_tokens=3, temperature=0.0, ignore_eos=True))
    while eng.has_work():
        eng.step()
    assert set(a.output) <= {4, 5} and len(a.output) == 3 and len(b.output) == 3
    c = eng.add_request([1, 2, 3], other)               # the finished request's program is evicted for this one
    while eng.has_work():
        eng.step()
    assert set(c.output) <= {6, 7} and len(eng.con_pool.entries) == 1

    real = torch.zeros

    def boom(*a, **k):
        if k.get("dtype") == torch.int32:              # the pool buffer (the compiler's masks are bool)
            raise torch.OutOfMemoryError("out of memory")
        return real(*a, **k)
    eng2 = _engine()
    monkeypatch.setattr(cn.torch, "zeros", boom)
    with pytest.raises(MemoryError, match=cn.POOL_ENV):
        eng2.add_request([1, 2, 3], small)
    monkeypatch.undo()
    assert eng2.con_pool is None and len(eng2.generate([[1, 2, 3]], SamplingParams(max_tokens=2))[0].output) >= 1


def test_ops_entry_runs_the_oracle_on_cpu_tensors():
    case = cc.exact_batch(1000)
    pst, cst = case.pstates[0].clone(), case.cstates[0].clone()
    for c in range(cc.CALLS):
        out = torch.empty(case.B, dtype=torch.int32)
        ops.sample_constrained(case.logits, case.temps[c], case.top_k, case.top_p[c], case.u[c], out, pst, case.rows,
                               case.rep, case.freq, case.pres, case.min_p[c], case.pool, cst, case.prog, case.slot,
                               case.bans[c])
        assert torch.equal(out.long(), case.tokens[c])
    assert torch.equal(cst, case.cstates[-1]) and torch.equal(pst, case.pstates[-1])
    ops.constraint_state_init(cst, 2, 5)
    assert cst[2] == 5
    with pytest.raises(ValueError):
        ops.constraint_state_init(cst, cst.numel(), 0)


# ---------------------------------------------------------------------- API
def test_api_round_trip_and_422s():
    from fastapi.testclient import TestClient
    from shai_amd.serving import llm_api
    from shai_amd.serving.common import ServerEnv
    env = ServerEnv(app="mistral", pod_name="pod0", nodepool="mi355x", model_id="m", device="cpu", config="tiny",
                    num_inference_steps=2, max_new_tokens=4, max_seq_len=16, height=64, width=64)
    app = llm_api.create_app(env=env)
    c = TestClient(app)
    tok = app.state.service.tokenizer
    yes, no = tok.encode("yes", add_special_tokens=False), tok.encode("no thanks", add_special_tokens=False)
    req = {"prompt": "What model are you?", "max_new_tokens": 6, "temperature": 1.0, "seed": 4,
           "guided_choice": ["yes", "no thanks"], "logit_bias": {str(yes[0]): 1.5}, "allowed_token_ids":
           sorted(set(yes + no + [EOS])), "bad_words": ["maybe"], "min_tokens": 0}
    r = c.post("/generate", json=req)
    assert r.status_code == 200, r.text
    assert base64.b64decode(r.json()["text"]).decode().strip() in (tok.decode(yes, skip_special_tokens=True).strip(),
                                                                   tok.decode(no, skip_special_tokens=True).strip())
    r = c.post("/generate", json={"prompt": "x", "max_new_tokens": 5, "temperature": 0.0, "min_tokens": 5,
                                  "logit_bias": {str(EOS): 100}, "bad_words_ids": [[7, 8]],
                                  "guided_choice_ids": None})
    assert r.status_code == 200, r.text
    for bad in ({"logit_bias": {"x": 1.0}}, {"logit_bias": {"3": 101}}, {"logit_bias": {str(V_TINY): 1.0}},
                {"allowed_token_ids": []}, {"allowed_token_ids": [V_TINY + 5]}, {"min_tokens": -1},
                {"min_tokens": 3}, {"bad_words_ids": [[]]}, {"guided_choice_ids": [[1, V_TINY]]},
                {"guided_choice": ["yes"], "min_tokens": 1}, {"bad_words": [""]}, {"guided_choice": []}):
        assert c.post("/generate", json={"prompt": "x", "max_new_tokens": 2, **bad}).status_code == 422, bad
    assert c.post("/generate", json={"prompt": "x", "max_new_tokens": 2}).status_code == 200
    # without a tokenizer the string forms are rejected, the id forms work
    app.state.service.tokenizer, keep = None, tok
    try:
        assert c.post("/generate", json={"prompt": "x", "max_new_tokens": 2, "bad_words": ["a"]}).status_code == 422
    finally:
        app.state.service.tokenizer = keep


def test_params_survive_pickling():
    p = _mixed_params()[2]
    q = pickle.loads(pickle.dumps(p))
    assert q == p and cn.program_key(q, [EOS], V_TINY) == cn.program_key(p, [EOS], V_TINY)
    assert torch.equal(cn.compile_program(q, [EOS], V_TINY).words, cn.compile_program(p, [EOS], V_TINY).words)
