"""The constrained sampler on the GPU against the oracle (tests/constraint_cases.py), and the engine-level properties
with graphs, async decode and the full-vocabulary route."""
import dataclasses

import pytest
import torch

import constraint_cases as cc
from shai_amd import ops
from shai_amd.engines.llm import LLMEngine, SamplingParams
from shai_amd.models.llama import LlamaConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
d = lambda t: t.to(DEV).contiguous()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("V", cc.VOCABS)
def test_exact_cases_states_and_canaries(V, dt):
    """Token equality with the fp64 expectation over three consecutive calls; after each call the automaton state
    words are the expectation's (the canaries among them untouched); the penalty state is the expectation's."""
    case = cc.exact_batch(V)
    logits = case.logits.to(DEV, DTYPES[dt])
    pst, cst, pool = d(case.pstates[0]), d(case.cstates[0]), d(case.pool)
    for c in range(cc.CALLS):
        out = torch.full((case.B,), -7, dtype=torch.int32, device=DEV)
        ops.sample_constrained(logits, d(case.temps[c]), d(case.top_k), d(case.top_p[c]), d(case.u[c]), out, pst,
                               d(case.rows), d(case.rep), d(case.freq), d(case.pres), d(case.min_p[c]), pool, cst,
                               d(case.prog), d(case.slot), d(case.bans[c]))
        print("call", c, "picked", out.tolist(), "expected", case.tokens[c].tolist())
        assert torch.equal(out.cpu().long(), case.tokens[c])
        assert torch.equal(cst.cpu(), case.cstates[c + 1])
        assert torch.equal(pst.cpu(), case.pstates[c + 1])
    assert torch.equal(cst.cpu()[0::2], case.cstates[0][0::2]) and int(cst[1]) == 999
    assert torch.equal(pool.cpu(), case.pool)
    for r in (0, 3):
        assert torch.equal(pst[r].cpu(), case.pstates[0][r])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_rows_without_a_program_take_the_penalised_path(dt):
    """Every program offset -1 (junk in the slot / ban fields, a pool and state words present): bit for bit the
    tokens and the penalty state of ops.sample_penalized on the same inputs; no state word moves."""
    import sampler_cases as sc
    case = sc.exact_batch(32003)
    con = cc.exact_batch(32003)
    logits = case.logits.to(DEV, DTYPES[dt])
    st_a, st_b = d(case.states[0]), d(case.states[0])
    pool, cst = d(con.pool), d(con.cstates[0])
    none = torch.full((case.B,), -1, dtype=torch.int32, device=DEV)
    slot = torch.arange(case.B, dtype=torch.int32, device=DEV)
    ban = torch.ones(case.B, dtype=torch.int32, device=DEV)
    for c in range(sc.CALLS):
        a = torch.empty(case.B, dtype=torch.int32, device=DEV)
        b = torch.empty(case.B, dtype=torch.int32, device=DEV)
        args = (logits, d(case.temps[c]), d(case.top_k), d(case.top_p[c]), d(case.u[c]))
        pen = (d(case.rows), d(case.rep), d(case.freq), d(case.pres), d(case.min_p[c]))
        ops.sample_penalized(*args, a, st_a, *pen)
        ops.sample_constrained(*args, b, st_b, *pen, pool, cst, none, slot, ban)
        assert torch.equal(a, b) and torch.equal(a.cpu().long(), case.tokens[c])
        assert torch.equal(st_a, st_b)
    assert torch.equal(cst.cpu(), con.cstates[0])


def test_general_values_membership():
    """Random bf16 logits, non-dyadic penalties and biases, random allow-masks: every pick lies in the oracle's kept
    set and is allowed, over 200 uniforms."""
    case = cc.general_case()
    g = lambda t: t[case.base].to(DEV).contiguous()
    state = case.words[case.base].to(DEV).contiguous()
    rows = torch.arange(case.B, dtype=torch.int32, device=DEV)
    cst = torch.zeros(case.B, dtype=torch.int32, device=DEV)
    out = torch.empty(case.B, dtype=torch.int32, device=DEV)
    ops.sample_constrained(g(case.logits), g(case.temps), g(case.top_k), g(case.top_p), case.u.to(DEV), out, state,
                           rows, g(case.rep), g(case.freq), g(case.pres), g(case.min_p), d(case.pool), cst,
                           g(case.prog), rows, torch.zeros_like(rows))
    picks = out.cpu().long()
    assert bool(((picks >= 0) & (picks < case.V)).all())
    inside, allowed = case.kept[case.base, picks], case.allowed[case.base, picks]
    print("kept set sizes", case.kept.sum(-1).tolist(), "allowed", case.allowed.sum(-1).tolist(), "distinct picks",
          picks.unique().numel())
    assert bool(allowed.all()), picks[~allowed].tolist()
    assert bool(inside.all()), picks[~inside].tolist()
    assert int(cst.abs().sum()) == 0                        # one-state programs: the state stays


def test_constraint_state_init_and_checks():
    cst = torch.full((5,), 7, dtype=torch.int32, device=DEV)
    ops.constraint_state_init(cst, 3, 12)
    assert cst.tolist() == [7, 7, 7, 12, 7]
    with pytest.raises(ValueError):
        ops.constraint_state_init(cst, 5, 0)
    with pytest.raises(ValueError):
        ops.constraint_state_init(cst, 0, 1024)


# ---------------------------------------------------------------------- engine
TINY = LlamaConfig.tiny()
EOS = TINY.eos_token_id
PROMPTS = [[3, 17, 99, 250, 7, 7, 400, 12], [5, 6, 7], [9, 9, 9, 9, 41], list(range(20, 90))]
CHOICES = [[5, 6, 7], [5, 9], [11]]


def _params(full_vocab=False):
    return [SamplingParams(max_tokens=9, temperature=0.9, seed=3, guided_choice=CHOICES),
            SamplingParams(max_tokens=12, temperature=0.8, seed=11, frequency_penalty=0.5, presence_penalty=0.25,
                           min_p=0.05, ignore_eos=True, bad_words_ids=[[40], [41, 42]],
                           top_k=0 if full_vocab else 50),
            SamplingParams(max_tokens=10, temperature=0.0, min_tokens=6, logit_bias={EOS: 100.0, 17: -100.0},
                           allowed_token_ids=list(range(0, 200))),
            SamplingParams(max_tokens=8, temperature=0.9, ignore_eos=True, seed=2)]


def _run(params, prompts=PROMPTS, **kw):
    eng = LLMEngine(TINY, device=DEV, max_num_seqs=4, max_model_len=256, **kw)
    with torch.inference_mode():
        seqs = [eng.add_request(p, q) for p, q in zip(prompts, params)]
        while eng.has_work():
            eng.step()
    return eng, seqs


def _outs(seqs):
    return [(s.output, s.finish_reason) for s in seqs]


def _check(seqs):
    g, b, m, _ = seqs
    assert g.finish_reason == "stop" and g.output[-1] == EOS and g.output[:-1] in CHOICES, g.output
    assert 40 not in b.output and not any(b.output[i:i + 2] == [41, 42] for i in range(len(b.output)))
    assert len(m.output) == 7 and EOS not in m.output[:6] and m.output[6] == EOS, m.output
    assert all(t < 200 and t != 17 for t in m.output)


@pytest.fixture(scope="module")
def graph_run():
    return _run(_params())


def test_engine_graph_replay_equals_eager(graph_run):
    eng, seqs = graph_run
    assert any(g.graph is not None and g.con and g.pen == 2 for g in eng._graphs.values())
    _check(seqs)
    _, eager = _run(_params(), use_graphs=False)
    assert _outs(seqs) == _outs(eager)
    assert eng.bm.num_free == eng.num_kv_blocks and sorted(eng._con_free) == list(range(4))
    assert all(e.refs == 0 for e in eng.con_pool.entries.values())


def test_engine_async_equals_sync(graph_run):
    _, sync = _run(_params(), async_decode=False)
    assert _outs(graph_run[1]) == _outs(sync)


def test_engine_plain_sequences_are_unmoved_by_constrained_neighbours():
    """The plain sequences' tokens next to constrained ones (constrained sampler, pool, state words) are their tokens
    without any of that: the same four requests with the new fields left neutral, which run today's graphs.  (No
    request can stop early, so both runs have the same batch shapes and the logits come from the same GEMM kernels;
    only the sampler differs.)"""
    ps = [SamplingParams(max_tokens=9, temperature=0.9, seed=3, ignore_eos=True, allowed_token_ids=[5, 6, 7, 9, 11]),
          SamplingParams(max_tokens=12, temperature=0.8, seed=11, ignore_eos=True, bad_words_ids=[[40], [41, 42]],
                         logit_bias={17: -100.0, 99: 2.0}),
          SamplingParams(max_tokens=10, temperature=0.7, seed=5, ignore_eos=True),
          SamplingParams(max_tokens=8, temperature=0.9, seed=2, ignore_eos=True)]
    eng, mixed = _run(ps)
    neutral = SamplingParams()
    strip = {f: getattr(neutral, f) for f in ("logit_bias", "allowed_token_ids", "bad_words_ids")}
    eng0, alone = _run([dataclasses.replace(p, **strip) for p in ps])
    assert eng0.con_pool is None and eng0.con_state is None and all(len(k) == 4 for k in eng0._graphs)
    assert any(g.con for g in eng._graphs.values()) and set(mixed[0].output) <= {5, 6, 7, 9, 11}
    assert mixed[2].output == alone[2].output and mixed[3].output == alone[3].output


def test_engine_full_vocabulary_route_with_constraints():
    eng, seqs = _run(_params(full_vocab=True))
    assert any(g.full_vocab and g.con for g in eng._graphs.values())
    _check(seqs)
    _, sync = _run(_params(full_vocab=True), async_decode=False, use_graphs=False)
    assert _outs(seqs) == _outs(sync)
