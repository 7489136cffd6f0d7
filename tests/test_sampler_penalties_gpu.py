"""The penalised sampler, the penalty-state init and the log-probability kernel on the GPU against the oracle
(tests/sampler_cases.py), and the engine-level properties with graphs, async decode and the full-vocabulary route."""
import pytest
import torch

import sampler_cases as sc
from shai_amd import ops
from shai_amd.engines.llm import LLMEngine, SamplingParams
from shai_amd.models.llama import LlamaConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _call(case, logits, state, c, rows=None):
    d = lambda t: t.to(DEV).contiguous()
    out = torch.full((case.B,), -7, dtype=torch.int32, device=DEV)
    ops.sample_penalized(logits, d(case.temps[c]), d(case.top_k), d(case.top_p[c]), d(case.u[c]), out, state,
                         d(case.rows if rows is None else rows), d(case.rep), d(case.freq), d(case.pres),
                         d(case.min_p[c]))
    return out


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("V", sc.VOCABS)
def test_exact_cases_and_state(V, dt):
    """Token equality with the oracle over three consecutive calls; the state the sampler kept is the host recount;
    rows without a state row and the canary rows either side are untouched."""
    case = sc.exact_batch(V)
    logits = case.logits.to(DEV, DTYPES[dt])
    state = case.states[0].to(DEV)
    toks = torch.stack([_call(case, logits, state, c) for c in range(sc.CALLS)]).cpu()
    print("picked", toks.tolist(), "expected", case.tokens.tolist())
    assert torch.equal(toks.long(), case.tokens)
    assert torch.equal(state.cpu(), case.states[-1])
    for r in [0, case.B + 1] + [b + 1 for b in range(case.B) if case.rows[b] < 0]:
        assert torch.equal(state[r].cpu(), case.states[0][r])
    for b in range(case.B):
        if case.rows[b] >= 0:
            assert torch.equal(state[b + 1].cpu() - case.states[0][b + 1],
                               sc.recount(case.tokens[:, b].tolist(), 0, V))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_neutral_rows_sample_as_the_plain_kernel(dt):
    """Every row without a state row, min_p 0: the penalised kernel returns the plain kernel's tokens."""
    case = sc.exact_batch(32003)
    logits = case.logits.to(DEV, DTYPES[dt])
    d = lambda t: t.to(DEV).contiguous()
    for c in range(sc.CALLS):
        plain = torch.empty(case.B, dtype=torch.int32, device=DEV)
        ops.sample(logits, d(case.temps[c]), d(case.top_k), d(case.top_p[c]), d(case.u[c]), plain)
        out = torch.empty(case.B, dtype=torch.int32, device=DEV)
        none = torch.full((case.B,), -1, dtype=torch.int32, device=DEV)
        for state in (None, case.states[0].to(DEV)):
            ops.sample_penalized(logits, d(case.temps[c]), d(case.top_k), d(case.top_p[c]), d(case.u[c]), out, state,
                                 none, d(case.rep), d(case.freq), d(case.pres), torch.zeros(case.B, device=DEV))
            assert torch.equal(out, plain)
            assert state is None or torch.equal(state.cpu(), case.states[0])


def test_penalty_state_init():
    V = 32003
    st = torch.full((3, V), 7, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, V, (700,), generator=g).tolist()
    toks += toks[:50] + [-1, V, V + 5, 2 ** 31 - 1, -2 ** 31, 0, V - 1, 4096, 4095, 4096]   # duplicates, out of range
    ops.penalty_state_init(st, 1, toks, 300)
    assert torch.equal(st[1].cpu(), sc.recount(toks, 300, V))
    assert bool((st[0] == 7).all()) and bool((st[2] == 7).all())
    ops.penalty_state_init(st, 1, toks[:9], 9)            # empty output: flags only, the old row is gone
    assert torch.equal(st[1].cpu(), sc.recount(toks[:9], 9, V))
    ops.penalty_state_init(st, 2, [], 0)                  # no tokens at all: a cleared row
    assert int(st[2].abs().sum()) == 0 and bool((st[0] == 7).all())
    small = torch.full((2, 1000), 7, dtype=torch.int32, device=DEV)
    ops.penalty_state_init(small, 0, [999, 999, 1000, 3], 1)
    assert torch.equal(small[0].cpu(), sc.recount([999, 999, 1000, 3], 1, 1000)) and bool((small[1] == 7).all())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("V", sc.VOCABS)
def test_token_logprobs(V, dt):
    """Ids equal the oracle's; values within 1e-4 of the fp64 log-softmax (the fp32 tree sum over 128k terms is good
    to ~1e-5 relative, exp / log add a few ulp: a tenfold margin); two runs are bitwise equal."""
    case = sc.logprob_case(V)
    logits = case.logits.to(DEV, DTYPES[dt])
    toks, row_n = case.tokens.to(DEV), case.row_n.to(DEV)
    runs = []
    for _ in range(2):
        vals = torch.full((4, 1 + case.N), 123.0, device=DEV)
        ids = torch.full((4, 1 + case.N), -9, dtype=torch.int32, device=DEV)
        ops.token_logprobs(logits, toks, case.N, row_n, vals, ids)
        runs.append((vals.cpu(), ids.cpu()))
    (vals, ids), (vals2, ids2) = runs
    assert torch.equal(vals, vals2) and torch.equal(ids, ids2)
    live = case.row_n >= 0
    assert torch.equal(ids[live], case.ids[live])
    assert bool((ids[~live] == -9).all()) and bool((vals[~live] == 123.0).all())       # a skipped row is not written
    ok = torch.isfinite(case.vals) & live[:, None]
    assert torch.equal(torch.isfinite(vals) & live[:, None], ok)
    err = float((vals[ok].double() - case.vals[ok]).abs().max())
    print("max |logprob - fp64|", err)
    assert err <= 1e-4
    # without per-row counts every row gets all N
    v3, i3 = ops.token_logprobs(logits, toks, case.N)
    full = sc.ref.token_logprobs(case.logits, case.tokens, case.N, dtype=torch.float64)
    assert torch.equal(i3.cpu(), full[1]) and float((v3.cpu().double() - full[0]).abs().max()) <= 1e-4


def test_general_values_membership():
    """Random bf16 logits, non-dyadic penalties: every pick lies in the oracle's kept set, over 200 uniforms."""
    case = sc.general_case()
    d = lambda t: t[case.base].to(DEV).contiguous()
    state = case.words[case.base].to(DEV).contiguous()
    rows = torch.arange(case.B, dtype=torch.int32, device=DEV)
    out = torch.empty(case.B, dtype=torch.int32, device=DEV)
    ops.sample_penalized(d(case.logits), d(case.temps), d(case.top_k), d(case.top_p), case.u.to(DEV), out, state, rows,
                         d(case.rep), d(case.freq), d(case.pres), d(case.min_p))
    picks = out.cpu().long()
    assert bool(((picks >= 0) & (picks < case.V)).all())
    inside = case.kept[case.base, picks]
    print("kept set sizes", case.kept.sum(-1).tolist(), "distinct picks", picks.unique().numel())
    assert bool(inside.all()), picks[~inside].tolist()
    # and each pick was counted once in its own state row
    delta = state.cpu() - case.words[case.base]
    assert int(delta.sum()) == case.B and bool((delta[torch.arange(case.B), picks] == 1).all())


# ---------------------------------------------------------------------- engine
TINY = LlamaConfig.tiny()
PROMPTS = [[3, 17, 99, 250, 7, 7, 400, 12], [5, 6, 7], [9, 9, 9, 9, 41], list(range(20, 90))]


def _params(full_vocab=False):
    return [SamplingParams(max_tokens=9, temperature=0.0, ignore_eos=True, repetition_penalty=1.3, logprobs=3),
            SamplingParams(max_tokens=12, temperature=0.8, seed=11, frequency_penalty=0.5, presence_penalty=0.25,
                           min_p=0.05, ignore_eos=True, top_k=0 if full_vocab else 50),
            SamplingParams(max_tokens=7, temperature=0.7, ignore_eos=True, logprobs=0, seed=5),
            SamplingParams(max_tokens=8, temperature=0.9, ignore_eos=True, seed=2)]


def _run(params, prompts=PROMPTS, **kw):
    eng = LLMEngine(TINY, device=DEV, max_num_seqs=4, max_model_len=256, **kw)
    with torch.inference_mode():
        seqs = [eng.add_request(p, q) for p, q in zip(prompts, params)]
        while eng.has_work():
            eng.step()
    return eng, seqs


def _same(a, b):
    """Same tokens, same logprob ids, logprob values bitwise equal."""
    return [(s.output, s.logprobs) for s in a] == [(s.output, s.logprobs) for s in b]


@pytest.fixture(scope="module")
def graph_run():
    return _run(_params())


def test_engine_graph_replay_equals_eager(graph_run):
    eng, seqs = graph_run
    assert any(g.graph is not None and g.pen == 2 and g.lp for g in eng._graphs.values())
    _, eager = _run(_params(), use_graphs=False)
    assert _same(seqs, eager)
    for s in seqs:
        assert len(s.logprobs) == (0 if s.params.logprobs is None else len(s.output))
        assert all(e["token"] == t for e, t in zip(s.logprobs, s.output))


def test_engine_async_equals_sync(graph_run):
    _, sync = _run(_params(), async_decode=False)
    assert _same(graph_run[1], sync)


def test_engine_plain_sequence_is_unmoved_by_a_penalised_neighbour(graph_run):
    """The plain sequence's tokens in the mixed batch (penalised sampler, state table, logprobs kernel) are its tokens
    without any of that: the same four requests with the new fields left neutral, which run today's graphs.  (Same
    batch shapes on both sides, so its logits come from the same GEMM kernels; only the sampler differs.)"""
    import dataclasses
    neutral = SamplingParams()
    strip = {f: getattr(neutral, f) for f in ("repetition_penalty", "presence_penalty", "frequency_penalty", "min_p",
                                              "logprobs")}
    eng0, alone = _run([dataclasses.replace(p, **strip) for p in _params()])
    assert eng0.pen_state is None and all(len(k) == 4 for k in eng0._graphs)
    assert graph_run[1][3].output == alone[3].output
    assert graph_run[1][2].output == alone[2].output          # (logprobs only: the same tokens too)
    eng, _ = graph_run
    assert eng.bm.num_free == eng.num_kv_blocks and sorted(eng._pen_free) == list(range(4))


def test_engine_full_vocabulary_route_with_penalties():
    eng, seqs = _run(_params(full_vocab=True))
    assert any(g.full_vocab and g.pen == 2 for g in eng._graphs.values())
    _, sync = _run(_params(full_vocab=True), async_decode=False, use_graphs=False)
    assert _same(seqs, sync)
    assert all(len(s.output) == s.params.max_tokens for s in seqs)
    # the greedy penalised row does not depend on its neighbour's route
    _, other = _run(_params())
    assert seqs[0].output == other[0].output


def test_engine_state_row_is_a_recount():
    eng = LLMEngine(TINY, device=DEV, max_num_seqs=4, max_model_len=256, async_decode=False)
    with torch.inference_mode():
        s = eng.add_request(PROMPTS[2], SamplingParams(max_tokens=12, temperature=0.9, seed=4, ignore_eos=True,
                                                       repetition_penalty=1.2, frequency_penalty=0.3))
        while len(s.output) < 7:
            eng.step()
        assert torch.equal(eng.pen_state[s.pen_row].cpu(), sc.recount(s.tokens, s.n_prompt0, TINY.vocab_size))
        while eng.has_work():
            eng.step()
