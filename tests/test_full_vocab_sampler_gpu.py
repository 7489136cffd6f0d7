"""The full-vocabulary sampler launches (top_k none or above 1024) against the fp64 oracle on the CPU."""
import dataclasses
from types import SimpleNamespace

import pytest
import torch

import full_vocab_cases as fc
import sampler_cases as sc
from shai_amd import ops
from shai_amd.engines.llm import LLMEngine, SamplingParams
from shai_amd.models.llama import LlamaConfig
from shai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
d = lambda t: None if t is None else t.to(DEV).contiguous()


def _sample(kind, logits, temps, top_k, top_p, u, a=None, state=None, cstate=None, min_p=None, full_vocab=True):
    """One launch of the plain / pen / con sampler on the GPU; ``a``: the case with the penalty / constraint inputs."""
    out = torch.full((logits.shape[0],), -7, dtype=torch.int32, device=DEV)
    if kind == "plain":
        return ops.sample(logits, d(temps), d(top_k), d(top_p), d(u), out, full_vocab=full_vocab)
    pen = (state, d(a.rows), d(a.rep), d(a.freq), d(a.pres), d(min_p))
    if kind == "pen":
        return ops.sample_penalized(logits, d(temps), d(top_k), d(top_p), d(u), out, *pen, full_vocab=full_vocab)
    return ops.sample_constrained(logits, d(temps), d(top_k), d(top_p), d(u), out, *pen, d(a.pool), cstate,
                                  d(a.prog), d(a.slot), d(a.ban), full_vocab=full_vocab)


FLAT_V = 4096
FLAT = {"none": (0, 4096, 1), "k3000": (3000, 3000, 1), "mask": (0, 1366, 3)}   # top_k, tokens kept, index stride


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("mode", list(FLAT))
def test_flat_row_is_exact(mode, dt):
    """Equal logits, T = 1, top_p = 1: n kept tokens of equal weight, u = (j + 0.5) / n picks the j-th of them in
    index order.  Nothing rounds: the weights are 2^40 each.  (A 1024-candidate buffer fails every j >= 1024.)"""
    top_k, n, stride = FLAT[mode]
    js, B = torch.tensor([0, 1023, 1024, 1025, n - 1]), 5
    logits = torch.full((B, FLAT_V), 2.0)
    a = SimpleNamespace(rows=torch.full((B,), -1, dtype=torch.int32), rep=torch.ones(B), freq=torch.zeros(B),
                        pres=torch.zeros(B), pool=fc.every_third(FLAT_V), prog=torch.zeros(B, dtype=torch.int32),
                        slot=torch.arange(B, dtype=torch.int32), ban=torch.zeros(B, dtype=torch.int32))
    args = (torch.ones(B), torch.full((B,), top_k, dtype=torch.int32), torch.ones(B), (js + 0.5) / n)
    cstate = torch.zeros(B, dtype=torch.int32)
    want = ref.sample_constrained(logits, *args, None, a.rows, a.rep, a.freq, a.pres, torch.zeros(B),
                                  a.pool if mode == "mask" else None, cstate, a.prog, a.slot, a.ban,
                                  dtype=torch.float64)
    assert want.tolist() == (js * stride).tolist()
    got = _sample("con" if mode == "mask" else "plain", logits.to(DEV, DTYPES[dt]), *args, a, None, d(cstate),
                  torch.zeros(B))
    assert got.cpu().tolist() == want.tolist()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("V,kind", [(1025, "plain"), (4099, "plain"), (32003, "plain"), (128256, "plain"),
                                    (4099, "pen"), (4099, "con")])
def test_head_resolved_rows_are_exact(V, kind, dt):
    """The fp64 oracle's tokens over CALLS calls for top_k 0 / -1 / V / 1025; the state counts them, canaries stay."""
    a = fc.ladder_case(V, kind)
    logits, state, cstate = a.logits.to(DEV, DTYPES[dt]), d(a.states[0]), d(a.cstate)
    toks = torch.stack([_sample(kind, logits, a.temps[c], a.top_k, a.top_p[c], a.u[c], a, state, cstate, a.min_p[c])
                        for c in range(sc.CALLS)]).cpu()
    assert torch.equal(toks.long(), a.tokens), (toks.tolist(), a.tokens.tolist())
    if kind != "plain":
        assert torch.equal(state.cpu(), a.states[-1]) and torch.equal(state[0].cpu(), a.states[0][0])


def _bulk(a):
    z, none = torch.zeros(a.B), torch.full((a.B,), -1, dtype=torch.int32)
    pen = SimpleNamespace(rows=none, rep=z + 1, freq=z, pres=z, pool=a.pool, prog=none + 1,
                          slot=torch.arange(a.B, dtype=torch.int32), ban=none + 1)
    return _sample("con", a.logits.to(DEV), z + 1, none + 1, a.top_p, a.u, pen, None,
                   torch.zeros(a.B, dtype=torch.int32, device=DEV), z + 0.1).cpu().long()


def test_bulk_draw_is_within_the_fp64_interval_and_repeats():
    """Kept sets far above 1024: the token's fp64 CDF interval, widened by d = 1e-4 of the total, holds u * kept (the
    exponent's argument is <= 32, the fp32 product with 1 / T and the hardware exp are a few 1e-6 relative per term,
    integer sums add nothing: tenfold that).  Masked and below-min_p tokens have an empty interval.  Runs repeat."""
    a = fc.bulk_case()
    t = _bulk(a)
    print("tokens", t.tolist(), "slack", ((a.target - a.lo[t]) / a.total).tolist())
    assert bool(((a.lo[t] - 1e-4 * a.total <= a.target) & (a.target <= a.hi[t] + 1e-4 * a.total)).all())
    assert torch.equal(_bulk(a), t)


@pytest.mark.parametrize("kind", ["plain", "pen"])
def test_top_k_rows_do_not_depend_on_full_vocabulary_neighbours(kind):
    """Rows with top_k 50 and 1024, and a greedy row, in a full-vocabulary launch: the candidate-buffer launch's
    tokens on the same inputs."""
    a = fc.ladder_case(4099, kind)
    logits = a.logits.to(DEV, torch.bfloat16)
    temps = a.temps[0] * torch.tensor([1.0, 0.0, 1.0, 1.0])
    full, alone = (_sample(kind, logits, temps, torch.tensor(top_k, dtype=torch.int32), a.top_p[0], a.u[0], a,
                           d(a.states[0]), None, a.min_p[0], full_vocab=fv).cpu()
                   for top_k, fv in (([50, 0, 1024, -1], True), ([50, 7, 1024, 9], False)))
    assert torch.equal(full[:3], alone[:3])


def _engine(cfg, **kw):
    eng = LLMEngine(cfg, device=DEV, max_num_seqs=4, max_model_len=256, **kw)
    params = [SamplingParams(max_tokens=10, temperature=0.9, top_k=0, top_p=0.9, seed=3, ignore_eos=True),
              SamplingParams(max_tokens=8, temperature=0.8, top_k=0, seed=11, frequency_penalty=0.5, min_p=0.001,
                             ignore_eos=True),
              SamplingParams(max_tokens=9, temperature=0.7, top_k=50, seed=5, ignore_eos=True)]
    with torch.inference_mode():
        seqs = [eng.add_request(p, q) for p, q in zip([[3, 17, 99, 250, 7], [5, 6, 7], [9, 9, 41]], params)]
        while eng.has_work():
            eng.step()
    return eng, [s.output for s in seqs]


def test_engine_samples_full_vocabulary_rows_inside_the_graph(monkeypatch):
    cfg = dataclasses.replace(LlamaConfig.tiny(), vocab_size=2048)
    eng, out = _engine(cfg)
    assert any(g.graph is not None and g.full_vocab and not g.after_replay for g in eng._graphs.values())
    assert out == _engine(cfg, async_decode=False, use_graphs=False)[1] and [len(o) for o in out] == [10, 8, 9]
    monkeypatch.setenv("SHAI_FULL_VOCAB_SAMPLER", "0")
    eng0, out0 = _engine(cfg)
    assert all(g.after_replay for g in eng0._graphs.values() if g.full_vocab) and [len(o) for o in out0] == [10, 8, 9]
