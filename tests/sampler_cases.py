"""Shared inputs and the fp64 oracle for the sampler tests (penalties, min_p, logprobs).

Plain helper functions for tests/test_sampler_penalties_{cpu,gpu}.py (no fixtures, no pytest settings).  The rule under
test is ``shai_amd.ops.reference`` (``penalize_logits`` / ``sample_candidates`` / ``token_logprobs``); here it runs with
fp64 probabilities and is the expectation for the fp32 oracle, the CPU engine and the kernels.

Exact cases: token EQUALITY is demanded, so nothing may depend on rounding.
  * Logits are integers in [-8, 8] (exact in bf16), penalties are dyadic (r in {2, 0.5}, f in {0.5, -0.25}, p = 0.25)
    and counts are small, so every penalised logit is exact in fp32 whatever the compiler contracts: both sides sort
    the same values, the candidate order (descending value, ascending index) is identical.
  * For sampled rows the generator draws T, top_p, min_p and the uniform, and keeps them only if every decision has
    a margin in fp64: each |p_i - min_p| >= MARGIN (p_0 = 1), each |mass before i - top_p * total| >= MARGIN * total,
    each |cdf_i - u * kept mass| >= MARGIN * total.  fp32 sums of <= 1024 positive terms and the hardware exp are
    good to ~1e-5 relative, a hundred times below MARGIN.
  * A batch is sampled ``CALLS`` times in a row; the state moves between calls (the sampler counts what it picks), so
    calls 2 and 3 see penalties that call 1 caused.

Rows of an exact batch (state row = batch row + 1; state rows 0 and B + 1, and the rows of batch rows without state,
are canaries that nothing may touch):
  0 plain    sampled, no state row (its r / f / p are set and must be ignored)
  1 count    greedy, crafted: a token with count 3 beats a prompt-only token by 0.25, and loses to it once counted again
  2 minp     sampled, penalised, min_p > 0, top_k 50; logits are a ladder 8..3 over a bulk <= 0, min_p drops some
  3 tie      greedy, crafted: the penalty takes the arg-max (a prompt-only 8) below a tied pair of 5s; lowest index wins
  4 k1024    sampled, penalised, top_k 1024 (= every entry when V < 1024), r = 0.5, f = -0.25; 24 entries above a bulk
  5 negative sampled, penalised, all logits negative
  6 minponly sampled, min_p > 0, no state row; the same ladder
"""
import functools
from types import SimpleNamespace

import torch

from shai_amd.ops import reference as ref

MARGIN = 1e-3
CALLS = 3
VOCABS = (1000, 32003, 128256)
ROWS = ("plain", "count", "minp", "tie", "k1024", "negative", "minponly")
FLAG, CMASK = ref.PENALTY_PROMPT_FLAG, ref.PENALTY_COUNT_MASK


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _words(g, V):
    """Random state words: ~10 % of the entries sampled 1..3 times, ~5 % flagged as prompt tokens."""
    c = torch.randint(1, 4, (V,), generator=g) * (torch.rand(V, generator=g) < 0.10)
    f = (torch.rand(V, generator=g) < 0.05).long() * FLAG
    return (c + f).to(torch.int32)


def margins(l, T, top_k, top_p, min_p, u):
    """Smallest margin (in the units above) of the min_p cut, the nucleus cut and the draw for one fp32 row ``l`` of
    penalised logits, in fp64; and the kept length."""
    V = l.numel()
    vals, _ = torch.sort(l, descending=True, stable=True)
    K = V if top_k <= 0 or top_k > V else top_k
    p = torch.exp((vals[:K] - vals[0]).double() / T)
    m = float("inf")
    if min_p > 0:
        m = min(m, float((p - min_p).abs().min()))
    keep = (p >= min_p)
    keep[0] = True
    p = p * keep
    cum = p.cumsum(0)
    total = float(cum[-1])
    before = (cum - p)[keep]
    m = min(m, float((before - top_p * total).abs().min()) / total)
    L = max(1, int((before <= top_p * total).sum()))
    target = u * float(cum[L - 1])
    m_draw = float((cum[:L] - target).abs().min()) / total
    return min(m, m_draw), m, L


def _craft(kind, g, V):
    """(logits fp32 [V], state words int32 [V]) of one row."""
    lo, hi = {"count": (-8, 1), "tie": (-8, 4), "negative": (-8, -1), "k1024": (-8, 0)}.get(kind, (-8, 8))
    l = torch.randint(lo, hi + 1, (V,), generator=g).float()
    w = _words(g, V)
    pick = torch.randperm(V, generator=g)[:3].sort().values.tolist()
    if kind == "k1024":      # 1024 equal candidates would leave no margin for the draw (steps of 1 / 1024 of the
        top = torch.randperm(V, generator=g)[:24]     # mass): a bulk <= 0 under 24 entries at 1..8, some of them seen
        l[top] = torch.arange(24).float() // 3 + 1
    if kind in ("minp", "minponly"):   # a ladder whose lower rungs hold real mass, so that where min_p cuts matters
        lad = torch.tensor([8] * 2 + [7] * 3 + [6] * 4 + [5] * 10 + [4] * 20 + [3] * 11).float()
        l.clamp_(max=0)
        l[torch.randperm(V, generator=g)[:lad.numel()]] = lad
    if kind == "count":      # r 2, f 0.5, p 0.25: x = 8 / 2 - 1.5 - 0.25 = 2.25 > y = 4 / 2 = 2 > the rest (<= 1)
        x, y = pick[1], pick[0]
        l[x], w[x] = 8.0, 3
        l[y], w[y] = 4.0, FLAG
    if kind == "tie":        # r 2: a = 8 / 2 = 4 < the unseen pair at 5; everything else <= 4
        i, j, a = pick
        l[a], w[a] = 8.0, FLAG
        l[i], w[i] = 5.0, 0
        l[j], w[j] = 5.0, 0
    return l, w


PEN = {"plain": (2.0, 0.5, 0.25), "count": (2.0, 0.5, 0.25), "minp": (2.0, 0.5, 0.25), "tie": (2.0, 0.0, 0.0),
       "k1024": (0.5, -0.25, 0.25), "negative": (2.0, 0.5, 0.0), "minponly": (1.0, 0.0, 0.0)}
TOPK = {"plain": 50, "count": 50, "minp": 50, "tie": 7, "k1024": 1024, "negative": 40, "minponly": 64}
STATELESS = ("plain", "minponly")


@functools.lru_cache(maxsize=None)
def exact_batch(V, seed=0):
    """One exact batch at vocabulary size V: inputs of CALLS consecutive sampler calls and the expected tokens and
    states.  Tensors are on the CPU (logits fp32, integer-valued); never modified by the tests."""
    g = _gen(1000 * seed + V)
    B = len(ROWS)
    logits = torch.empty(B, V)
    state0 = torch.empty(B + 2, V, dtype=torch.int32)
    state0[0], state0[B + 1] = _words(g, V), _words(g, V)
    for b, kind in enumerate(ROWS):
        logits[b], state0[b + 1] = _craft(kind, g, V)
    rows = torch.tensor([-1 if k in STATELESS else b + 1 for b, k in enumerate(ROWS)], dtype=torch.int32)
    rep, freq, pres = (torch.tensor([PEN[k][i] for k in ROWS]) for i in range(3))
    top_k = torch.tensor([TOPK[k] for k in ROWS], dtype=torch.int32)
    temps, top_p, min_p, u = (torch.zeros(CALLS, B) for _ in range(4))
    tokens = torch.zeros(CALLS, B, dtype=torch.int64)
    states = [state0]
    for c in range(CALLS):
        st = states[-1].clone()
        lpen = ref.penalize_logits(logits, ref.penalty_words(st, rows, B, V, "cpu"), rep, freq, pres)
        for b, kind in enumerate(ROWS):
            if kind in ("count", "tie"):     # greedy
                top_p[c, b] = 1.0
                continue
            for _ in range(400):
                T = float(torch.randint(4, 13, (1,), generator=g)) / 8            # 0.5 .. 1.5
                tp = float(torch.randint(50, 100, (1,), generator=g)) / 100
                mp = float(torch.randint(1, 30, (1,), generator=g)) / 100 if kind in ("minp", "minponly") else 0.0
                uu = float(torch.rand(1, generator=g))
                if margins(lpen[b], T, int(top_k[b]), tp, mp, uu)[0] >= MARGIN and (
                        mp == 0 or float(torch.exp((lpen[b].topk(int(top_k[b])).values.min() - lpen[b].max()) / T))
                        < mp):                                   # (min_p rows: min_p drops something)
                    break
            else:
                raise AssertionError(f"no parameters with a margin for row {kind} at V={V}")
            temps[c, b], top_p[c, b], min_p[c, b], u[c, b] = T, tp, mp, uu
        # fp32 copies of the parameters are what every implementation receives: decide the expectation on them
        tokens[c] = ref.sample_candidates(lpen, temps[c], top_k.long(), top_p[c], min_p[c], u[c], dtype=torch.float64)
        for b in range(B):
            if temps[c, b] > 0:
                assert margins(lpen[b], float(temps[c, b]), int(top_k[b]), float(top_p[c, b]), float(min_p[c, b]),
                               float(u[c, b]))[0] >= MARGIN / 2, (V, c, ROWS[b])
        ref.penalty_state_add(st, rows, tokens[c])
        states.append(st)
    return SimpleNamespace(V=V, B=B, logits=logits, rows=rows, rep=rep, freq=freq, pres=pres, top_k=top_k,
                           temps=temps, top_p=top_p, min_p=min_p, u=u, tokens=tokens, states=states)


def run_calls(case, penalize=ref.penalize_logits, candidates=ref.sample_candidates, update=True,
              dtype=torch.float32):
    """The CALLS consecutive calls of an exact batch through the oracle's pieces (or a mutant of one) on the CPU:
    (tokens [CALLS, B], final state)."""
    st = case.states[0].clone()
    out = []
    for c in range(CALLS):
        lpen = penalize(case.logits, ref.penalty_words(st, case.rows, case.B, case.V, "cpu"), case.rep, case.freq,
                        case.pres)
        toks = candidates(lpen, case.temps[c], case.top_k.long(), case.top_p[c], case.min_p[c], case.u[c],
                          dtype=dtype)
        if update:
            ref.penalty_state_add(st, case.rows, toks)
        out.append(toks)
    return torch.stack(out), st


# ---- mutants of the rule: each must give a token that differs from the exact cases' expectation
def mutant_output_only(logits, words, rep, freq, pres):
    """Repetition penalty on sampled tokens only (prompt tokens forgotten)."""
    return ref.penalize_logits(logits, words & CMASK, rep, freq, pres)


def mutant_mul_positive(logits, words, rep, freq, pres):
    """l * r whatever the sign of l."""
    l = logits.float()
    c = words & CMASK
    l = torch.where(words != 0, l * rep[:, None], l) - freq[:, None] * c.float()
    return torch.where(c > 0, l - pres[:, None], l)


def mutant_presence_by_count(logits, words, rep, freq, pres):
    """Presence penalty times the count."""
    c = (words & CMASK).float()
    return ref.penalize_logits(logits, words, rep, freq, torch.zeros_like(pres)) - pres[:, None] * c


def mutant_minp_after_nucleus(l, temps, top_k, top_p, min_p, uniforms, dtype=torch.float32):
    """The nucleus cut over all top-k candidates first, min_p on what it kept."""
    B, V = l.shape
    vals, idx = torch.sort(l, dim=-1, descending=True, stable=True)
    ar = torch.arange(V)[None, :]
    k = torch.where((top_k <= 0) | (top_k > V), torch.full_like(top_k, V), top_k)[:, None]
    greedy = temps <= 0
    T = torch.where(greedy, torch.ones_like(temps), temps).to(dtype)[:, None]
    p0 = torch.exp((vals - vals[:, :1]).to(dtype) / T) * (ar < k)
    cum0 = p0.cumsum(-1)
    keep = (ar < k) & ((cum0 - p0) <= top_p.to(dtype)[:, None] * cum0[:, -1:])
    keep = keep & ((p0 >= min_p.to(dtype)[:, None]) | (ar == 0))
    p = p0 * keep
    cum = p.cumsum(-1)
    L = keep.sum(-1).clamp(min=1)
    target = uniforms.to(dtype) * cum.gather(-1, (L - 1)[:, None]).squeeze(-1)
    pick = ((cum <= target[:, None]) & (ar < (L - 1)[:, None])).sum(-1)
    pick = torch.where(greedy, torch.zeros_like(pick), pick)
    return idx.gather(-1, pick[:, None]).squeeze(-1)


# ---- general values: membership only
@functools.lru_cache(maxsize=None)
def general_case(V=32003, n_base=4, n_u=50, seed=7):
    """Random bf16 logits with non-dyadic penalties: n_base (logits, state) rows, each drawn at n_u uniforms (B =
    n_base * n_u rows, every one with a state row of its own).  ``kept`` [n_base, V]: the tokens the fp64 oracle can
    draw.  The penalised fp32 logits are the same bits on both sides (IEEE division, no contraction), so the
    candidate order is; the min_p and nucleus cuts are kept only with the exact cases' margin, so the kept set is."""
    g = _gen(seed)
    rep = torch.tensor([1.3, 1.1, 0.8, 1.7][:n_base])
    freq = torch.tensor([0.3, -0.2, 0.15, 0.7][:n_base])
    pres = torch.tensor([0.2, 0.6, -0.3, 0.1][:n_base])
    top_k = torch.tensor([50, 1024, 200, 8][:n_base], dtype=torch.int32)
    while True:
        logits = (torch.randn(n_base, V, generator=g) * 3).to(torch.bfloat16)
        words = torch.stack([_words(g, V) for _ in range(n_base)])
        temps = torch.randint(5, 12, (n_base,), generator=g).float() / 8
        top_p = torch.randint(60, 99, (n_base,), generator=g).float() / 100
        min_p = torch.randint(1, 10, (n_base,), generator=g).float() / 100
        lpen = ref.penalize_logits(logits, words, rep, freq, pres)
        if all(margins(lpen[b], float(temps[b]), int(top_k[b]), float(top_p[b]), float(min_p[b]), 0.5)[1] >= MARGIN
               for b in range(n_base)):
            break
    u = torch.rand(n_base * n_u, generator=g)
    _, kept = ref.sample_candidates(lpen, temps, top_k.long(), top_p, min_p, torch.zeros(n_base),
                                    dtype=torch.float64, return_kept=True)
    base = torch.arange(n_base).repeat_interleave(n_u)
    return SimpleNamespace(V=V, B=n_base * n_u, base=base, logits=logits, words=words, rep=rep, freq=freq, pres=pres,
                           top_k=top_k, temps=temps, top_p=top_p, min_p=min_p, u=u, kept=kept)


# ---- logprobs
@functools.lru_cache(maxsize=None)
def logprob_case(V, seed=3):
    """Random logits [4, V] (bf16-representable fp32, so bf16 and fp32 inputs hold the same values), picked tokens,
    per-row counts (5, 0, skip, 3) and the fp64 expectation for N = 5."""
    g = _gen(seed * 7919 + V)
    logits = (torch.randn(4, V, generator=g) * 4).to(torch.bfloat16).float()
    tokens = torch.randint(0, V, (4,), generator=g).to(torch.int32)
    row_n = torch.tensor([5, 0, -1, 3], dtype=torch.int32)
    vals, ids = ref.token_logprobs(logits, tokens, 5, row_n, dtype=torch.float64)
    return SimpleNamespace(V=V, N=5, logits=logits, tokens=tokens, row_n=row_n, vals=vals, ids=ids)


def recount(tokens, n_prompt, V):
    """Host recount of a state row from a token list: prompt flags for the first n_prompt, counts for the rest."""
    w = torch.zeros(V, dtype=torch.int32)
    for t in tokens[n_prompt:]:
        if 0 <= t < V:
            w[t] += 1
    for t in tokens[:n_prompt]:
        if 0 <= t < V:
            w[t] |= FLAG
    return w
