"""Shared inputs and the fp64 expectation for the constrained-sampling tests (token masks, logit_bias, min_tokens,
guided choice).

Plain helper functions for tests/test_constrained_sampling_{cpu,gpu}.py (no fixtures, no pytest settings).  The rule
under test is ``shai_amd.ops.reference`` (``constrain_logits`` / ``sample_candidates`` / ``con_next``); here it runs
with fp64 probabilities and is the expectation for the fp32 oracle, the CPU engine and the kernel.

Exact cases: token EQUALITY is demanded, so nothing may depend on rounding (see tests/sampler_cases.py for the
argument).  Logits are integers in [-8, 8], biases are dyadic (+-0.5, +-2, -100), penalties are dyadic, and for the
sampled rows T, top_p and the uniform are drawn until every decision keeps ``MARGIN`` -- the margins are taken over
the FINITE candidates only (the masked ones are cut before anything is decided).  A batch is sampled ``CALLS`` times
in a row: the automaton states (and the penalty counts) move between the calls.

Programs come from the compiler (``engines.constraints.compile_program``) and lie back to back in a pool behind a junk
prefix; row b's state word is ``cstate[2 * b + 1]``, the even words and the words of rows without a program are
canaries.  Rows (EOS = 2, a second stop token STOP2):
  0 plain      sampled, no program: program offset -1, and junk in its slot / ban_stop fields
  1 allowed3   allowed_token_ids of 3 tokens under top_k 50, top_p 1, the largest uniform 1 - 2^-24: the pick is allowed
  2 greedymask greedy; the raw arg-max, token V - 1 (in the partial last mask word when V % 32 != 0), is a bad word
  3 biaspen    greedy, repetition penalty 2: +2 lifts x (6) over the arg-max y (7), the penalty then halves it to 4,
               below z (4 + 0.5 bias, unseen); with the bias after the penalty x would be 6 / 2 + 2 = 5 and win
  4 banstop    greedy, the arg-max is EOS, min_tokens 2: banned in calls 1 and 2, picked in call 3
  5 badword    greedy, bad word [a, b], frequency penalty 2: call 1 picks a (8); in call 2 a is 5.75 and the arg-max b
               (7) is banned behind a, so c (6) wins and the state returns to the root; call 3 picks b
  6 guided     sampled, guided_choice [[g1, g2], [h1]]: walked g1, g2, then only the stop set is left
  7 u1         as allowed3 at the closed end u = 1.0: the draw lands on the last candidate, which must be the last
               FINITE one -- with the -inf tail kept it is a masked token.  (For u < 1 the product u * total never
               reaches the total in fp32 or fp64, so this is the one uniform at which keeping the tail shows.)
"""
import functools
from types import SimpleNamespace

import torch

import sampler_cases as sc
from shai_amd.engines import constraints as cn
from shai_amd.ops import reference as ref

MARGIN = sc.MARGIN
CALLS = 3
VOCABS = (1000, 32003, 128256)
ROWS = ("plain", "allowed3", "greedymask", "biaspen", "banstop", "badword", "guided", "u1")
EOS = 2
SAMPLED = ("plain", "guided")
U_MAX = 1.0 - 2.0 ** -24
PEN_ROW = {"biaspen": 1, "badword": 2}          # rows of the penalty-state table (0 and 3 are canaries)
PEN = {"biaspen": (2.0, 0.0, 0.0), "badword": (1.0, 2.0, 0.25)}
JUNK = 5                                         # junk words in front of the first program


def params_of(**kw):
    """Just the fields the compiler reads."""
    d = dict(logit_bias=None, allowed_token_ids=None, bad_words_ids=None, min_tokens=0, guided_choice=None,
             ignore_eos=False, max_tokens=16, stop_token_ids=None)
    d.update(kw)
    return SimpleNamespace(**d)


def finite_margins(l, T, top_k, top_p, min_p, u):
    """``sampler_cases.margins`` over the finite candidates of one constrained row: the top-k cut counts the masked
    entries (they are candidates until the finite cut), the decisions are made among the finite ones."""
    V = l.numel()
    K = V if top_k <= 0 or top_k > V else top_k
    vals = torch.sort(l, descending=True, stable=True).values[:K]
    vals = vals[torch.isfinite(vals)]
    return sc.margins(vals, T, 0, top_p, min_p, u)


def _special(g, V, n):
    """n distinct token ids, none of them EOS, V - 1 or below 3."""
    while True:
        ids = (torch.randperm(V - 4, generator=g)[:n] + 3).tolist()
        if EOS not in ids and V - 1 not in ids:
            return ids


@functools.lru_cache(maxsize=None)
def exact_batch(V, seed=0):
    g = sc._gen(7000 * seed + V)
    B = len(ROWS)
    ids = _special(g, V, 16)
    stop2, (a3, b3, c3), (x, y, z, n1, n2, n3), (wa, wb, wc), (g1, g2, h1) = ids[0], ids[1:4], ids[4:10], ids[10:13], \
        ids[13:16]
    stop = [EOS, stop2]
    logits = torch.randint(-8, 9, (B, V), generator=g).float()
    pstate0 = torch.stack([sc._words(g, V) for _ in range(4)])
    progs = {}
    # 1 / 7: three allowed tokens at 3, 2, 1 under a bulk that holds many 8s (the raw top 50 has none of them)
    for r in (1, 7):
        logits[r, torch.tensor([a3, b3, c3])] = torch.tensor([3.0, 2.0, 1.0])
        progs[r] = params_of(allowed_token_ids=[c3, a3, b3])
    # 2: the arg-max is token V - 1 and it is banned
    logits[2].clamp_(max=7)
    logits[2, V - 1] = 8.0
    progs[2] = params_of(bad_words_ids=[[V - 1]])
    # 3: bias before the penalty
    logits[3].clamp_(max=3)
    logits[3, torch.tensor([x, y, z])] = torch.tensor([6.0, 7.0, 4.0])
    pstate0[1, torch.tensor([x, y])] = sc.FLAG
    pstate0[1, z] = 0
    progs[3] = params_of(logit_bias={x: 2.0, z: 0.5, n1: -100.0, n2: -0.5, n3: -2.0})
    # 4: the arg-max is EOS, banned while fewer than 2 tokens were generated
    logits[4].clamp_(max=7)
    logits[4, EOS] = 8.0
    progs[4] = params_of(min_tokens=2, stop_token_ids=[stop2])
    # 5: a two-token bad word
    logits[5].clamp_(max=5)
    logits[5, torch.tensor([wa, wb, wc])] = torch.tensor([8.0, 7.0, 6.0])
    pstate0[2, torch.tensor([wa, wb, wc])] = 0
    progs[5] = params_of(bad_words_ids=[[wa, wb], [wb, wc, wa]])
    # 6: guided choice
    logits[6, torch.tensor([g1, g2, h1])] = torch.tensor([5.0, -3.0, 4.0])
    logits[6, torch.tensor(stop)] = torch.tensor([1.0, 2.0])
    progs[6] = params_of(guided_choice=[[g1, g2], [h1]], stop_token_ids=[stop2])
    compiled = {r: cn.compile_program(p, stop, V) for r, p in progs.items()}
    blocks, offs, at = [torch.full((JUNK,), -12345, dtype=torch.int32)], {}, JUNK
    for r in sorted(compiled):
        if r == 7:                       # rows 1 and 7 share a program
            offs[7] = offs[1]
            continue
        offs[r] = at
        blocks.append(compiled[r].words)
        at += compiled[r].words.numel()
    blocks.append(torch.full((3,), -777, dtype=torch.int32))
    pool = torch.cat(blocks)
    prog = torch.tensor([offs.get(b, -1) for b in range(B)], dtype=torch.int32)
    slot = torch.tensor([2 * b + 1 for b in range(B)], dtype=torch.int32)
    cstate0 = torch.tensor([900 + i if i % 2 == 0 else 0 for i in range(2 * B + 1)], dtype=torch.int32)
    cstate0[1] = 999                                             # row 0: no program, its word is a canary too
    min_tokens = torch.tensor([progs[b].min_tokens if b in progs else 0 for b in range(B)])
    min_tokens[0] = 5                                            # junk: the plain row has no program to ban with
    rows = torch.tensor([PEN_ROW.get(k, -1) for k in ROWS], dtype=torch.int32)
    rep, freq, pres = (torch.tensor([PEN.get(k, (2.0, 0.5, 0.25))[i] for k in ROWS]) for i in range(3))
    top_k = torch.tensor([50] * B, dtype=torch.int32)
    temps, top_p, u = torch.zeros(CALLS, B), torch.ones(CALLS, B), torch.zeros(CALLS, B)
    min_p = torch.zeros(CALLS, B)
    for r, uu in ((1, U_MAX), (7, 1.0)):
        temps[:, r], u[:, r] = 1.0, uu
    tokens = torch.zeros(CALLS, B, dtype=torch.int64)
    bans = torch.zeros(CALLS, B, dtype=torch.int32)
    pstates, cstates = [pstate0], [cstate0]
    for c in range(CALLS):
        pst, cst = pstates[-1].clone(), cstates[-1].clone()
        bans[c] = ref.ban_stop(torch.full((B,), c), min_tokens).to(torch.int32)
        crows = ref.con_rows(pool, cst, prog, slot, V)
        l = ref.constrain_logits(logits, ref.penalty_words(pst, rows, B, V, "cpu"), rep, freq, pres, crows, bans[c])
        for b, kind in enumerate(ROWS):
            if kind not in SAMPLED:
                continue
            for _ in range(800):
                T = float(torch.randint(4, 13, (1,), generator=g)) / 8
                tp = float(torch.randint(50, 100, (1,), generator=g)) / 100
                uu = float(torch.rand(1, generator=g))
                if finite_margins(l[b], T, 50, tp, 0.0, uu)[0] < MARGIN:
                    continue
                if kind == "guided" and c == 0:      # the walk starts down the two-token choice
                    t1 = ref.sample_candidates(l[b:b + 1], torch.tensor([T]), top_k[b:b + 1].long(),
                                               torch.tensor([tp]), torch.zeros(1), torch.tensor([uu]),
                                               dtype=torch.float64)
                    if int(t1) != g1:
                        continue
                break
            else:
                raise AssertionError(f"no parameters with a margin for row {kind} at V={V}")
            temps[c, b], top_p[c, b], u[c, b] = T, tp, uu
        tokens[c] = ref.sample_candidates(l, temps[c], top_k.long(), top_p[c], min_p[c], u[c], dtype=torch.float64)
        for b, kind in enumerate(ROWS):
            if kind in SAMPLED:
                assert finite_margins(l[b], float(temps[c, b]), 50, float(top_p[c, b]), 0.0,
                                      float(u[c, b]))[0] >= MARGIN / 2, (V, c, kind)
        ref.penalty_state_add(pst, rows, tokens[c])
        ref.con_advance(cst, crows, tokens[c])
        pstates.append(pst)
        cstates.append(cst)
    named = SimpleNamespace(stop=stop, allowed3=(a3, b3, c3), x=x, y=y, z=z, wa=wa, wb=wb, wc=wc, g1=g1, g2=g2, h1=h1)
    return SimpleNamespace(V=V, B=B, logits=logits, rows=rows, rep=rep, freq=freq, pres=pres, top_k=top_k, temps=temps,
                           top_p=top_p, min_p=min_p, u=u, tokens=tokens, pstates=pstates, cstates=cstates, pool=pool,
                           prog=prog, slot=slot, bans=bans, min_tokens=min_tokens, compiled=compiled, ids=named)


def run_calls(case, candidates=ref.sample_candidates, advance=True, ban_rule=ref.ban_stop, topk_first=False,
              dtype=torch.float32, **constrain_kw):
    """The CALLS consecutive calls of an exact batch through the oracle's pieces (or mutants of them) on the CPU:
    (tokens [CALLS, B], final penalty state, final automaton states)."""
    pst, cst = case.pstates[0].clone(), case.cstates[0].clone()
    out = []
    for c in range(CALLS):
        ban = ban_rule(torch.full((case.B,), c), case.min_tokens).to(torch.int32)
        crows = ref.con_rows(case.pool, cst, case.prog, case.slot, case.V)
        words = ref.penalty_words(pst, case.rows, case.B, case.V, "cpu")
        l = ref.constrain_logits(case.logits, words, case.rep, case.freq, case.pres, crows, ban, **constrain_kw)
        if topk_first:      # mutant: the top-k cut on the unmasked values, the mask on what it kept
            free = ref.constrain_logits(case.logits, words, case.rep, case.freq, case.pres,
                                        [None if r is None else (_unmasked(r[0]), r[1], r[2]) for r in crows], ban)
            idx = torch.sort(free, dim=-1, descending=True, stable=True).indices[:, :50]
            top = torch.zeros_like(free, dtype=torch.bool).scatter_(1, idx, True)
            l = torch.where(top, l, torch.full_like(l, float("-inf")))
        toks = candidates(l, case.temps[c], case.top_k.long(), case.top_p[c], case.min_p[c], case.u[c], dtype=dtype)
        ref.penalty_state_add(pst, case.rows, toks)
        if advance:
            ref.con_advance(cst, crows, toks)
        out.append(toks)
    return torch.stack(out), pst, cst


def _unmasked(pv):
    """A program view with every token allowed in every state (bias kept)."""
    import copy
    q = copy.copy(pv)
    q.masks = torch.full_like(pv.masks, -1)
    q.stop = torch.zeros_like(pv.stop)
    return q


def mutant_tail_kept(l, temps, top_k, top_p, min_p, uniforms, dtype=torch.float32):
    """``ref.sample_candidates`` without the finite cut: the -inf candidates stay as a zero-mass tail."""
    B, V = l.shape
    vals, idx = torch.sort(l, dim=-1, descending=True, stable=True)
    ar = torch.arange(V)[None, :]
    k = torch.where((top_k <= 0) | (top_k > V), torch.full_like(top_k, V), top_k)[:, None]
    greedy = temps <= 0
    T = torch.where(greedy, torch.ones_like(temps), temps).to(dtype)[:, None]
    p = torch.exp((vals - vals[:, :1]).to(dtype) / T)
    keep = (ar < k) & ((p >= min_p.to(dtype)[:, None]) | (ar == 0))
    p = p * keep
    cum = p.cumsum(-1)
    keep = keep & ((cum - p) <= top_p.to(dtype)[:, None] * cum[:, -1:])
    L = keep.sum(-1).clamp(min=1)
    target = uniforms.to(dtype) * cum.gather(-1, (L - 1)[:, None]).squeeze(-1)
    pick = ((cum <= target[:, None]) & (ar < (L - 1)[:, None])).sum(-1)
    pick = torch.where(greedy, torch.zeros_like(pick), pick)
    return idx.gather(-1, pick[:, None]).squeeze(-1)


# ---- general values: membership only
@functools.lru_cache(maxsize=None)
def general_case(V=32003, n_base=4, n_u=50, seed=11):
    """Random bf16 logits, non-dyadic penalties and biases, a random allow-mask per base row: n_base (logits, state,
    program) rows, each drawn at n_u uniforms.  ``kept`` [n_base, V]: the tokens the fp64 oracle can draw;
    ``allowed`` [n_base, V].  The constrained fp32 logits are the same bits on both sides (one fp32 add, IEEE
    division, no contraction), so the candidate order is; the cuts keep the exact cases' margin."""
    g = sc._gen(seed)
    rep = torch.tensor([1.3, 1.1, 0.8, 1.7][:n_base])
    freq = torch.tensor([0.3, -0.2, 0.15, 0.7][:n_base])
    pres = torch.tensor([0.2, 0.6, -0.3, 0.1][:n_base])
    top_k = torch.tensor([50, 1024, 200, 8][:n_base], dtype=torch.int32)
    frac = [0.5, 0.01, 0.9, 0.002][:n_base]
    while True:
        logits = (torch.randn(n_base, V, generator=g) * 3).to(torch.bfloat16)
        words = torch.stack([sc._words(g, V) for _ in range(n_base)])
        temps = torch.randint(5, 12, (n_base,), generator=g).float() / 8
        top_p = torch.randint(60, 99, (n_base,), generator=g).float() / 100
        min_p = torch.randint(1, 10, (n_base,), generator=g).float() / 100
        blocks, offs, at = [], [], 0
        for b in range(n_base):
            allow = (torch.rand(V, generator=g) < frac[b]).nonzero().reshape(-1).tolist()
            top = logits[b].float().topk(40).indices.tolist()
            bias = {int(t): float(v) for t, v in zip(top, (torch.rand(40, generator=g) * 6 - 3).tolist())}
            p = params_of(allowed_token_ids=allow, logit_bias=bias)
            blk = cn.compile_program(p, [EOS], V).words
            blocks.append(blk)
            offs.append(at)
            at += blk.numel()
        pool = torch.cat(blocks)
        prog = torch.tensor(offs, dtype=torch.int32)
        crows = ref.con_rows(pool, torch.zeros(n_base, dtype=torch.int32), prog, torch.arange(n_base), V)
        l = ref.constrain_logits(logits, words, rep, freq, pres, crows, torch.zeros(n_base, dtype=torch.int32))
        if all(finite_margins(l[b], float(temps[b]), int(top_k[b]), float(top_p[b]), float(min_p[b]), 0.5)[1]
               >= MARGIN for b in range(n_base)):
            break
    u = torch.rand(n_base * n_u, generator=g)
    _, kept = ref.sample_candidates(l, temps, top_k.long(), top_p, min_p, torch.zeros(n_base), dtype=torch.float64,
                                    return_kept=True)
    base = torch.arange(n_base).repeat_interleave(n_u)
    return SimpleNamespace(V=V, B=n_base * n_u, base=base, logits=logits, words=words, rep=rep, freq=freq, pres=pres,
                           top_k=top_k, temps=temps, top_p=top_p, min_p=min_p, u=u, kept=kept,
                           allowed=torch.isfinite(l), pool=pool, prog=prog)
