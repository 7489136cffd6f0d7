"""Inputs for tests/test_full_vocab_sampler_gpu.py: plain helpers, CPU tensors the tests never modify.  Logits are
integers in [-8, 8], penalties dyadic and T >= 0.5 (as tests/sampler_cases.py): both sides order identical values."""
import functools
from types import SimpleNamespace

import torch

import sampler_cases as sc
from shai_amd.ops import reference as ref

LADDER = torch.tensor([8] * 2 + [7] * 3 + [6] * 4 + [5] * 10 + [4] * 20 + [3] * 11).float()


def every_third(V):
    """The block of a one-state constraint program that allows the tokens 0, 3, 6, ..."""
    mask = ref.con_mask(range(0, V, 3), V)
    return ref.con_pack(V, mask[None], torch.zeros_like(mask), [0], [[]])


@functools.lru_cache(maxsize=None)
def ladder_case(V, kind):
    """Head-resolved rows: ~50 tokens at 3..8 over a bulk <= 0, one row per top_k in (0, -1, V, 1025), CALLS calls
    whose T / top_p / min_p / u leave every decision a margin of sc.MARGIN of the total in fp64 (the bulk must still be
    summed right).  kind: plain / pen / con.  ``tokens`` [CALLS, B] and ``states`` are the fp64 oracle's."""
    g = torch.Generator().manual_seed(V + len(kind))
    top_k, B = torch.tensor([0, -1, V, 1025], dtype=torch.int32), 4
    logits = torch.randint(-8, 1, (B, V), generator=g).float()
    for b in range(B):
        logits[b, torch.randperm(V, generator=g)[:LADDER.numel()]] = LADDER
    pen = kind != "plain"
    state = torch.stack([sc._words(g, V) for _ in range(B + 2)]) if pen else None   # rows 0 and B + 1: canaries
    rows = torch.arange(1, B + 1, dtype=torch.int32)
    rep, freq, pres = torch.full((B,), 2.0), torch.full((B,), 0.5), torch.full((B,), 0.25)
    pool = every_third(V) if kind == "con" else None
    prog, slot = torch.zeros(B, dtype=torch.int32), torch.arange(B, dtype=torch.int32)
    ban, cstate = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    temps, top_p, min_p, u = (torch.zeros(sc.CALLS, B) for _ in range(4))
    tokens, states = [], [state]
    for c in range(sc.CALLS):
        st = states[-1].clone() if pen else None
        words = ref.penalty_words(st, rows, B, V, "cpu") if pen else None
        l = logits if not pen else ref.constrain_logits(logits, words, rep, freq, pres,
                                                        ref.con_rows(pool, cstate, prog, slot, V), ban)
        for b in range(B):
            for _ in range(400):
                T = float(torch.randint(4, 13, (1,), generator=g)) / 8
                tp = float(torch.randint(50, 100, (1,), generator=g)) / 100
                mp = float(torch.randint(1, 30, (1,), generator=g)) / 100 if pen and b % 2 else 0.0
                uu = float(torch.rand(1, generator=g))
                if sc.margins(l[b], T, int(top_k[b]), tp, mp, uu)[0] >= sc.MARGIN:
                    break
            else:
                raise AssertionError(f"no parameters with a margin for V={V} {kind} row {b}")
            temps[c, b], top_p[c, b], min_p[c, b], u[c, b] = T, tp, mp, uu
        tokens.append(ref.sample_candidates(l, temps[c], top_k.long(), top_p[c], min_p[c], u[c], dtype=torch.float64))
        if pen:
            ref.penalty_state_add(st, rows, tokens[-1])
            states.append(st)
    return SimpleNamespace(V=V, B=B, kind=kind, logits=logits, top_k=top_k, temps=temps, top_p=top_p, min_p=min_p,
                           u=u, rows=rows, rep=rep, freq=freq, pres=pres, pool=pool, prog=prog, slot=slot, ban=ban,
                           cstate=cstate, tokens=torch.stack(tokens), states=states)


@functools.lru_cache(maxsize=None)
def bulk_case(V=128256):
    """A flat-ish row (integers in [-2, 2], T = 1) under the every-third mask and min_p 0.1 (drops the -1s and -2s),
    at top_p 1.0 and 0.9 times eight uniforms: ~25,000 kept tokens.  ``lo`` / ``hi`` [V]: per token the fp64 mass
    before / through it in sorted order (inf / -inf: never drawn); ``target`` = u * kept mass."""
    g = torch.Generator().manual_seed(5)
    row = torch.randint(-2, 3, (V,), generator=g).float()
    top_p, u, B = torch.tensor([1.0, 0.9]).repeat_interleave(8), ((torch.arange(8) + 0.5) / 8).repeat(2), 16
    l = torch.where(ref.con_mask_bits(ref.con_mask(range(0, V, 3), V), V), row, torch.tensor(float("-inf")))
    vals, idx = torch.sort(l, descending=True, stable=True)
    p = torch.exp((vals - vals[0]).double()) * (vals > float("-inf"))
    p = p * (p >= 0.1)
    cum = p.cumsum(0)
    total = float(cum[-1])
    lo, hi = torch.empty(V, dtype=torch.float64), torch.empty(V, dtype=torch.float64)
    lo[idx] = torch.where(p > 0, cum - p, torch.tensor(float("inf"), dtype=torch.float64))
    hi[idx] = torch.where(p > 0, cum, torch.tensor(float("-inf"), dtype=torch.float64))
    kept = torch.stack([cum[int(((cum - p) <= float(tp) * total).sum()) - 1] for tp in top_p.double()])
    return SimpleNamespace(V=V, B=B, logits=row.expand(B, V).contiguous(), top_p=top_p, u=u, lo=lo, hi=hi,
                           target=u.double() * kept, total=total, pool=every_third(V))
