"""Constrained sampling on the host: the compiler from a request's options to a constraint program, the host
automaton, and the device pool with its program cache.

A request's ``logit_bias`` / ``allowed_token_ids`` / ``bad_words_ids`` / ``min_tokens`` / ``guided_choice`` compile
to one immutable PROGRAM (``ops.reference.con_pack``: per-state allow-masks, a stop mask, sparse transitions with a
default, a sparse bias), shared by every request with equal options.  The sampler kernel applies the mask of the
sequence's current state while it loads the logits and advances the state word when it picks, so look-ahead decode
keeps working; the host replays the same automaton (``Program.advance``) only to (re)initialise a state word on
admission.  ``compile_program`` is a pure function of (options, stop set, V): tensor-parallel ranks agree.
"""
from __future__ import annotations

import math
import numbers
import os
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..ops import reference as ref

MAX_STATES = ref.CON_MAX_STATES
MAX_BIAS = ref.CON_MAX_BIAS
POOL_ENV = "SHAI_CONSTRAINT_POOL_MIB"
FIELDS = ("logit_bias", "allowed_token_ids", "bad_words_ids", "min_tokens", "guided_choice")


def _is_int(x) -> bool:
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def _id_list(xs, name) -> List[int]:
    if not isinstance(xs, (list, tuple)) or not all(_is_int(t) and t >= 0 for t in xs):
        raise ValueError(f"{name} must be a list of non-negative token ids, got {xs!r}")
    return [int(t) for t in xs]


def validate(p) -> None:
    """The checks that need no vocabulary size (``SamplingParams.validate``); ids are range-checked at compile."""
    if p.logit_bias is not None:
        if not isinstance(p.logit_bias, dict):
            raise ValueError(f"logit_bias must be a dict of token id -> value, got {p.logit_bias!r}")
        if len(p.logit_bias) > MAX_BIAS:
            raise ValueError(f"logit_bias holds {len(p.logit_bias)} entries, at most {MAX_BIAS} are allowed")
        for k, v in p.logit_bias.items():
            if not (_is_int(k) and k >= 0):
                raise ValueError(f"logit_bias key {k!r} is not a token id")
            if not (isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v) and -100 <= v <= 100):
                raise ValueError(f"logit_bias[{k}] must be finite and in [-100, 100], got {v!r}")
    if p.allowed_token_ids is not None:
        if not _id_list(p.allowed_token_ids, "allowed_token_ids"):
            raise ValueError("allowed_token_ids must not be empty")
    for name in ("bad_words_ids", "guided_choice"):
        xs = getattr(p, name)
        if xs is None:
            continue
        if not isinstance(xs, (list, tuple)) or (name == "guided_choice" and not xs):
            raise ValueError(f"{name} must be a{' non-empty' if name == 'guided_choice' else ''} list of token-id "
                             f"lists, got {xs!r}")
        for w in xs:
            if not _id_list(w, f"{name} entry"):
                raise ValueError(f"{name} holds an empty entry")
    if not (_is_int(p.min_tokens) and p.min_tokens >= 0):
        raise ValueError(f"min_tokens must be an integer >= 0, got {p.min_tokens!r}")
    if p.min_tokens > p.max_tokens:
        raise ValueError(f"min_tokens ({p.min_tokens}) exceeds max_tokens ({p.max_tokens})")
    if p.guided_choice is not None:
        if p.ignore_eos:
            raise ValueError("guided_choice cannot be combined with ignore_eos: a choice ends with a stop token")
        if p.min_tokens > 0:
            raise ValueError("guided_choice cannot be combined with min_tokens > 0 (no product automata)")
        if any(len(w) > 1 for w in p.bad_words_ids or ()):
            raise ValueError("guided_choice cannot be combined with a multi-token bad_words_ids entry (no product "
                             "automata)")


def needed(p) -> bool:
    """Whether the request needs a constraint program at all."""
    return bool(p.logit_bias) or p.allowed_token_ids is not None or bool(p.bad_words_ids) or p.min_tokens > 0 \
        or p.guided_choice is not None


def program_key(p, stop: Sequence[int], V: int) -> Tuple:
    """What a program depends on (min_tokens only through whether the stop set may be banned)."""
    t = lambda xs: None if xs is None else tuple(tuple(w) for w in xs)
    return (V, tuple(sorted(set(stop))), tuple(sorted((p.logit_bias or {}).items())),
            None if p.allowed_token_ids is None else tuple(sorted(set(p.allowed_token_ids))),
            t(p.bad_words_ids), t(p.guided_choice), p.min_tokens > 0)


class Program:
    """A compiled constraint program: the int32 block the kernel reads (``words``) and the same automaton for the
    host.  Immutable."""
    __slots__ = ("V", "S", "words", "default", "edges")

    def __init__(self, V, masks, stop, default, edges, bias):
        self.V, self.S = V, len(default)
        self.default = tuple(default)
        self.edges: Tuple[Dict[int, int], ...] = tuple(dict(e) for e in edges)
        self.words = ref.con_pack(V, masks, stop, default, [sorted(e.items()) for e in self.edges], bias)

    def advance(self, state: int, token: int) -> int:
        return self.edges[state].get(int(token), self.default[state])

    def replay(self, tokens: Sequence[int]) -> int:
        s = 0
        for t in tokens:
            s = self.advance(s, t)
        return s


def _check_ids(ids, V, name):
    for t in ids:
        if not 0 <= t < V:
            raise ValueError(f"{name}: token id {t} outside the vocabulary [0, {V})")


def _cap(n):
    if n > MAX_STATES:
        raise ValueError(f"the constraint program needs {n} states, at most {MAX_STATES} are supported")


def compile_program(p, stop: Sequence[int], V: int) -> Program:
    """Options -> program.  ``stop``: the ids that end this request (EOS unless ignored, and its stop_token_ids).
    Raises ValueError for ids out of range, more than MAX_STATES states, or a reachable state that allows nothing."""
    validate(p)
    stop = sorted(set(int(t) for t in stop))
    _check_ids(stop, V, "stop_token_ids")
    W = ref.con_words(V)
    bias = sorted((int(k), float(v)) for k, v in (p.logit_bias or {}).items())
    _check_ids([k for k, _ in bias], V, "logit_bias")
    base = torch.zeros(W * 32, dtype=torch.bool)
    if p.allowed_token_ids is not None:
        _check_ids(p.allowed_token_ids, V, "allowed_token_ids")
        base[torch.tensor(sorted(set(p.allowed_token_ids)), dtype=torch.int64)] = True
    else:
        base[:V] = True
    words = [list(map(int, w)) for w in p.bad_words_ids or ()]
    for w in words:
        _check_ids(w, V, "bad_words_ids")
    for w in words:
        if len(w) == 1:
            base[w[0]] = False
    stop_bits = torch.zeros(W * 32, dtype=torch.bool)
    if stop:
        stop_bits[torch.tensor(stop, dtype=torch.int64)] = True
    multi = [w for w in words if len(w) > 1]
    if p.guided_choice is not None:
        default, edges, rows = _trie(p.guided_choice, stop, stop_bits, base, V)
    elif multi:
        default, edges, rows = _aho_corasick(multi, base)
    else:
        default, edges, rows = [0], [{}], [base]
    bits = torch.stack(rows)
    live = bits & ~stop_bits if p.min_tokens > 0 else bits   # what a step that bans the stop set leaves
    empty = (~live.any(-1)).nonzero().reshape(-1).tolist()
    if empty:
        raise ValueError(f"the constraints leave nothing allowed in state {empty[0]} of the program (of {len(rows)}): "
                         "allowed_token_ids / bad_words_ids / guided_choice / min_tokens exclude every token there")
    return Program(V, ref.con_mask_pack(bits), ref.con_mask_pack(stop_bits), default, edges, bias)


def _trie(choices, stop, stop_bits, base, V):
    """guided_choice: state = trie node (0 the root); a node allows its children, a node that ends a choice also the
    stop set; the default transition stays (only a stop token takes it, and the sequence ends there)."""
    if not stop:
        raise ValueError("guided_choice needs a stop token (EOS or stop_token_ids) to end a choice with")
    children: List[Dict[int, int]] = [{}]
    ends = [False]
    for c in choices:
        _check_ids(c, V, "guided_choice")
        if any(t in stop for t in c):
            raise ValueError(f"guided_choice entry {list(c)!r} contains a stop token")
        s = 0
        for t in c:
            if t not in children[s]:
                children[s][t] = len(children)
                children.append({})
                ends.append(False)
                _cap(len(children))
            s = children[s][t]
        ends[s] = True
    rows = []
    for ch, end in zip(children, ends):
        m = torch.zeros_like(base)
        if ch:
            m[torch.tensor(sorted(ch), dtype=torch.int64)] = True
        if end:
            m |= stop_bits
        rows.append(m & base)
    return list(range(len(children))), children, rows


def _aho_corasick(words, base):
    """Multi-token bad words: the DFA over the words' proper prefixes (Aho-Corasick).  State = the longest suffix of
    the output that is a prefix of some word minus its last token; it bans the last token of every word whose other
    tokens end the output.  Explicit edges: every token whose target is not the root; default: the root."""
    goto: List[Dict[int, int]] = [{}]
    ban: List[set] = [set()]
    for w in words:
        s = 0
        for t in w[:-1]:
            if t not in goto[s]:
                goto[s][t] = len(goto)
                goto.append({})
                ban.append(set())
                _cap(len(goto))
            s = goto[s][t]
        ban[s].add(w[-1])
    fail = [0] * len(goto)
    delta: List[Dict[int, int]] = [dict(goto[0])] + [{} for _ in goto[1:]]
    order = list(goto[0].values())
    for s in order:                       # breadth first: a state's failure state is complete before it
        f = fail[s]
        ban[s] |= ban[f]
        delta[s] = dict(delta[f])
        delta[s].update(goto[s])
        for t, n in goto[s].items():
            fail[n] = delta[f].get(t, 0)
            order.append(n)
    rows = []
    for b in ban:
        m = base.clone()
        if b:
            m[torch.tensor(sorted(b), dtype=torch.int64)] = False
        rows.append(m)
    return [0] * len(goto), delta, rows


def pool_words_from_env() -> int:
    raw = os.environ.get(POOL_ENV, "64")
    try:
        mib = float(raw)
    except ValueError:
        raise ValueError(f"{POOL_ENV}={raw!r} is not a number") from None
    if not mib > 0:
        raise ValueError(f"{POOL_ENV} must be > 0, got {raw!r}")
    return max(ref.CON_HDR, int(mib * 2 ** 20) // 4)


class _Entry:
    __slots__ = ("key", "prog", "off", "refs")

    def __init__(self, key, prog, off):
        self.key, self.prog, self.off, self.refs = key, prog, off, 0


class ConstraintPool:
    """Device memory for program blocks and the cache of the programs in it.  One int32 buffer that never moves
    (decode graphs capture its address); blocks are first-fit allocated, a program is kept while sequences hold it
    and afterwards until its room is needed (zero-reference programs go least recently used first).  Blocks arrive
    by ordinary stream-ordered copies, so a block is never overwritten under a launch enqueued before."""

    def __init__(self, device, n_words: Optional[int] = None):
        n_words = pool_words_from_env() if n_words is None else int(n_words)
        try:
            self.buf = torch.zeros(n_words, dtype=torch.int32, device=device)
        except (RuntimeError, MemoryError) as e:   # torch.OutOfMemoryError is a RuntimeError
            raise MemoryError(f"no room for the constraint pool ({4 * n_words / 2 ** 20:.1f} MiB): lower {POOL_ENV} "
                              f"or gpu_memory_utilization: {e}") from None
        self.free: List[List[int]] = [[0, n_words]]            # [offset, length], by offset
        self.entries: "OrderedDict[Tuple, _Entry]" = OrderedDict()   # least recently used first

    def _alloc(self, n: int) -> int:
        for i, (off, ln) in enumerate(self.free):
            if ln >= n:
                if ln == n:
                    del self.free[i]
                else:
                    self.free[i] = [off + n, ln - n]
                return off
        return -1

    def _release_block(self, off: int, n: int) -> None:
        self.free.append([off, n])
        self.free.sort()
        out = [self.free[0]]
        for off, ln in self.free[1:]:
            if out[-1][0] + out[-1][1] == off:
                out[-1][1] += ln
            else:
                out.append([off, ln])
        self.free = out

    def acquire(self, key: Tuple, make) -> _Entry:
        """The entry of ``key`` with one more reference; ``make()`` compiles the program if it is not cached.
        MemoryError if it does not fit after every unreferenced program is evicted."""
        e = self.entries.get(key)
        if e is None:
            prog = make()
            n = prog.words.numel()
            off = self._alloc(n)
            while off < 0:
                victim = next((v for v in self.entries.values() if v.refs == 0), None)
                if victim is None:
                    raise MemoryError(f"the constraint program ({4 * n / 2 ** 20:.2f} MiB) does not fit the constraint "
                                      f"pool ({4 * self.buf.numel() / 2 ** 20:.2f} MiB, programs of live requests "
                                      f"hold the rest): raise {POOL_ENV}")
                del self.entries[victim.key]
                self._release_block(victim.off, victim.prog.words.numel())
                off = self._alloc(n)
            self.buf[off:off + n].copy_(prog.words, non_blocking=False)
            e = self.entries[key] = _Entry(key, prog, off)
        self.entries.move_to_end(key)
        e.refs += 1
        return e

    def release(self, e: _Entry) -> None:
        assert e.refs > 0
        e.refs -= 1
