"""The attention edge tests, tested (no GPU): the bound C follows from the CPU emulation of the kernels' rounding,
every off-by-one-key mutant of the oracle's mask fails the strict rule, the unmutated oracle passes it -- and the
suite's older close() rule on plain randn inputs accepts the long-row mutants, which is why tests/attn_edges.py
exists."""
import math

import pytest
import torch

import attn_edges as ae

_cases = {}


def case(name):
    """(case, [(index, q, k, v, vis, bias)], oracle) -- built once per name, never modified."""
    if name not in _cases:
        c = ae.make(name)
        _cases[name] = (c, list(ae.sequences(c)), ae.oracle(c))
    return _cases[name]


def kv_len(c, b):
    return c.kv_list[b] if c.kv_list is not None else c.Skv


def mutant_fails(name, b, vis2):
    """The oracle of sequence b with the visible-key counts vis2, rounded to bf16, must fail against the real one."""
    c, seqs, ref = case(name)
    _, q, k, v, vis, bias = seqs[b]
    vis2 = vis2.clamp(0, k.shape[0])
    rows = (vis2 != vis).nonzero()[:, 0]   # the other rows are the oracle's own
    assert len(rows), "the mutation changes nothing"
    o, _ = ae.attend64(q[rows], k, v, vis2[rows], c.scale, None if bias is None else bias[:, rows])
    o64, a = ref[b][1][rows], ref[b][2][rows]
    with pytest.raises(AssertionError, match="out of bound"):
        ae.assert_edges_close(o.to(torch.bfloat16), o64, a, what=name)
    # ... by a wide margin: |err| / a_abs >= 1 somewhere, at least 16 times the bound (C <= 1 / 16)
    assert float(((o - o64).abs() / a.clamp_min(ae.ABS)).max()) >= 1.0


def test_c_is_capped():
    assert ae.C <= 1 / 16
    assert 4 * ae.FLOOR <= ae.C


@pytest.mark.parametrize("name", list(ae.CASES))
def test_floor(name):
    """Four times the rounding emulation's worst |emu - o64| / a_abs stays within C, case by case."""
    f = ae.floor_of(case(name)[0])
    print(f"{name}: floor {f:.5f}, 4x = {4 * f:.5f}, C = {ae.C}")
    assert 4 * f <= ae.C


@pytest.mark.parametrize("name", list(ae.CASES))
def test_reference_passes_and_probes_dominate(name):
    c, _, ref = case(name)
    for (b, rows), o64, a in ref:
        ae.assert_edges_close(o64.to(torch.bfloat16), o64, a, what=name)
    assert ae.probes_dominate(c, ref) >= 0.95   # a probed row returns its planted +-8


DENSE_LENS = ["v1_d128", "v1_d64_bias", "f64dma", "f64dma_cross", "f64dma_shared_q", "f64x2", "f128", "knob_d64"]


@pytest.mark.parametrize("name", DENSE_LENS + ["f64dma_causal", "f128_causal", "v1_d128_causal_qlens"])
@pytest.mark.parametrize("d", [1, -1])
def test_mutant_kv_len(name, d):
    """kv_len + 1 (the poison key leaks) and kv_len - 1 (the last valid key is dropped), every batch."""
    c, seqs, _ = case(name)
    for b in range(len(seqs)):
        vis = seqs[b][4]
        kl = kv_len(c, b)
        mutant_fails(name, b, torch.where(vis >= kl, vis + d, vis))


@pytest.mark.parametrize("name", DENSE_LENS)
def test_mutant_partial_last_key_tile_dropped(name):
    c, seqs, _ = case(name)
    n = 0
    for b in range(len(seqs)):
        kl = kv_len(c, b)
        if kl % 64 and kl > 64:
            mutant_fails(name, b, seqs[b][4].clamp(max=kl // 64 * 64))
            n += 1
    assert n


CAUSAL = ["v1_d128_causal", "v1_d128_causal_qlens", "f64dma_causal", "f64x2_causal", "f128_causal", "f128_chunk",
          "knob_d64", "knob_d128", "paged_prefill"]


def _diag(vis, kl, d, rows):
    """The causal diagonal moved by d keys in ``rows`` (the kv_len edge stays where it is)."""
    return torch.where(rows, (vis + d).clamp(0, kl), vis)


@pytest.mark.parametrize("name", CAUSAL)
@pytest.mark.parametrize("d", [1, -1])
def test_mutant_diagonal_all_rows(name, d):
    c, seqs, _ = case(name)
    for b in range(len(seqs)):
        vis = seqs[b][4]
        if len(vis) > 1:   # a single query row ending at kv_len - 1 has no diagonal of its own
            mutant_fails(name, b, _diag(vis, kv_len(c, b), d, torch.ones_like(vis, dtype=torch.bool)))


@pytest.mark.parametrize("name", ["f64x2_causal", "f128_causal", "knob_d64", "knob_d128"])
@pytest.mark.parametrize("d", [1, -1])
def test_mutant_diagonal_rows_from_1024(name, d):
    c, seqs, _ = case(name)
    n = 0
    for b in range(len(seqs)):
        vis = seqs[b][4]
        if len(vis) > 1026:
            mutant_fails(name, b, _diag(vis, kv_len(c, b), d, torch.arange(len(vis)) >= 1024))
            n += 1
    assert n


@pytest.mark.parametrize("name", CAUSAL)   # f128_chunk: causal_offset = 900
@pytest.mark.parametrize("d", [1, -1])
def test_mutant_diagonal_one_probed_row(name, d):
    c, seqs, _ = case(name)
    n = 0
    for b, r, e, _ in c.probes:
        vis = seqs[b][4]
        kl = kv_len(c, b)
        if e == kl - 1 and d > 0:
            continue   # this row's edge is kv_len, not the diagonal (test_mutant_kv_len moves it)
        mutant_fails(name, b, _diag(vis, kl, d, torch.arange(len(vis)) == r))
        n += 1
    assert n


@pytest.mark.parametrize("name", [n for n in ae.CASES if n.startswith("decode")])
@pytest.mark.parametrize("d", [1, -1])
def test_mutant_decode_ctx(name, d):
    """ctx + 1 and ctx - 1 at every context length of the decode cases (bf16 and fp8 caches)."""
    c, seqs, _ = case(name)
    assert c.kv_list == ae.DECODE_CTX
    for b in range(len(seqs)):
        mutant_fails(name, b, seqs[b][4] + d)


# ----------------------------------------------------------------------------- the gap this file closes
def close(a, b, atol, rtol=2e-2):   # the rule of tests/test_kernels_gpu.py, test_kv8_gpu.py, test_kv8_prefill_gpu.py
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    assert torch.isfinite(a).all(), "non-finite output"
    assert bad < 1e-3, f"{bad*100:.3f}% elements out of tolerance; max err {err.max().item():.4g}"
    return bad


def _plain(S, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    return r(S, 4, 64), r(S, 2, 64), r(S, 2, 64)


def test_old_rule_accepts_the_long_row_mutants():
    """On record: with plain randn inputs at the suite's long-row shapes, close() (2e-2 + 2e-2 |ref|, 0.1 % of the
    elements free) accepts a leaked masked key, a dropped last key, a dropped partial last key tile, and a causal
    diagonal that is one key off for every row from 1024 on."""
    sc = 1 / math.sqrt(64)
    S, kl = 2200, 2190   # test_flash2_d64_long_spikes_varlen's shape, one batch
    q, k, v = _plain(S, 1)
    vis = torch.full((S,), kl)
    want = ae.attend64(q, k, v, vis, sc)[0].to(torch.bfloat16)
    mutants = (("kv_len + 1", vis + 1), ("kv_len - 1", vis - 1), ("tail tile dropped", vis.clamp(max=kl // 64 * 64)))
    for what, vis2 in mutants:
        got = ae.attend64(q, k, v, vis2, sc)[0].to(torch.bfloat16)
        assert not torch.equal(got, want)
        print(f"{what}: close() flags {close(got, want, 2e-2) * 100:.4f} % of the elements")
    S = 1100             # test_flash64_x2_large_grid's rows, causal
    q, k, v = _plain(S, 2)
    vis = torch.arange(S) + 1
    want = ae.attend64(q, k, v, vis, sc)[0].to(torch.bfloat16)
    vis2 = torch.where(torch.arange(S) >= 1024, (vis + 1).clamp(max=S), vis)
    got = ae.attend64(q, k, v, vis2, sc)[0].to(torch.bfloat16)
    assert not torch.equal(got, want)
    print(f"diagonal + 1 from row 1024: close() flags {close(got, want, 2e-2) * 100:.4f} % of the elements")
