"""The row-wise / element-wise kernel tests, tested (no GPU): the committed cases of tests/rowwise_exact.py meet the
preconditions of their rules (exact sums, dyadic tables, more than two grid caps of loop items, the measured K floor
inside its cap), the fp32 references pass the rules, and every mutant of the explicit-index models fails them -- while
the older rules (close() with its 0.1 % allowance, assert_close(1e-3) on GroupNorm statistics) accept the number of
mutants printed by each test and recorded in COVERAGE.md."""
import pytest
import torch

import gemm_exact as ge
import rowwise_exact as rx
from shai_amd.ops import reference as ref

BF16 = torch.bfloat16
ACCEPTED = {}     # family -> (mutant runs, runs the old rule accepts)


def _old_close(mutant, want):
    return ge.close_bad_share(mutant, want) < 1e-3


def _tally(family, accepted):
    n, a = ACCEPTED.get(family, (0, 0))
    ACCEPTED[family] = (n + 1, a + int(accepted))


# ----------------------------------------------------------------------------- 1. preconditions
def test_k_floor():
    """The fp32 evaluation of the row norms stays within K_FLOOR 2^-24 M of fp64 on every committed case, K is 4 times
    that and inside the cap of 256."""
    worst, name = 0.0, None
    for n in rx.ROWNORM_CASES:
        f = rx.rownorm_floor(rx.make_rownorm(n))
        if f > worst:
            worst, name = f, n
    print(f"row-norm floor {worst:.3f} at {name} over {len(rx.ROWNORM_CASES)} cases; K_FLOOR {rx.K_FLOOR}, K {rx.K}")
    assert worst <= rx.K_FLOOR
    assert rx.K == 4 * rx.K_FLOOR and rx.K <= rx.K_CAP


def test_row_norm_cases_cover_the_kernels():
    """All eight NV instances, all five MAXC instances, rows 1 / 5 / 37, D no multiple of 64, one live lane in the
    last chunk; row sums exact in fp32 in any order; residual sums that need the rounding to bf16."""
    assert sorted({D // 64 for D in rx.D8ROW}) == list(range(1, 9)) and all(rx.is_row8(D) for D in rx.D8ROW)
    maxc = {min(m for m in (1, 2, 4, 8, 16) if m >= (D + 511) // 512) for D in rx.DWAVE}
    assert maxc == {1, 2, 4, 8, 16} and not any(rx.is_row8(D) for D in rx.DWAVE)
    assert any((D - 8) % 512 == 0 for D in rx.DWAVE)
    rounded = 0
    for n in rx.ROWNORM_CASES:
        c = rx.make_rownorm(n)
        x = c.view("x")
        assert torch.equal(x.float().sum(-1).double(), x.double().sum(-1)), n
        assert torch.equal(x.float().flip(-1).sum(-1).double(), x.double().sum(-1)), n
        if c.residual:
            s = c.f64("x") + c.f64("r")
            rounded += int((rx.rownorm_h(c).double() != s).sum())
        if c.mod:
            assert c.rows % c.mod or c.mod == 1, n       # the last group is partial
    assert rounded > 1000
    assert {rx.ROWNORM_CASES[n]["mod"] for n in rx.ROWNORM_CASES if n.startswith("mod_")} == {1, 3, 77}


@pytest.mark.parametrize("name", [n for n in rx.ROWNORM_CASES if "_r37_" in n or "_res_" in n or n.startswith("mod_")])
def test_row_norm_reference_and_model_pass(name):
    """ops.reference (fp32, residual rounded to bf16 first) and the unmutated index model pass the rule."""
    c = rx.make_rownorm(name)
    x, w, b = c.view("x"), c.view("w"), c.view("b")
    if c.mod:
        y, res = ref.layernorm_mod(x, w, b, c.mod, c.eps), None
    elif c.norm == "rms":
        y, res = ref.rmsnorm(x, w, c.eps, c.view("r"), c.w_offset)
    else:
        y, res = ref.layernorm(x, w, b, c.eps, c.view("r"))
    h, y64, tol = rx.rownorm_want(c)
    if c.norm == "rms" or c.family == "random":
        # (F.layer_norm's running moments lose the mean of a spike row whose eight spikes nearly cancel: -1.50e-6 for
        # -1.80e-6 at ln_D2056_r37_one_lane; the plain formula of test_k_floor and the kernels sum such rows exactly)
        rx.assert_within(y, y64, tol, name + " reference")
    if c.residual:
        rx.assert_exact(res, h, name + " reference residual")
    out, rfull = rx.rownorm_model(c)
    rx.check_rownorm(c, out, rx.rownorm_out(c)[1], rfull, rx.rows_out(c.rows, c.D)[1], name + " model")


def test_tables_are_dyadic_and_distinct():
    g = rx._gen(1)
    (cb, ci), (sb, si) = rx.rope_table(g, 129, 129)
    co, si_ = cb[ci] * 64, sb[si] * 64
    assert torch.equal(co, co.round()) and torch.equal(si_, si_.round())
    assert float(co.abs().max()) <= 64 and float(si_.abs().max()) <= 64
    pairs = (co.long() + 64) * 129 + (si_.long() + 64)
    assert pairs.unique().numel() == 129 * 129
    for name, (fn, _) in rx.GRID_CASES.items():
        c = rx.make_grid(name)
        if c.has("cos"):
            assert torch.equal(c.view("cos") * 64, (c.view("cos") * 64).round()), name


@pytest.mark.parametrize("name", list(rx.QKNR_CASES))
def test_qk_norm_rope_reference_passes(name):
    c = rx.make_qknr(name)
    x = c.bufs["x"].clone()
    ref.qk_norm_rope(x[1:1 + c.rows, :3 * c.H * c.D], c.view("qw"), c.view("kw"), c.view("cos"), c.view("sin"), c.H,
                     c.D, c.S, c.eps)
    rx.check_qknr(c, x)
    assert x.shape[1] > 3 * c.H * c.D and c.rows % 4


def test_gn_cases():
    """Every sum below 2^24, probes at the ends of every stats block, the extra HW of each C gives more than one block
    with ppb no multiple of 4 P, two-source cases split a group; the model's pixel walk and ops.reference agree with
    the oracle."""
    for C, HW in rx.GN_HW_EXTRA.items():
        for N in (1, 3):
            nb, ppb, P = rx.gn_geometry(N, HW, C)
            assert nb > 1 and ppb % (4 * P), (C, HW, N, nb, ppb, P)
    assert rx.gn_geometry(1, 100, 320) == (3, 34, 6)
    assert any(rx.gn_geometry(3, kw["HW"], kw["C"])[1] > 4 * rx.gn_geometry(3, kw["HW"], kw["C"])[2]
               for kw in rx.GN_CASES.values())           # the 4-deep loop and its tail both run
    for name, kw in rx.GN_CASES.items():
        c = rx.make_gn(name)
        x = rx.gn_x64(c)
        want = rx.gn_sums64(x.view(c.N, c.HW, c.G, -1))
        assert float(rx.gn_sums64(x.abs().view(c.N, c.HW, c.G, -1)).max()) < rx.LIMIT, name
        nb, ppb, _ = rx.gn_geometry(c.N, c.HW, c.C)
        for blk in range(nb):
            for p in (blk * ppb, min(c.HW, (blk + 1) * ppb) - 1):
                if 0 <= p < c.HW:
                    assert float(x[:, p].abs().min()) >= 8, (name, p)
        assert torch.equal(rx.gn_model_sums(c), want), name
        if c.has("x2"):
            assert c.C1 % (c.C // c.G) and c.C1 % 8 == 0
        sc, sh = ref.groupnorm_stats(x.to(BF16), c.view("gamma"), c.view("beta"), c.G, rx.GN_EPS)
        rx.check_gn(c, sc, sh, name + " reference")


def test_grid_cases_take_three_trips():
    for name in rx.BIG:
        c = rx.make_grid(name)
        cap = rx.CAP_RQC if c.kind == "rqc" else rx.CAP
        assert rx.grid_items(c) > 2 * cap, name
    small = [n for n in rx.GRID_CASES if "_small" in n]
    assert all(rx.grid_items(rx.make_grid(n)) < rx.CAP for n in small) and len(small) >= 20


@pytest.mark.parametrize("name", [n for n, (fn, _) in rx.GRID_CASES.items() if "_small" in n])
def test_grid_small_references_pass(name):
    """The fp32 references of ops.reference pass the rule of every small case (the big ones share the code path)."""
    _reference_passes(rx.make_grid(name))


def _reference_passes(c):
    n, k = c.name, c.kind
    if k == "gated":
        for gf in (False, True):
            y, z = rx.gated_want(c, gf)
            got = ref.gated_act(c.view("x"), c.act, gf)
            rx.assert_smooth(got, y, z, n) if c.smooth else rx.assert_exact(got, rx.to_bf16_exact(y), n)
    elif k == "bias_act":
        y, z = rx.bias_act_want(c)
        got = ref.bias_act(c.view("x"), c.view("bias"), c.view("residual"), c.act, c.alpha)
        rx.assert_smooth(got, y, z, n) if c.smooth else rx.assert_exact(got, rx.to_bf16_exact(y), n)
    elif k == "rope":
        wb = rx.to_bf16_exact(rx.rope_model(c))
        q = rx.rope_view(c, c.view("x")).clone()
        ref.rope(q, c.pos, c.view("cos"), c.view("sin"), c.rot, c.neox)
        rx.assert_exact(q, rx.rope_view(c, wb[1:1 + c.T]), n)
    elif k == "rope_pairs":
        want = rx.to_bf16_exact(rx.rope_pairs_want(c))
        x = c.view("x").clone().unflatten(2, (c.H, c.Dh))
        ref.rope_pairs(x, c.view("cos"), c.view("sin"))
        rx.assert_exact(x.flatten(2), want[:, :c.T, :c.H * c.Dh], n)
    elif k == "kvw":
        kw, vw = rx.kvw_want(c)
        kc = torch.full((c.nblocks, c.Hkv, 64, c.D), rx.SENTINEL, dtype=BF16)
        vc = kc.clone()
        ref.kv_write(c.view("k").unflatten(1, (c.Hkv, c.D)), c.view("v").unflatten(1, (c.Hkv, c.D)), kc, vc, c.slots)
        rx.assert_exact(kc, kw.to(BF16), n)
        rx.assert_exact(vc, vw.to(BF16), n)
        assert int((c.slots < 0).sum()) > 0
    elif k == "rqc":
        import shai_amd.ops as ops
        full, kw, vw = rx.rqc_model(c)
        x = c.bufs["x"].clone()
        kc = torch.full((c.nblocks, c.Hkv, 64, c.D), rx.SENTINEL, dtype=BF16)
        vc = kc.clone()
        ops.rope_qkv_cache(x[1:1 + c.T, :(c.H + 2 * c.Hkv) * c.D], c.pos, c.view("cos"), c.view("sin"), kc, vc, c.slots,
                           c.H, c.Hkv)
        rx.assert_exact(x, rx.to_bf16_exact(full), n)
        rx.assert_exact(kc, kw.to(BF16), n)
        rx.assert_exact(vc, vw.to(BF16), n)
        assert c.H > c.Hkv and int((c.slots < 0).sum()) > 0
    elif k == "sched":
        y, terms, active = rx.sched_want(c)
        lat = c.view("lat").clone()
        if c.B:
            ref.sched_step_rows(c.view("mo"), lat.view(c.B, -1), c.cfg, c.guidance, c.pred, c.rows_params)
            assert 0 < int(active.sum()) < c.n
        else:
            ref.sched_step(c.view("mo"), lat, c.cfg, c.guidance, c.pred, c.a_t, c.a_prev, c.dt)
        if c.pred == 2:
            rx.assert_exact(lat, rx.to_bf16_exact(y), n)
        else:
            rx.assert_smooth(lat[active], y[active], terms[active], n)
            rx.assert_exact(lat[~active], c.view("lat")[~active], n)
    elif k == "embedding":
        assert int(c.ids.max()) < c.vocab


@pytest.mark.parametrize("D", [8, 2048, 2056, 4096])
def test_softmax_rule_accepts_fp32(D):
    c = rx.make_grid(f"softmax_D{D}")
    y = torch.softmax(c.f64("x") * c.scale, -1)
    assert float((c.f64("x") * c.scale).amax(-1).sub((c.f64("x") * c.scale).amin(-1)).max()) <= 20
    rx.assert_within(torch.softmax(c.view("x").float() * c.scale, -1).to(BF16), y, rx.ulp_bf16(y), c.name)
    assert float(y.min()) > 2.0 ** -120


# ----------------------------------------------------------------------------- 2. mutants
def _rownorm_mutant_cases(mut):
    names = list(rx.ROWNORM_CASES)
    cs = [(n, rx.ROWNORM_CASES[n]) for n in names]
    if mut == "stats_short":      # visible where the last 16-byte vector carries the row's energy
        return [n for n, k in cs if k["family"] in ("spike_last", "one_lane")]
    if mut == "mirror_stats":
        return [n for n, k in cs if rx.is_row8(k["D"]) and k["rows"] % 8]
    if mut == "w_neighbour":
        return [n for n, k in cs if (k.get("w", True) or k.get("mod")) and k["family"] != "one_lane"
                and not (k["family"] == "spike_first" and k["D"] > 8)]
    if mut == "mod_per_wave":
        return [n for n, k in cs if k.get("mod")]
    if mut in ("x_stride_D", "out_stride_D"):
        return [n for n, k in cs if k.get("layout") == "cols"]
    if mut == "res_dead_lanes":
        return [n for n, k in cs if k.get("residual") and rx.is_row8(k["D"]) and k["rows"] % 8]
    raise ValueError(mut)


@pytest.mark.parametrize("mut", ["stats_short", "mirror_stats", "w_neighbour", "mod_per_wave", "x_stride_D",
                                 "out_stride_D", "res_dead_lanes"])
def test_row_norm_mutant_fails_the_rule(mut):
    """Each addressing mistake of the row norms fails the rule on every committed case it applies to; how many of
    these runs close() accepts is printed."""
    names = _rownorm_mutant_cases(mut)
    assert len(names) >= 2
    accepted = 0
    for n in names:
        c = rx.make_rownorm(n)
        out, rfull = rx.rownorm_model(c, mut)
        idx = rx.rownorm_out(c)[1]
        with pytest.raises(AssertionError, match="differ"):
            rx.check_rownorm(c, out, idx, rfull, rx.rows_out(c.rows, c.D)[1], n)
        ok = _old_close(out[idx], rx.rownorm_want(c)[1])    # close() looks at the output view only
        accepted += ok
        _tally("row norms", ok)
    print(f"{mut}: {len(names)} cases, all fail the rule; close() accepts {accepted}")


GN_MUTANTS = ["last_pixel_dropped", "boundary_twice", "second_vector_dropped", "x2_stride_c1", "span_group_x_only"]


@pytest.mark.parametrize("mut", GN_MUTANTS)
def test_gn_mutant_fails_the_rule(mut):
    names = []
    for n, kw in rx.GN_CASES.items():
        nb = rx.gn_geometry(kw["N"], kw["HW"], kw["C"])[0]
        if (mut == "last_pixel_dropped" or (mut == "boundary_twice" and nb > 1)
                or (mut == "second_vector_dropped" and kw["C"] > 2048)
                or (mut in ("x2_stride_c1", "span_group_x_only") and kw.get("C1"))):
            names.append(n)
    assert len(names) >= 2
    accepted = 0
    for n in names:
        c = rx.make_gn(n)
        sc, sh, _, _ = rx.gn_finish64(c, rx.gn_model_sums(c, mut))
        with pytest.raises(AssertionError, match="differ"):
            rx.check_gn(c, sc.float(), sh.float(), n)
        want_sc, want_sh, _, _ = rx.gn_want(c)
        ok = (torch.allclose(sc, want_sc, atol=1e-3, rtol=1e-3) and torch.allclose(sh, want_sh, atol=1e-3, rtol=1e-3))
        accepted += ok
        _tally("gn_stats", ok)
    print(f"{mut}: {len(names)} cases, all fail the rule; assert_close(1e-3) accepts {accepted}")


def _trip_setup(c):
    """(buffer before, expected buffer, loop item per element, cap) of a big case's output, as fp64 / int tensors."""
    k = c.kind
    if k in ("gated", "bias_act", "embedding"):
        rows, D = (c.rows, c.F) if k == "gated" else (c.rows, c.D) if k == "bias_act" else (c.T, c.D)
        y = rx.gated_want(c, False)[0] if k == "gated" else rx.bias_act_want(c)[0] if k == "bias_act" else \
            c.f64("table")[c.ids.long()]
        item = rx.gated_items(c) if k == "gated" else rx.flat8_items(rows, D)
        return torch.full((rows, D), rx.SENTINEL, dtype=torch.float64), y, item, rx.CAP
    if k == "rope":
        return c.bufs["x"].double(), rx.rope_model(c), rx.rope_model(c, items=True), rx.CAP
    if k == "rope_pairs":
        return c.bufs["x"].double(), rx.rope_pairs_want(c), rx.rope_pairs_items(c), rx.CAP
    if k == "kvw":
        return (torch.full((c.nblocks, c.Hkv, 64, c.D), rx.SENTINEL, dtype=torch.float64), rx.kvw_want(c)[1],
                rx.kvw_want(c, want_items=True)[1], rx.CAP)
    if k == "rqc":
        return (torch.full((c.nblocks, c.Hkv, 64, c.D), rx.SENTINEL, dtype=torch.float64), rx.rqc_model(c)[1],
                rx.rqc_items(c)[1], rx.CAP_RQC)
    if k == "sched":
        return c.f64("lat"), rx.sched_want(c)[0], torch.arange(c.n) // 8, rx.CAP
    raise ValueError(k)


@pytest.mark.parametrize("name", rx.BIG)
def test_second_trip_skipped_fails(name):
    """A grid-stride loop that never takes its second trip leaves items cap .. 2 cap - 1 as they were: the exact rule
    fails on every big case (for rope_qkv_cache: its k cache)."""
    c = rx.make_grid(name)
    before, want, item, cap = _trip_setup(c)
    mutant = rx.trip_mutant(before, want, item, cap, "skip_second_trip")
    with pytest.raises(AssertionError, match="differ"):
        rx.assert_full_exact(mutant.float().to(BF16), want.float().to(BF16), want.numel(), name)
    ok = _old_close(mutant, want)
    _tally("grid-stride", ok)
    print(f"{name}: second trip skipped, close() bad share {ge.close_bad_share(mutant, want):.3f}"
          f"{' -- accepted' if ok else ''}")


def test_loop_step_griddim_fails():
    """A loop step of gridDim.x (not gridDim.x * blockDim.x) visits every item again and again: out-of-place kernels
    still give the right answer, the in-place sched_step adds dt * v once per visit."""
    c = rx.make_grid("sched_big")
    want = rx.sched_want(c)[0]
    mutant = rx.sched_step_mutant(c, "step_griddim")
    with pytest.raises(AssertionError, match="differ"):
        rx.assert_full_exact(mutant.float().to(BF16), want.float().to(BF16), c.n, c.name)
    _tally("grid-stride", _old_close(mutant, want))


ROPE_MUTANTS = [("rope_small_pairs", "neox_for_pairs"), ("rope_small_pairs_half", "neox_for_pairs"),
                ("rope_small_neox_half", "cos_stride"), ("rope_small_pairs_half", "cos_stride"),
                ("rope_small_pairs_half", "past_rot"), ("rope_small_neox", "tok_stride"),
                ("rope_small_pairs_half", "tok_stride"), ("rope_big", "tok_stride")]


@pytest.mark.parametrize("name,mut", ROPE_MUTANTS)
def test_rope_mutant_fails(name, mut):
    c = rx.make_grid(name)
    want = rx.rope_model(c)
    mutant = rx.rope_model(c, mut)
    with pytest.raises(AssertionError, match="differ"):
        rx.assert_full_exact(mutant.float().to(BF16), rx.to_bf16_exact(want), c.T * c.H * c.rot, name)
    idx = c.idx["x"]
    _tally("rope", _old_close(mutant[idx], want[idx]))


KV_MUTANTS = [("kvw_small", "slot_neg_written"), ("kvw_small", "block_offset_confused"),
              ("kvw_big", "slot_neg_written"), ("rqc_small_64", "slot_neg_written"),
              ("rqc_small_128", "block_offset_confused"),
              ("rqc_small_64", "k_unrotated"), ("rqc_small_128", "k_unrotated"),
              ("rqc_small_64", "v_second8_dropped"), ("rqc_small_128", "v_second8_dropped")]


@pytest.mark.parametrize("name,mut", KV_MUTANTS)
def test_kv_mutant_fails(name, mut):
    c = rx.make_grid(name)
    if c.kind == "kvw":
        want, mutant = torch.stack(rx.kvw_want(c)), torch.stack(rx.kvw_want(c, mut))
    else:
        want, mutant = torch.stack(rx.rqc_model(c)[1:]), torch.stack(rx.rqc_model(c, mut)[1:])
    with pytest.raises(AssertionError, match="differ"):
        rx.assert_full_exact(mutant.float().to(BF16), want.float().to(BF16), want != rx.SENTINEL, name)
    _tally("kv", _old_close(mutant, want))


def test_canary_and_poison_mutants():
    """One element written behind the view, and one poison element changed in an in-place buffer, are both caught."""
    c = rx.make_rownorm("rms_D320_r5_random")
    out, _ = rx.rownorm_model(c)
    idx = rx.rownorm_out(c)[1]
    hit = out.clone()
    hit[1 + c.rows, 0] = 3.0
    with pytest.raises(AssertionError, match="canary overwritten"):
        rx.check_rownorm(c, hit, idx)
    c = rx.make_grid("rope_small_neox")
    want = rx.to_bf16_exact(rx.rope_model(c))
    written = rx.rope_model(c, items=True) >= 0
    hit = want.clone()
    hit[0, 5] = 3.0
    with pytest.raises(AssertionError, match="canary overwritten"):
        rx.assert_full_exact(hit, want, written, c.name)
    hit = want.clone()
    hit[1, c.H * c.Dh + 3] = 3.0      # a k column of the packed row
    with pytest.raises(AssertionError, match="canary overwritten"):
        rx.assert_full_exact(hit, want, written, c.name)


# ----------------------------------------------------------------------------- 3. layout
def test_operands_alias_their_poison_buffers():
    cases = [rx.make_rownorm(n) for n in list(rx.ROWNORM_CASES)[::23]] + [rx.make_qknr(n) for n in rx.QKNR_CASES]
    cases += [rx.make_gn(n) for n in list(rx.GN_CASES)[::5]] + [rx.make_grid(n) for n in rx.GRID_CASES if "_small" in n]
    for c in cases:
        assert c.poison_count() > 0, c.name
        for key, buf in c.bufs.items():
            v = c.view(key)
            assert v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
            assert v.numel() < buf.numel() and v.data_ptr() % 16 == 0, (c.name, key)
            if c.kind == "rownorm" and c.mod and key in ("w", "b"):
                continue      # scale and shift are chunks of one tensor: each is the other's neighbour
            mask = torch.ones(buf.shape, dtype=torch.bool)
            mask[c.idx[key]] = False
            assert bool((buf.float()[mask].abs() == rx.POISON).all()), (c.name, key)
    for c in cases:
        if c.kind == "rownorm":
            buf, idx = rx.rownorm_out(c)
            assert int((buf == rx.SENTINEL).sum()) == buf.numel() and buf[idx].data_ptr() % 16 == 0
            assert buf[idx].is_contiguous() == (c.layout != "cols")


def test_zz_old_rules_accept():
    """How many mutant runs of this file the older rules accept (every one of them fails the new rules)."""
    for fam, (n, a) in sorted(ACCEPTED.items()):
        print(f"{fam}: {a} of {n} mutant runs accepted by the old rule")
    if ACCEPTED:
        assert sum(a for _, a in ACCEPTED.values()) > 0
