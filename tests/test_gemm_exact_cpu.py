"""The bit-exact GEMM / conv tests, tested (no GPU): every committed case of tests/gemm_exact.py meets the exactness
preconditions (so the zero tolerance is derived, not tuned), every addressing mutant of an explicit-index model fails
the exact rule, the poison / canary layout really surrounds the operands -- and the suite's older rules (relative
Frobenius error, close()) accept the mutants listed in TABLE, which is why tests/gemm_exact.py exists."""
import pytest
import torch

import gemm_exact as ge
from shai_amd.ops import reference as ref

ALL_CONV = list(ge.CONV_CASES) + list(ge.HALO_CASES)
FROB = {"gemm": 1e-2, "conv": 2e-2}   # the suite's relative Frobenius thresholds


# ----------------------------------------------------------------------------- 1. preconditions
@pytest.mark.parametrize("name", list(ge.GEMM_CASES))
def test_gemm_case_is_exact(name):
    """Magnitude bound < 2^24; the fp32 reference equals the fp64 oracle bit for bit; |y| <= 256 where partials are
    taken; at least half of the outputs non-zero."""
    c = ge.make_gemm(name)
    bound = ge.gemm_bound(c)
    assert bound < ge.LIMIT
    acts = [None] if (c.slices or c.glu) else [None, "relu"]
    if c.glu:
        acts = ["relu"]   # the GLU layout's exact activation (there is no GLU without one)
    for act in acts:
        want, y64, _ = ge.gemm_want(c, act)
        x, w = c.view("x"), c.view("w")
        if c.fp8:
            w = (w.float() * c.w_scale[:, None]).to(ge.BF16)
            assert torch.equal(w.float(), c.w_int)   # the hand-built fp8 pair decodes to the integers exactly
        if c.mx:   # quantize_mxfp4 round-trips a weight drawn from the e2m1 grid times a power of two
            assert torch.equal(ref.dequant_mxfp4(c.wq, c.w_scale, torch.float32), w.float())
        if c.slices:
            got = torch.einsum("smk,snk->smn", x.float().view(c.slices, -1, c.K), w.float())
            got = (got + c.view("bias2d").float()[:, None]).reshape(c.M, c.N).to(ge.BF16)
        elif c.rows_per_gate or c.res_inplace:
            out = c.view("residual").clone() if c.res_inplace else torch.empty(*want.shape, dtype=ge.BF16)
            got = ref.gemm_into(x, w, out, c.view("bias"), act, out if c.res_inplace else c.view("residual"),
                                c.view("gate"), c.rows_per_gate or 1, c.alpha, c.res_alpha, c.glu)
        else:
            got = ref.linear(x, w, c.view("bias"), act, c.view("residual"), c.glu, c.alpha, c.res_alpha,
                             residual_rows=c.residual_rows)
        ge.assert_exact(got, want, f"{name} fp32 reference, act {act}")
    plain = ge.gemm_finish64(c, ge.gemm_z64(c))   # (ReLU zeroes half by design: the plain epilogue's share)
    assert float((plain != 0).double().mean()) >= 0.5
    if name in ge.PARTIALS_CASES:
        y64 = ge.gemm_want(c)[1]
        assert float(y64.abs().max()) <= 256
        # fp32 partials of the bf16 output are the fp64 ones, and rows have variance >= 1 (the LayerNorm moments)
        assert torch.equal(ref.col_partials(ge.to_bf16_exact(y64)).double(), ge.col_partials64(y64))
        assert float(y64.var(-1, unbiased=False).min()) >= 1.0
    print(f"{name}: magnitude bound {bound:.0f}")


@pytest.mark.parametrize("name", ALL_CONV)
def test_conv_case_is_exact(name):
    c = ge.make_conv(name)
    bound = float(ge.conv_y64(c, absolute=True).max())
    assert bound < ge.LIMIT
    y64 = ge.conv_y64(c)
    want = ge.to_bf16_exact(y64)
    norm = None
    if c.has("norm"):
        norm = (c.view("norm")[0], c.view("norm")[1], None)
    got = ref.conv2d(c.view("x"), c.view("w"), c.view("bias"), c.k, c.k, c.stride, c.pad, upsample=c.up,
                     x2=c.view("x2"), norm=norm, temb=c.view("temb"), residual=c.view("residual"))
    ge.assert_exact(got, want, f"{name} ref.conv2d")
    if c.kind == "up2":
        wp = ref.pack_up2_phase_weight(c.view("w"), c.C)
        # phase weights are sums of at most 4 integer taps: exact in bf16
        assert float(wp.float().abs().max()) <= 8 and torch.equal(wp.float(), wp.float().round())
        got = ref.conv2d_up2_phases(c.view("x"), wp, c.view("bias"), c.view("temb"))
        ge.assert_exact(got, want, f"{name} ref.conv2d_up2_phases")
        ge.assert_exact(ge.to_bf16_exact(ge.conv_finish64(c, ge.phase_model(c))), want, f"{name} phase model")
    if name != "walk":   # (the model of the 272-tile case is built per image where a mutant needs it)
        ge.assert_exact(ge.to_bf16_exact(ge.conv_finish64(c, ge.conv_model(c))), want, f"{name} index model")
    if c.gn:
        assert float(y64.abs().max()) <= 256
        assert torch.equal(ref.col_partials(want.reshape(-1, c.Co)).double(), ge.col_partials64(y64.reshape(-1, c.Co)))
    assert float((y64 != 0).double().mean()) >= 0.5
    print(f"{name}: magnitude bound {bound:.0f}")


def test_smooth_rule_accepts_fp32_and_rejects_a_bf16_intermediate():
    """The smooth rule on the SiLU / GELU cases: an fp32 evaluation passes; an activation rounded to bf16 before the
    residual is added (one rounding too many) does not."""
    c = ge.make_gemm("tails")
    for act in ("silu", "gelu"):
        _, y64, zabs = ge.gemm_want(c, act)
        z = ge.gemm_z64(c).float()
        r = c.view("residual").float()
        f = torch.nn.functional.silu if act == "silu" else torch.nn.functional.gelu
        ge.assert_smooth((f(z) + c.res_alpha * r).to(ge.BF16), y64, zabs, act)
        with pytest.raises(AssertionError, match="differ"):
            ge.assert_smooth((f(z).to(ge.BF16).float() + c.res_alpha * r).to(ge.BF16), y64, zabs, act)


# ----------------------------------------------------------------------------- 2. mutants
def _scores(kind, mutant, want, table):
    """The mutant must fail the exact rule; prints its scores under the suite's rules; a TABLE mutant must pass them."""
    with pytest.raises(AssertionError, match="differ"):
        ge.assert_exact(mutant, want, "mutant")
    fro, bad = ge.frobenius(mutant, want), ge.close_bad_share(mutant, want)
    n = int((mutant.double() != want.double()).sum())
    print(f"  {n} wrong elements: rel Frobenius {fro:.2e} (suite: < {FROB[kind]:g}), close() bad share {bad:.2e} "
          f"(suite: < 1e-3){' -- accepted by the suite' if table else ''}")
    if table == "both":
        assert fro < FROB[kind] and bad < 1e-3
    elif table == "frobenius":
        assert fro < FROB[kind]


def _gemm_mutant(c, mut):
    x, w, bias = c.f64("x"), ge.gemm_weight64(c), c.f64("bias")
    z = ge.gemm_z64(c)
    kw = {}
    if mut in ("k_tail_last_row", "k_tail_last_tile"):      # the last K-tile's 8 columns dropped
        rows = slice(c.M - 1, c.M) if mut == "k_tail_last_row" else slice((c.M - 1) // 256 * 256, c.M)
        z[rows] = c.alpha * x[rows, :c.K - 8] @ w[:, :c.K - 8].t() + bias
    elif mut == "dup_last_row":
        pass
    elif mut == "bias_lost_last2":
        z[:, -2:] -= bias[-2:]
    elif mut == "bias_late_quad":                           # the last column quad reads the bias one column late
        q = (c.N - 1) // 4 * 4
        start = c.idx["bias"][0].start
        late = c.bufs["bias"].double()[start + q + 1:start + c.N + 1]   # its last element is poison
        z[:, q:] += late - bias[q:]
    elif mut == "gate_local_m":
        kw["gate_rows"] = (torch.arange(c.M) // c.rows_per_gate).repeat(c.B)
    elif mut == "res_ldc":                                  # the residual's rows strided by ldc (= N) instead of ldr
        buf = c.bufs["residual"].double()
        ldr = buf.shape[-1]
        flat = buf.flatten()
        m, n = torch.arange(c.M)[:, None], torch.arange(c.No)[None, :]
        kw["residual"] = flat[ldr + m * c.No + n]
    y = ge.gemm_finish64(c, z, **kw)
    if mut == "dup_last_row":
        y[-1] = y[-2]
    return y.float().to(ge.BF16)


GEMM_MUTANTS = [("many_tiles", "k_tail_last_row", "both"), ("many_tiles", "dup_last_row", "both"),
                ("tails", "bias_lost_last2", "frobenius"), ("tails", "k_tail_last_tile", None),
                ("tails", "bias_late_quad", None), ("narrow_store", "res_ldc", None),
                ("gate_batched", "gate_local_m", None)]


@pytest.mark.parametrize("name,mut,table", GEMM_MUTANTS)
def test_gemm_mutant_fails_the_exact_rule(name, mut, table):
    c = ge.make_gemm(name)
    print(f"{name} / {mut}:")
    _scores("gemm", _gemm_mutant(c, mut), ge.gemm_want(c)[0], table)


def test_partials_mutant_rows_past_m():
    """Rows 384..511 of the second 256-row tile (the poison rows behind x) added to the last block's partials."""
    c = ge.make_gemm("stats_half_tile")
    y64 = ge.gemm_want(c)[1]
    want = ge.col_partials64(y64)
    past = c.bufs["x"].double()[c.M:c.M + 128, :c.K] @ c.f64("w").t()
    mutant = want.clone()
    mutant[-1, :, 0] += past.sum(0)
    mutant[-1, :, 1] += (past * past).sum(0)
    with pytest.raises(AssertionError, match="differ"):
        ge.assert_exact(mutant, want, "partials")


CONV_MUTANTS = [("walk", "corner_leak", "both"), ("walk", "left_wrap", "frobenius"),
                ("image_edges", "corner_leak", "frobenius"), ("image_edges", "left_wrap", None),
                ("image_edges", "top_prev_image", None), ("image_edges", "taps_transposed", None),
                ("concat_unequal", "concat_off8", None), ("up_nine_taps", "upsample_src", None),
                ("stride2", "stride_origin", None), ("norm_prologue", "norm_pad", None),
                ("halo_plain", "top_prev_image", None), ("halo_concat", "concat_off8", None)]


@pytest.mark.parametrize("name,mut,table", CONV_MUTANTS)
def test_conv_mutant_fails_the_exact_rule(name, mut, table):
    c = ge.make_conv(name)
    print(f"{name} / {mut}:")
    y64 = ge.conv_y64(c)
    if name == "walk":   # both mutants touch image 0 only
        m64 = y64.clone()
        part = ge.conv_model(c, mut, images=[0])
        for n_ in ("bias",):
            part = part + c.f64(n_)
        m64[0] = part[0]
    else:
        m64 = ge.conv_finish64(c, ge.conv_model(c, mut))
    _scores("conv", m64.float().to(ge.BF16), ge.to_bf16_exact(y64), table)


@pytest.mark.parametrize("name", ["phase_groups", "phase_temb"])
def test_phase_swap_mutant(name):
    c = ge.make_conv(name)
    print(f"{name} / phase px <-> py:")
    m64 = ge.conv_finish64(c, ge.phase_model(c, swap=True))
    _scores("conv", m64.float().to(ge.BF16), ge.to_bf16_exact(ge.conv_y64(c)), None)


def test_canary_mutant():
    """One element written past column N (the fourth lane of a 16-byte store at the ragged last quad)."""
    c = ge.make_gemm("narrow_store")
    want = ge.gemm_want(c)[0]
    for ldc in c.ldcs[1:]:
        full = ge.full_want(c, want, ldc)
        ge.assert_canaries(full.clone(), full, "clean")
        hit = full.clone()
        hit[8 + c.M - 1, c.No] = 3.0
        with pytest.raises(AssertionError, match="canary overwritten"):
            ge.assert_canaries(hit, full, "mutant")
        hit = full.clone()
        hit[7, 0] = 3.0     # the row above the view
        with pytest.raises(AssertionError, match="canary overwritten"):
            ge.assert_canaries(hit, full, "mutant")


# ----------------------------------------------------------------------------- 3. layout
@pytest.mark.parametrize("name", list(ge.GEMM_CASES) + ALL_CONV)
def test_operands_alias_their_poison_buffers(name):
    c = ge.make_gemm(name) if name in ge.GEMM_CASES else ge.make_conv(name)
    assert c.poison_count() > 0
    for key, buf in c.bufs.items():
        v = c.view(key)
        assert v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        if key == "norm":
            continue   # the kernels take scale / shift as one whole allocation
        assert v.numel() < buf.numel(), key
        mask = torch.ones(buf.shape, dtype=torch.bool)
        mask[c.idx[key]] = False
        lim = ge.POISON_F8 if c.dtype[key] == ge.F8 else ge.POISON
        assert bool((buf.float()[mask].abs() == lim).all()), key           # all around: poison
        assert float(v.float().abs().max()) <= 16, key                     # inside: the small numbers
        assert v.data_ptr() % 16 == 0, key
    if c.kind == "gemm":
        assert c.view("x").stride(-2) > c.K and c.view("x").stride(-2) % 8 == 0
        if not c.slices:
            assert c.view("w").stride(-2) > c.K and c.view("w").stride(-2) % (16 if c.fp8 else 8) == 0
        for ldc in c.ldcs:
            buf, view, _ = ge.out_buffer(c, ldc, "cpu")
            assert view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() and view.data_ptr() % 16 == 0
            assert int((buf == ge.SENTINEL).sum()) >= buf.numel() - view.numel() > 0
        if name in ("tails", "narrow_store", "glu_tails") or name.startswith("skinny"):
            assert any(ldc % 4 for ldc in c.ldcs)   # the narrow store path runs
