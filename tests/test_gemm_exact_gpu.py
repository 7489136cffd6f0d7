"""GEMM and conv kernels against bf16(fp64 result) with ZERO tolerance, every element compared (tests/gemm_exact.py).

The operands are small integers, alpha / res_alpha dyadic, and every partial sum stays below 2^24: each fp32 operation
of the kernels is exact in any accumulation order, so after the one rounding to bf16 the output must equal the oracle
bit for bit -- whatever the tile shape, split-K count or MFMA order.  A wrong row, a column quad that lost its bias, a
pad tap that wrapped to the previous row or image, a partial that counted rows past M: each is a failure here, while
the suite's averaged rules (relative Frobenius error, close()) accept them (tests/test_gemm_exact_cpu.py shows both).
Every operand lies in a poison buffer, every GEMM output in a buffer of canaries.

Forced configs: v2 tiles 0-4, v4 9 / 10 (persistent 11 / 12), four-wave 13, W-stationary 15; split-K as 3000 + cfg +
100 * splits; the skinny kernels 1000 / 1100 / 1200 / 1250 + kg.  The conv cases run in child processes
(tests/gemm_exact_worker.py): SHAI_GEMM_FORCE / SHAI_GEMM_FORCE_SPLITS are read once per process.
"""
import os
import re
import subprocess
import sys

import pytest
import torch

import gemm_exact as ge
import shai_amd.ops as ops

pytestmark = pytest.mark.gpu
TILE = [0, 1, 2, 3, 4, 9, 10, 11, 12, 13]
SPLITTABLE = [0, 1, 2, 3, 4, 9, 10, 11, 12]
V4 = [9, 10, 11, 12]
WS = 15
_want = {}


def want(name, act=None):
    """(case, bf16 expected output on the GPU, fp64 result, |z|): computed once per (case, activation), shared."""
    if (name, act) not in _want:
        c = ge.make_gemm(name)
        w, y64, zabs = ge.gemm_want(c, act)
        _want[(name, act)] = (c, w.cuda(), y64, zabs)
    return _want[(name, act)]


def run_into(name, force, act=None, ldcs=None, smooth=False):
    """The case through ops.gemm_into at every output layout of the case: exact rule (or the smooth rule) on the
    view, the canaries around it untouched."""
    c, w, y64, zabs = want(name, act)
    d = c.place("cuda")
    if c.mx:
        d["w"] = c.wq.cuda()
    for ldc in ldcs or c.ldcs:
        buf, out, _ = ge.out_buffer(c, ldc, "cuda")
        ops.gemm_into(d["x"], d["w"], out, d.get("bias"), act=act, residual=out if c.res_inplace else d.get("residual"),
                      gate=d.get("gate"), rows_per_gate=c.rows_per_gate or 1, alpha=c.alpha, res_alpha=c.res_alpha,
                      glu=c.glu, force_cfg=force, w_scale=None if c.w_scale is None else c.w_scale.cuda())
        what = f"{name} force_cfg {force} act {act} ldc {ldc}"
        if smooth:
            ge.assert_smooth(out, y64, zabs, what)
            ge.assert_canaries(buf, ge.full_want(c, out.cpu(), ldc), what)
        else:
            ge.assert_exact(out, w, what)
            ge.assert_canaries(buf, ge.full_want(c, w.cpu(), ldc), what)
    ge.TOTALS["poison"] += c.poison_count()


def forced(cfg, splits):
    return cfg if splits == 1 else 3000 + cfg + 100 * splits


@pytest.mark.parametrize("cfg,splits", [(c, 1) for c in TILE] + [(c, s) for c in SPLITTABLE for s in (2, 3)])
def test_tails(cuda, cfg, splits):
    """(300, 328, 136): M tail, N tail on the wide store path, last K-tile of 8; bias + residual in place + alpha 0.5,
    res_alpha 2; unsplit, and split-K 2 / 3 on every splittable config (the four-wave kernel runs the whole K)."""
    run_into("tails", forced(cfg, splits))


@pytest.mark.parametrize("cfg", TILE)
def test_narrow_store(cuda, cfg):
    """(257, 322, 72): one row past a tile, N not a multiple of 4, own residual (ldr != ldc)."""
    run_into("narrow_store", cfg)


@pytest.mark.parametrize("cfg", TILE)
def test_many_tiles(cuda, cfg):
    """(65836, 72, 64): 258 row tiles, the last with 44 rows."""
    run_into("many_tiles", cfg)


@pytest.mark.parametrize("cfg", TILE)
def test_gate_batched(cuda, cfg):
    """B 3 x (300, 384, 256) strided 3-D views, rows_per_gate 150, output in a row-offset slice."""
    run_into("gate_batched", cfg)


@pytest.mark.parametrize("cfg", TILE + [WS])
def test_relu(cuda, cfg):
    """``tails`` with ReLU (exact) on every config that instantiates it; one that does not raises."""
    if cfg == WS:
        with pytest.raises(RuntimeError, match="bad force_cfg"):
            run_into("tails", cfg, act="relu", ldcs=[328])
        with pytest.raises(RuntimeError, match="bad force_cfg"):
            run_into("ws_bias", cfg, act="relu", ldcs=[640])
        return
    run_into("tails", cfg, act="relu")


@pytest.mark.parametrize("name", ["ws_plain", "ws_bias", "ws_residual"])
def test_ws(cuda, name):
    """W-stationary kernel (cfg 15) at (300, 640, 320): plain, bias (alpha 2), bias + residual in place."""
    run_into(name, WS)


@pytest.mark.parametrize("kind", [1000, 1100, 1200, 1250])
@pytest.mark.parametrize("M", ge.SKINNY_M)
def test_skinny(cuda, M, kind):
    """Skinny kernels at M 1 / 33 / 64, N 328, K 1096: separate fold, in-launch fixup, the wide kernel and its
    6-stage form, 1 and 3 K groups."""
    for kg in (1, 3):
        run_into(f"skinny_{M}", kind + kg)


@pytest.mark.parametrize("kind", [1000, 1100])
@pytest.mark.parametrize("M", ge.SKINNY_M)
def test_skinny_fp8(cuda, M, kind):
    """The fp8-weight skinny path on a hand-built exact pair (integer-valued e4m3 codes, w_scale 2^-k per row)."""
    for kg in (1, 3):
        run_into(f"skinny8_{M}", kind + kg)


@pytest.mark.parametrize("kind", [1000, 1100])
def test_fp4_skinny(cuda, kind):
    """MXFP4 skinny kernel at M 33, N 328, K 1088, on a weight that quantize_mxfp4 round-trips exactly."""
    for kg in (1, 3):
        run_into("fp4_skinny_33", kind + kg)


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("splits", [1, 3])
def test_fp4_tile(cuda, tile, splits):
    """MXFP4 tile GEMM at (300, 328, 256), both tiles, unsplit and split-K 3: bias + residual, alpha 0.5 / 2."""
    run_into("fp4_tile", 1300 + 32 * tile + splits)


def _stats_forces():
    return [(cfg, 1) for cfg in TILE] + [(cfg, 3) for cfg in SPLITTABLE]


@pytest.mark.parametrize("name", ge.PARTIALS_CASES)
@pytest.mark.parametrize("stats", ["gn", "ln"])
def test_stats(cuda, name, stats):
    """linear_stats on every tile config, unsplit and split-K 3 (the fold writes the partials): the output exact, the
    GroupNorm partials exactly the fp64 sums (rows past M contribute nothing), the LayerNorm (mean, rstd) within rtol
    1e-5 of fp64 (about ten fp32 operations on exact sums; rows have variance >= 1, nothing cancels)."""
    c, w, y64, _ = want(name)
    d = c.place("cuda")
    gp64, mr64 = ge.col_partials64(y64), ge.row_moments64(y64, 1e-5)
    for cfg, splits in _stats_forces():
        y, st = ops.linear_stats(d["x"], d["w"], d["bias"], d["residual"], stats=stats, eps=1e-5,
                                 force_cfg=forced(cfg, splits))
        what = f"{name} {stats} cfg {cfg} splits {splits}"
        ge.assert_exact(y, w, what)
        if stats == "gn":
            ge.assert_exact(st.double().cpu(), gp64, what + " partials")
        else:
            got = st.double().cpu()
            err = ((got - mr64).abs() / mr64.abs().clamp_min(1e-300)).max().item()
            print(f"{what}: worst relative error of (mean, rstd) {err:.2e}")
            torch.testing.assert_close(got, mr64, rtol=1e-5, atol=0.0)
            ge.TOTALS["compared"] += got.numel()
    ge.TOTALS["poison"] += c.poison_count()


@pytest.mark.parametrize("name,cfgs", [("res_rows", V4 + [WS]), ("res_rows_64", [WS])])
def test_res_rows(cuda, name, cfgs):
    """Broadcast residual, M 512: 256 residual rows on v4 and the W-stationary kernel, 64 rows on the latter."""
    c, w, _, _ = want(name)
    d = c.place("cuda")
    for cfg in cfgs:
        y = ops.linear(d["x"], d["w"], d["bias"], residual=d["residual"], res_alpha=c.res_alpha,
                       residual_rows=c.residual_rows, force_cfg=cfg)
        ge.assert_exact(y, w, f"{name} cfg {cfg}")
    ge.TOTALS["poison"] += c.poison_count()


@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("cfg", TILE)
def test_smooth_tails(cuda, cfg, act):
    """``tails`` with SiLU / GELU: |y - y64| <= ulp_bf16(y64) + 1e-6 |z|, every element."""
    run_into("tails", cfg, act=act, ldcs=[328, 333], smooth=True)


@pytest.mark.parametrize("cfg", TILE)
def test_glu_tails(cuda, cfg):
    """The GLU pair layout at (300, 2 * 164, 136) with SiLU, by the smooth rule (z = value * gate pre-activation)."""
    run_into("glu_tails", cfg, act="silu", smooth=True)


@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_glu_ws(cuda, act):
    """The GLU pair layout at (300, 640, 320) on the W-stationary kernel."""
    run_into("glu_ws", WS, act=act, smooth=True)


# ----------------------------------------------------------------------------- halo conv (in process)
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("name", list(ge.HALO_CASES))
def test_halo_conv(cuda, name, waves):
    """Halo-tiled conv under set_halo_conv(2) with 4 and 8 waves: (2, 16, 16, 64 -> 128) with temb + residual +
    GroupNorm partials, (1, 32, 32, 64 + 64 -> 160).  (Mode 1 with the integer norm is not run: conv_halo_supported
    takes a normalised input only with SiLU, which is not exact.)"""
    prev = ops.set_halo_conv(-1, -1)
    try:
        ops.set_halo_conv(2, waves)
        c = ge.make_conv(name)
        y, gp = ge.run_conv(c, ops)
        ge.check_conv(c, y, gp, f"halo waves {waves}")
    finally:
        ops.set_halo_conv(prev, 0)


# ----------------------------------------------------------------------------- conv and weight-slice cases (children)
CONV_FORCES = [(cfg, sp) for cfg in V4 for sp in (1, 3, 4)] + [(13, 1)]


@pytest.mark.parametrize("cfg,splits", CONV_FORCES)
def test_conv_forced(cuda, cfg, splits):
    """Every conv case of gemm_exact.CONV_CASES (and ``bias2d_slices`` through linear_wslices) inside one child per
    forced (config, split-K count); a child that faults or fails ends the test."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_exact_worker.py")
    env = dict(os.environ, SHAI_GEMM_FORCE=str(cfg), SHAI_GEMM_FORCE_SPLITS=str(splits))
    r = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
    sys.stdout.write(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"TOTALS compared (\d+) canaries (\d+) poison (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    for key, v in zip(("compared", "canaries", "poison"), m.groups()):
        ge.TOTALS[key] += int(v)


def test_zz_totals(cuda):
    """What this file's checks looked at in this process (and its children): printed for the record."""
    print("TOTALS compared {compared} canaries {canaries} poison {poison}".format(**ge.TOTALS))
    assert ge.TOTALS["compared"] > 0
