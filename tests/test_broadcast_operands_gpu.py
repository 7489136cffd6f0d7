"""Broadcast operands read in place by the kernels (GemmArgs::res_rows, AttnArgs::q_batch_mod) against the same
kernel on the operand materialised by ``repeat`` with the field cleared.  The arithmetic is identical, so every
comparison is bit-equal (torch.equal), statistics written by the epilogue included.

* v4 GEMM (gemm_8ph.hip; configs 9 = 256 x 256, 10 = 256 x 320, 11 / 12 their persistent forms), unsplit and with 3
  K splits (the fold, gemm_splitk_reduce): M = 1024 over 512 residual rows and M = 768 over 256 (an odd number of
  wraps; M not a multiple of 512), N = 320 (an N tail on the 256-wide configs: the narrow epilogue), K = 128 + 64.
  The contract (res_rows a multiple of 256 that divides M) leaves no partial M tile.
* the same shapes as a 1x1 two-source conv (128 + 64 channels): SHAI_GEMM_FORCE / SHAI_GEMM_FORCE_SPLITS are read once
  per process, so each (config, splits) pair runs this file as a child.  Split 3 on the persistent configs is the
  launch of 9 / 10 (a split launch is never persistent) and is not repeated.
* W-stationary kernel (gemm_ws.hip): the LayerNorm-out form at M = 512 over 256 rows and M = 192 over 96 (both outputs),
  and the plain residual form over 96 rows through the dispatcher (only this kernel takes a 96-row wrap).
* cross-attention with shared queries on flash64_dma (B = 4 over 2 and over 1 query batches, Sq = 200, Skv = 77) and on
  flash64x2 (the router's choice from 1024 workgroups of 256 queries and 512 keys).
* bias2d as a column slice of a wider matrix (GemmArgs::bias2d_ld) against its contiguous copy, per kernel family.
* problems no kernel takes in place (a 100-row wrap, D = 128 attention) are expanded by the binding: same results.
* every other kernel family refuses the fields in its *_supported check.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1024, 512), (768, 256)]  # (M, res_rows)
N, K1, K2 = 320, 128, 64


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(torch.bfloat16)


def same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: {(a.float() - b.float()).abs().max().item():.3e} apart"


@pytest.mark.parametrize("stats", ["gn", "ln"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("cfg", [9, 10, 11, 12])
@pytest.mark.parametrize("M,rr", SHAPES)
def test_v4_gemm_res_rows(cuda, M, rr, cfg, splits, stats):
    from shai_amd import ops
    torch.manual_seed(0)
    x, w, b, r = rnd(M, K1 + K2), rnd(N, K1 + K2, scale=0.05), rnd(N), rnd(rr, N)
    force = cfg if splits == 1 else 3000 + 100 * splits + cfg
    y1, s1 = ops.linear_stats(x, w, b, residual=r, stats=stats, force_cfg=force, residual_rows=rr)
    y0, s0 = ops.linear_stats(x, w, b, residual=r.repeat(M // rr, 1), stats=stats, force_cfg=force)
    same(y1, y0, "output")
    same(s1, s0, "statistics")
    assert not torch.equal(y0[:rr], y0[rr:2 * rr])  # the wraps are not copies of each other


def _conv_case(M, rr):
    """1x1 conv over two sources, residual of rr pixels under M: (with the field, materialised) outputs + partials."""
    from shai_amd import ops
    torch.manual_seed(1)
    n = M // 256
    x, x2 = rnd(n, 16, 16, K1), rnd(n, 16, 16, K2)
    w, b, res = rnd(N, K1 + K2, scale=0.05), rnd(N), rnd(rr // 256, 16, 16, N)
    y1, p1 = ops.conv2d(x, w, b, 1, 1, x2=x2, residual=res, residual_rows=rr, stats="gn")
    y0, p0 = ops.conv2d(x, w, b, 1, 1, x2=x2, residual=res.repeat(M // rr, 1, 1, 1), stats="gn")
    return y1, p1, y0, p0


def _child():
    import shai_amd.native as native
    native.ops()
    for M, rr in SHAPES:
        y1, p1, y0, p0 = _conv_case(M, rr)
        ok = torch.equal(y1, y0) and torch.equal(p1, p0) and bool(torch.isfinite(y1.float()).all())
        print(f"conv M={M} res_rows={rr}: {'equal' if ok else 'FAIL'} (max |y| {y1.float().abs().max().item():.3f})")
    torch.cuda.synchronize()


@pytest.mark.parametrize("cfg,splits", [(9, 1), (10, 1), (11, 1), (12, 1), (9, 3), (10, 3)])
def test_v4_conv_res_rows(cuda, cfg, splits):
    env = dict(os.environ, SHAI_GEMM_FORCE=str(cfg), SHAI_GEMM_FORCE_SPLITS=str(splits))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": equal") == len(SHAPES) and "FAIL" not in r.stdout


@pytest.mark.parametrize("M,rr", [(512, 256), (192, 96)])
def test_ws_lnout_res_rows(cuda, M, rr):
    torch.manual_seed(2)
    x, w, b, r = rnd(M, 320), rnd(320, 320, scale=0.05), rnd(320), rnd(rr, 320)
    g, be = (1 + 0.1 * torch.randn(320, device="cuda")).bfloat16(), rnd(320, scale=0.1)
    outs = []
    for res, rows in ((r, rr), (r.repeat(M // rr, 1), 0)):
        y, y2 = torch.empty(M, 320, dtype=torch.bfloat16, device="cuda"), torch.empty(M, 320, dtype=torch.bfloat16,
                                                                                      device="cuda")
        assert torch.ops.shai.gemm_lnout(x, w, y, y2, b, res, 1.0, g, be, 1e-5, rows), "the fused kernel must run"
        outs.append((y, y2))
    same(outs[0][0], outs[1][0], "C")
    same(outs[0][1], outs[1][1], "C2")
    assert not torch.equal(outs[1][0][:rr], outs[1][0][rr:2 * rr])


def test_ws_residual_rows_through_dispatcher(cuda):
    """A 96-row wrap fits only the W-stationary kernel (32-row tiles): the dispatcher must land there, forced or not."""
    from shai_amd import ops
    torch.manual_seed(3)
    M, rr = 192, 96
    x, w, b, r = rnd(M, 320), rnd(320, 320, scale=0.05), rnd(320), rnd(rr, 320)
    want = ops.gemm_into(x, w, torch.empty(M, 320, dtype=torch.bfloat16, device="cuda"), b, residual=r.repeat(2, 1),
                         force_cfg=15)
    same(ops.linear(x, w, b, residual=r, residual_rows=rr, force_cfg=15), want, "forced W-stationary")
    same(ops.linear(x, w, b, residual=r, residual_rows=rr), want, "dispatched")
    with pytest.raises(RuntimeError):  # a v2 tile would read the residual past its end: refused, not run
        ops.linear(x, w, b, residual=r, residual_rows=rr, force_cfg=2)


@pytest.mark.parametrize("B,mod,H,Sq,Skv", [(4, 2, 2, 200, 77), (4, 1, 2, 200, 77), (128, 64, 8, 200, 512)],
                         ids=["dma-mod2", "dma-mod1", "x2"])
def test_attention_q_batch_mod(cuda, B, mod, H, Sq, Skv):
    from shai_amd import ops
    torch.manual_seed(4)
    q, k, v = rnd(mod, Sq, H, 64), rnd(B, Skv, H, 64), rnd(B, Skv, H, 64)
    o1 = ops.attention(q, k, v, q_batch_mod=mod)
    o0 = ops.attention(q.repeat(B // mod, 1, 1, 1), k, v)
    same(o1, o0, "attention output")
    assert not torch.equal(o0[0], o0[mod])  # different contexts


def test_unsupported_broadcasts_are_expanded(cuda):
    from shai_amd import ops
    torch.manual_seed(5)
    x, w, r = rnd(200, 64), rnd(48, 64, scale=0.1), rnd(100, 48)  # 100-row wrap: no kernel's tile
    same(ops.linear(x, w, residual=r, residual_rows=100), ops.linear(x, w, residual=r.repeat(2, 1)), "linear")
    q, k, v = rnd(2, 130, 2, 128), rnd(4, 77, 2, 128), rnd(4, 77, 2, 128)  # D = 128: kernels without q_batch_mod
    same(ops.attention(q, k, v, q_batch_mod=2), ops.attention(q.repeat(2, 1, 1, 1), k, v), "attention")


@pytest.mark.parametrize("path", ["v4", "v2-narrow", "halo", "phase", "unaligned"])
def test_bias2d_column_slice(cuda, path):
    """bias2d as a column slice of a wider matrix (GemmArgs::bias2d_ld: the time projections of all ResNets are the
    columns of one GEMM output) against its ``.contiguous()`` copy, on every kernel family that takes bias2d: the v4 wide
    epilogue, a v2 tile's narrow epilogue (8 input channels), the halo conv, the phase-decomposed upsample conv; and a
    view whose rows are not 16-byte aligned, which the ops copy first."""
    from shai_amd import ops
    torch.manual_seed(6)
    n, cout = 4, 320
    cin = 8 if path == "v2-narrow" else 320
    wide = rnd(n, 3 * cout + 8)
    t = wide[:, 4:4 + cout] if path == "unaligned" else wide[:, cout:2 * cout]
    assert not t.is_contiguous() and (t.data_ptr() % 16 == 0) == (path != "unaligned")
    x, res = rnd(n, 16, 16, cin), rnd(n, 16, 16, cout)
    w = ops.pack_conv_weight(torch.randn(cout, cin, 3, 3, device="cuda").mul(0.02).bfloat16())
    b = rnd(cout)
    kw = {}
    if path == "phase":
        kw, res = {"upsample": True, "w_up2": ops.pack_up2_phase_weight(w, cin)}, None
        assert ops.up2_phases_ok(x, 3, 3, 1, 1, temb=t)
    prev = ops.set_halo_conv(2) if path == "halo" else None
    try:
        y1, p1 = ops.conv2d(x, w, b, 3, 3, 1, 1, temb=t, residual=res, stats="gn", **kw)
        y0, p0 = ops.conv2d(x, w, b, 3, 3, 1, 1, temb=t.contiguous(), residual=res, stats="gn", **kw)
    finally:
        if prev is not None:
            ops.set_halo_conv(prev)
    same(y1, y0, "output")
    same(p1, p0, "GroupNorm partials")
    y2 = ops.conv2d(x, w, b, 3, 3, 1, 1, temb=wide[:, :cout].contiguous(), residual=res, **kw)
    assert not torch.equal(y1, y2)  # the slice's columns, not the matrix's first ones


def test_other_families_refuse(cuda):
    rows = dict(s.split("=") for s in torch.ops.shai.broadcast_refusals())
    assert set(rows) >= {"v2", "w4", "f8", "fp4", "skinny", "skinny2", "skinny_fp4", "halo", "flash2", "flash128x2",
                         "attn512", "v1"}
    for fam, v in rows.items():  # "1,0": takes the problem without the field, refuses it with the field set
        assert v == "1,0", f"{fam}: supported without / with the broadcast field = {v}"


if __name__ == "__main__" and "--child" in sys.argv:
    sys.path.insert(0, ROOT)
    _child()
