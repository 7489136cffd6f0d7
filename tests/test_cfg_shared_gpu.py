"""Classifier-free-guidance prefix sharing on the GPU kernels: one reduced-depth UNet forward with the full 320-wide
first level (so the folded proj_in, the LayerNorm-out out-projections, the merged proj_out and the broadcast-operand
kernels are the paths taken) at B = 2 (4 CFG rows), 64 x 64 latents -- shared (cfg_pairs=True) against unshared, eager
and under graph capture / replay.  Tolerance: that of tests/test_norm_handoff_gpu.py for two paths of one UNet."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.fixture(scope="module")
def setup(cuda):
    """(model, inputs, unshared output, calls seen in the shared forward), computed once for both tests."""
    from shai_amd import ops
    from shai_amd.models import unet2d
    from shai_amd.models.unet2d import UNet2DConditionModel, UNetConfig
    torch.manual_seed(21)
    cfg = UNetConfig(block_out_channels=(320, 640), layers_per_block=1, attention_heads=(5, 10),
                     cross_attention_dim=256, down_attn=(True, False), time_embed_dim=320)
    m = UNet2DConditionModel(cfg).cuda().eval()
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.03)
    lat = torch.randn(2, 64, 64, 4, device="cuda").bfloat16()
    x = torch.cat([lat, lat], 0)
    t = torch.tensor([500.0], device="cuda")
    kv = m.context_kv(torch.randn(4, 77, 256, device="cuda").bfloat16())  # cond / uncond contexts differ
    saved = (unet2d.NORM_HANDOFF, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS, ops.FOLD_MIN_TILES, ops.LNOUT)
    names = ("linear_wslices", "linear_lnout", "conv2d", "attention")
    orig = {n: getattr(ops, n) for n in names}
    calls = []

    def spy(name):
        def f(*a, **k):
            if name in ("linear_wslices", "linear_lnout") or k.get("residual_rows") or k.get("q_batch_mod"):
                calls.append((name, a[0].shape[0] if name != "linear_lnout" else a[0].numel() // a[0].shape[-1],
                              k.get("residual_rows", 0), k.get("q_batch_mod", 0)))
            return orig[name](*a, **k)
        return f

    unet2d.NORM_HANDOFF, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS = True, True, 0
    ops.FOLD_MIN_TILES, ops.LNOUT = 0, True  # the folded path at this batch too
    try:
        with torch.inference_mode():
            y0 = m(x, t, kv, cfg_pairs=False)
            for n in names:
                setattr(ops, n, spy(n))
            y1 = m(x, t, kv, cfg_pairs=True)
    finally:
        for n in names:
            setattr(ops, n, orig[n])
        unet2d.NORM_HANDOFF, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS, ops.FOLD_MIN_TILES, ops.LNOUT = saved
    return m, (x, t, kv), y0, y1, calls


def test_shared_matches_unshared(setup):
    m, _, y0, y1, calls = setup
    print("calls with broadcast operands / fused paths (name, rows, residual_rows, q_batch_mod):", calls)
    half = 2 * 64 * 64  # rows of one guidance half at the first level: whole 256-row tiles
    assert half % 256 == 0
    first = [c for c in calls if c[0] == "linear_wslices"][0]
    assert first[1] == half, "the first transformer's folded proj_in must run on half the rows"
    lnout = [c for c in calls if c[0] == "linear_lnout"]
    assert (lnout[0][1], lnout[0][2]) == (half, 0), "attn1.out + LayerNorm on half the rows"
    assert (lnout[1][1], lnout[1][2]) == (2 * half, half), "attn2.out reads the half-batch residual stream in place"
    assert ("attention", 2, 0, 2) in calls, "cross-attention with the queries of 2 images under 4 contexts"
    assert ("conv2d", 4, half, 0) in calls, "merged proj_out reads the half-batch block input in place"
    assert any(getattr(mod, "_po_merged", None) is not None for mod in m.modules()), "merged proj_out not taken"
    assert y1.shape == y0.shape == (4, 64, 64, 4) and torch.isfinite(y1.float()).all()
    assert rel(y0[:2], y0[2:]) > 1e-3, "the guidance halves must differ"
    r = rel(y1, y0)
    print(f"shared vs unshared UNet forward: rel {r:.3e}, max abs diff {(y1.float() - y0.float()).abs().max().item():.3e}")
    assert r < TOL


def test_shared_under_graph_capture(setup):
    m, (x, t, kv), y0, y1, _ = setup
    from shai_amd import ops
    from shai_amd.models import unet2d
    saved = (unet2d.NORM_HANDOFF, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS, ops.FOLD_MIN_TILES, ops.LNOUT)
    unet2d.NORM_HANDOFF, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS = True, True, 0
    ops.FOLD_MIN_TILES, ops.LNOUT = 0, True
    try:
        with torch.inference_mode():
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                m(x, t, kv, cfg_pairs=True)
            torch.cuda.current_stream().wait_stream(s)
            with torch.cuda.graph(g):
                yg = m(x, t, kv, cfg_pairs=True)
            yg.zero_()
            g.replay()
            torch.cuda.synchronize()
    finally:
        unet2d.NORM_HANDOFF, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS, ops.FOLD_MIN_TILES, ops.LNOUT = saved
    r = rel(yg, y0)
    print(f"graph replay of the shared forward vs eager unshared: rel {r:.3e}; vs eager shared: rel {rel(yg, y1):.3e}")
    assert torch.isfinite(yg.float()).all() and r < TOL
