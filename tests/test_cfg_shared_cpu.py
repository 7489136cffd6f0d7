"""Classifier-free-guidance prefix sharing (UNet2DConditionModel.forward(cfg_pairs=True)) on the reference ops: the
layers both guidance halves share run on half the rows and the output stays the full computation's; the broadcast
operands of the reference ops (residual_rows / q_batch_mod) are plain index arithmetic."""
import pytest
import torch

from shai_amd import ops
from shai_amd.ops import reference as ref

TOL = 1e-2  # tests/test_norm_handoff_cpu.py: the project's path-equivalence tolerance on the reference ops


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.fixture(scope="module")
def tiny_unet():
    from shai_amd.models.unet2d import UNet2DConditionModel, UNetConfig
    torch.manual_seed(11)
    cfg = UNetConfig.tiny()
    assert cfg.down_attn[0], "the tiny config's first down block must have attention (the sharing point)"
    m = UNet2DConditionModel(cfg).eval()
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.05)
    lat = torch.randn(2, 16, 16, 4).bfloat16()
    ctx = torch.randn(4, 77, cfg.cross_attention_dim).bfloat16()  # the two context halves differ
    assert rel(ctx[:2], ctx[2:]) > 0.5
    return m, lat, m.context_kv(ctx)


class _Paths:
    """Pin the model's path switches for one comparison and count the calls that carry a broadcast operand."""

    def __init__(self, handoff: bool, fold: bool):
        self.handoff, self.fold = handoff, fold
        self.calls = {"attention": 0, "residual": 0}

    def __enter__(self):
        from shai_amd.models import unet2d
        self.saved = (unet2d.NORM_HANDOFF, ops.FOLD_MIN_TILES, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS,
                      ref.attention, ref.linear, ref.conv2d)
        unet2d.NORM_HANDOFF, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS = self.handoff, True, 0
        if self.fold:
            ops.FOLD_MIN_TILES = 0
        att, lin, conv = ref.attention, ref.linear, ref.conv2d

        def attention(*a, **k):
            self.calls["attention"] += bool(k.get("q_batch_mod") or (len(a) > 9 and a[9]))
            return att(*a, **k)

        def linear(*a, **k):
            self.calls["residual"] += bool(k.get("residual_rows"))
            return lin(*a, **k)

        def conv2d(*a, **k):
            self.calls["residual"] += bool(k.get("residual_rows") or (len(a) > 14 and a[14]))
            return conv(*a, **k)

        ref.attention, ref.linear, ref.conv2d = attention, linear, conv2d
        return self

    def __exit__(self, *exc):
        from shai_amd.models import unet2d
        (unet2d.NORM_HANDOFF, ops.FOLD_MIN_TILES, unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS,
         ref.attention, ref.linear, ref.conv2d) = self.saved


@pytest.mark.parametrize("handoff,fold", [(True, True), (True, False), (False, False)],
                         ids=["folded", "handoff", "plain"])
def test_cfg_pairs_matches_full_batch(tiny_unet, handoff, fold):
    m, lat, kv = tiny_unet
    x = torch.cat([lat, lat], 0)
    t = torch.tensor([500.0])
    with _Paths(handoff, fold) as p:
        y0 = m(x, t, kv, cfg_pairs=False)
        assert p.calls == {"attention": 0, "residual": 0}
        y1 = m(x, t, kv, cfg_pairs=True)
        # the cross-attention with shared queries, its out-projection and the transformer's output projection
        assert p.calls == {"attention": 1, "residual": 2}, p.calls
    assert y1.shape == y0.shape == (4, 16, 16, 4)
    assert rel(y0[:2], y0[2:]) > 1e-3, "the guidance halves must differ (different contexts)"
    r = rel(y1, y0)
    print(f"cfg_pairs vs full batch ({'folded' if fold else 'handoff' if handoff else 'plain'}): rel {r:.3e}")
    assert r < TOL


def test_cfg_pairs_per_row_timesteps(tiny_unet):
    m, lat, kv = tiny_unet
    x = torch.cat([lat, lat], 0)
    t = torch.tensor([500.0, 120.0, 500.0, 120.0])  # rows i and B + i equal, as StepBatcher writes them
    with _Paths(True, True):
        assert rel(m(x, t, kv, cfg_pairs=True), m(x, t, kv, cfg_pairs=False)) < TOL


def test_flag_not_data_selects_the_path(tiny_unet):
    """Negative control: with halves that are NOT equal and cfg_pairs=False the output is the full computation (the
    second half follows its own latents); only the flag turns sharing on."""
    m, lat, kv = tiny_unet
    torch.manual_seed(12)
    other = torch.randn_like(lat.float()).bfloat16()
    x = torch.cat([lat, other], 0)
    t = torch.tensor([500.0])
    with _Paths(True, True) as p:
        y = m(x, t, kv, cfg_pairs=False)
        assert p.calls == {"attention": 0, "residual": 0}
        # row by row the full computation: each half alone, with its own context
        lo = m(x[:2], t, [k[:2] for k in kv], cfg_pairs=False)
        hi = m(x[2:], t, [k[2:] for k in kv], cfg_pairs=False)
        assert rel(y, torch.cat([lo, hi], 0)) < TOL
        # and the flag on the same unequal data does change the result: it is the flag that selects the path
        assert rel(m(x, t, kv, cfg_pairs=True)[2:], y[2:]) > 10 * TOL
        assert p.calls["attention"] == 1


def test_env_switch_restores_full_batch(tiny_unet):
    from shai_amd.models import unet2d
    m, lat, kv = tiny_unet
    x = torch.cat([lat, lat], 0)
    with _Paths(True, True) as p:
        unet2d.CFG_SHARED = False  # what SHAI_CFG_SHARED=0 sets
        m(x, torch.tensor([500.0]), kv, cfg_pairs=True)
        assert p.calls == {"attention": 0, "residual": 0}
        unet2d.CFG_SHARED, unet2d.CFG_SHARED_MIN_ROWS = True, 2 * 16 * 16 + 1  # below the row gate
        m(x, torch.tensor([500.0]), kv, cfg_pairs=True)
        assert p.calls == {"attention": 0, "residual": 0}


def test_reference_broadcast_operands():
    torch.manual_seed(13)
    x, w = torch.randn(12, 8).bfloat16(), torch.randn(6, 8).bfloat16()
    r = torch.randn(4, 6).bfloat16()
    torch.testing.assert_close(ref.linear(x, w, residual=r, residual_rows=4), ref.linear(x, w, residual=r.repeat(3, 1)))
    torch.testing.assert_close(ops.linear(x, w, residual=r, residual_rows=4), ref.linear(x, w, residual=r.repeat(3, 1)))
    y, y2 = ops.linear_lnout(x, w, None, r, None, None, residual_rows=4)
    y0, y02 = ops.linear_lnout(x, w, None, r.repeat(3, 1), None, None)
    torch.testing.assert_close(y, y0)
    torch.testing.assert_close(y2, y02)
    img = torch.randn(4, 3, 3, 8).bfloat16()
    wc = ops.pack_conv_weight((torch.randn(8, 8, 1, 1) * 0.3).bfloat16())
    res = torch.randn(2, 3, 3, 8).bfloat16()
    torch.testing.assert_close(ops.conv2d(img, wc, None, 1, 1, residual=res, residual_rows=2 * 9),
                               ops.conv2d(img, wc, None, 1, 1, residual=res.repeat(2, 1, 1, 1)))
    q, k, v = torch.randn(2, 5, 2, 8).bfloat16(), torch.randn(4, 7, 2, 8).bfloat16(), torch.randn(4, 7, 2, 8).bfloat16()
    o = ops.attention(q, k, v, q_batch_mod=2)
    assert o.shape == (4, 5, 2, 8)
    torch.testing.assert_close(o, ops.attention(q.repeat(2, 1, 1, 1), k, v))
    with pytest.raises(AssertionError):
        ref.linear(x, w, residual=torch.randn(5, 6).bfloat16(), residual_rows=5)  # 5 does not divide 12
