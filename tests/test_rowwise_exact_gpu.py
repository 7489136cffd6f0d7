"""Row-wise and element-wise kernels against an fp64 oracle, every element compared (tests/rowwise_exact.py).

Exact (torch.equal with bf16(fp64 result)) wherever the arithmetic is exact -- integer inputs, dyadic RoPE tables and
scalars: gated_act / bias_act without a smooth activation, rope, rope_pairs, kv_write, rope_qkv_cache, sched_step
pred 2, embedding, token_feedback, qk_norm_rope without weights; each of the grid-stride kernels once at a small odd
shape and once with more than twice its grid cap in loop items, so three trips of the loop run.  Within one bf16 ulp
of the oracle elsewhere (row norms with K = 30, softmax, SiLU / GELU, sched_step pred 0 / 1), GroupNorm (scale, shift)
within 4 / 8 fp32 roundings.  Operands lie in poison buffers, outputs in sentinel buffers that must survive around
the view.  The binding checks added with these tests each have a case that expects the error.
"""
import pytest
import torch

import rowwise_exact as rx
import shai_amd.ops as ops
from shai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def K():
    return ops._K()


# ----------------------------------------------------------------------------- row norms
@pytest.mark.parametrize("D", rx.D8ROW + rx.DWAVE)
@pytest.mark.parametrize("variant", list(rx.VARIANTS))
def test_row_norm(cuda, variant, D):
    """rmsnorm (w_offset 0 / 1) and layernorm (with / without w, b) at rows 1 / 5 / 37 and the four input families:
    every NV instance of the 8-row kernel (D = 64 k) and every MAXC instance of the wave-per-row kernel."""
    for rows in rx.ROWS:
        for fam in rx.FAMILIES:
            c = rx.make_rownorm(f"{variant}_D{D}_r{rows}_{fam}")
            obuf, idx, _, _ = rx.run_rownorm(c, K())
            rx.check_rownorm(c, obuf.cpu(), idx)


@pytest.mark.parametrize("name", [n for n in rx.ROWNORM_CASES if "_res_" in n])
def test_row_norm_residual(cuda, name):
    """residual_out == bf16(x + r) bit for bit (the sums need the rounding), y = norm(residual_out)."""
    c = rx.make_rownorm(name)
    obuf, idx, rbuf, ridx = rx.run_rownorm(c, K())
    rx.check_rownorm(c, obuf.cpu(), idx, rbuf.cpu(), ridx)


@pytest.mark.parametrize("name", [n for n in rx.ROWNORM_CASES if "_cols_" in n])
def test_row_norm_strided(cuda, name):
    """x and out as column slices of wider buffers (row stride D + 16); rmsnorm also through ops.rmsnorm(out=...)."""
    c = rx.make_rownorm(name)
    obuf, idx, _, _ = rx.run_rownorm(c, K())
    rx.check_rownorm(c, obuf.cpu(), idx)
    if c.norm == "rms":
        obuf, idx, _, _ = rx.run_rownorm(c, K(), use_ops=ops)
        rx.check_rownorm(c, obuf.cpu(), idx, what=name + " ops.rmsnorm(out=)")


@pytest.mark.parametrize("name", [n for n in rx.ROWNORM_CASES if n.startswith("mod_")])
def test_layernorm_mod(cuda, name):
    """rows_per_mod 1 / 3 / 77 at D 320 / 3072: groups that end inside a wave's 8 rows, the last group partial,
    scale / shift as strided column chunks of one tensor."""
    c = rx.make_rownorm(name)
    obuf, idx, _, _ = rx.run_rownorm(c, K())
    rx.check_rownorm(c, obuf.cpu(), idx)


def test_row_norm_rejected_layouts(cuda):
    """D above 8192 and a residual with a strided x raise."""
    x = torch.zeros(4, 8200, dtype=BF16, device="cuda")
    for fn in (lambda: K().rmsnorm(x, None, torch.empty_like(x), None, None, 1e-6, 0.0),
               lambda: K().layernorm(x, None, None, torch.empty_like(x), None, None, 1e-5),
               lambda: K().layernorm_mod(x, x[:1], x[:1], torch.empty_like(x), 4, 1e-6)):
        with pytest.raises(RuntimeError, match="<= 8192"):
            fn()
    wide = torch.zeros(4, 336, dtype=BF16, device="cuda")
    xs, r = wide[:, 8:328], torch.zeros(4, 320, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="contiguous"):
        K().rmsnorm(xs, None, torch.empty_like(r), r, torch.empty_like(r), 1e-6, 0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        K().layernorm(xs, None, None, torch.empty_like(r), r, torch.empty_like(r), 1e-5)


@pytest.mark.parametrize("name", list(rx.QKNR_CASES))
def test_qk_norm_rope(cuda, name):
    """D 64 / 128, H 1 / 3, 7 rows, ld = 3 H D + 16: weights on q / k / both / neither, with and without cos / sin.
    The v part and the padding never change; without weights the result is exact (without a table: unchanged)."""
    c = rx.make_qknr(name)
    d = c.place("cuda")
    ops.qk_norm_rope(d["x"], d.get("qw"), d.get("kw"), d.get("cos"), d.get("sin"), c.H, c.D, c.S, c.eps)
    rx.check_qknr(c, d["_x"])
    if not (c.has("qw") or c.has("kw") or c.has("cos")):
        assert torch.equal(d["_x"].cpu(), c.bufs["x"])


# ----------------------------------------------------------------------------- GroupNorm statistics
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("C,G", rx.GN_CG)
def test_gn_stats(cuda, monkeypatch, C, G, fused):
    """gn_stats_kernel + finalize (fused into the stats launch or not) three times per case (the tickets re-arm):
    (scale, shift) within 4 / 8 fp32 roundings of fp64; N = 1: the 256 partial slots sum to the exact integer sums."""
    monkeypatch.setattr(ops, "_GN_FUSED", fused)
    for name, kw in rx.GN_CASES.items():
        if (kw["C"], kw["G"]) != (C, G):
            continue
        c = rx.make_gn(name)
        d = c.place("cuda")
        for rep in range(3):
            sc, sh = ops.groupnorm_stats(d["x"], d["gamma"], d["beta"], G, rx.GN_EPS, x2=d.get("x2"))
            rx.check_gn(c, sc, sh, f"{name} fused {fused} call {rep}")
        if c.N == 1:
            part = torch.zeros(256, G, 2, dtype=torch.float32, device="cuda")
            sc, sh = torch.empty(1, C, dtype=torch.float32, device="cuda"), torch.empty(1, C, dtype=torch.float32,
                                                                                      device="cuda")
            K().groupnorm_stats(d["x"], d.get("x2"), d["gamma"], d["beta"], part, sc, sh, ops._gn_tickets(d["x"], 1),
                                G, rx.GN_EPS)
            want = rx.gn_sums64(rx.gn_x64(c).view(1, c.HW, G, -1))[0]
            rx.assert_exact(part.double().sum(0).cpu(), want, name + " partial sums")
            rx.check_gn(c, sc, sh, name + " own partials")
        rx.TOTALS["poison"] += c.poison_count()


# ----------------------------------------------------------------------------- grid-stride kernels
def _out_rows(rows, D):
    buf, idx = rx.rows_out(rows, D, after=1)
    buf = buf.cuda()
    return buf, buf[idx], idx


def _finish(c, buf, want64, idx, smooth=None, what=""):
    """Exact rule (or the smooth rule with ``smooth`` = sum of |terms|) on the view, canaries around it."""
    what = what or c.name
    if smooth is None:
        full = torch.full(buf.shape, rx.SENTINEL, dtype=BF16)
        full[idx] = rx.to_bf16_exact(want64)
        rx.assert_full_exact(buf, full, want64.numel(), what)
    else:
        rx.assert_smooth(buf[idx], want64, smooth, what)
        rx.assert_around(buf, torch.full(buf.shape, rx.SENTINEL, dtype=BF16), idx, what)
    rx.TOTALS["poison"] += c.poison_count()


@pytest.mark.parametrize("name", [n for n in rx.GRID_CASES if n.startswith("gated")])
def test_gated_act(cuda, name):
    """Strided x, both gate orders; relu exact (the big shape: 1 053 184 loop items), SiLU / GELU by the ulp rule."""
    c = rx.make_grid(name)
    d = c.place("cuda")
    for gate_first in (False, True):
        buf, out, idx = _out_rows(c.rows, c.F)
        K().gated_act(d["x"], out, ref.act_id(c.act), gate_first)
        y, zabs = rx.gated_want(c, gate_first)
        _finish(c, buf, y, idx, zabs if c.smooth else None, f"{name} gate_first {gate_first}")


@pytest.mark.parametrize("name", [n for n in rx.GRID_CASES if n.startswith("bias_act")])
def test_bias_act(cuda, name):
    c = rx.make_grid(name)
    d = c.place("cuda")
    buf, out, idx = _out_rows(c.rows, c.D)
    K().bias_act(d["x"], d.get("bias"), d.get("residual"), out, ref.act_id(c.act), c.alpha)
    y, zabs = rx.bias_act_want(c)
    _finish(c, buf, y, idx, zabs if c.smooth else None)


@pytest.mark.parametrize("name", ["embedding_small", "embedding_big"])
def test_embedding(cuda, name):
    c = rx.make_grid(name)
    d = c.place("cuda")
    buf, out, idx = _out_rows(c.T, c.D)
    K().embedding(c.ids.cuda(), d["table"], out)
    _finish(c, buf, c.f64("table")[c.ids.long()], idx)


@pytest.mark.parametrize("name", [n for n, (fn, _) in rx.GRID_CASES.items() if fn is rx.rope_case])
def test_rope(cuda, name):
    """NeoX and pair mode, rot_dim Dh and Dh / 2, q a view of packed qkv rows: the tail of each head, the k / v
    columns, the padding and the rows around never change."""
    c = rx.make_grid(name)
    d = c.place("cuda")
    ops.rope(rx.rope_view(c, d["x"]), c.pos.cuda(), d["cos"], d["sin"], c.rot, c.neox)
    want = rx.rope_model(c)
    rx.assert_full_exact(d["_x"], rx.to_bf16_exact(want), c.T * c.H * c.rot, name)
    q = rx.rope_view(c, c.view("x")).clone()       # the plain reference agrees with the index model
    ref.rope(q, c.pos, c.view("cos"), c.view("sin"), c.rot, c.neox)
    assert torch.equal(q, rx.rope_view(c, rx.to_bf16_exact(want)[1:1 + c.T]))
    rx.TOTALS["poison"] += c.poison_count()


@pytest.mark.parametrize("name", ["rope_pairs_small", "rope_pairs_big"])
def test_rope_pairs(cuda, name):
    """B > 1 with a batch stride of T + 1 rows and a token stride of H Dh + 8."""
    c = rx.make_grid(name)
    d = c.place("cuda")
    x = d["x"].unflatten(2, (c.H, c.Dh))
    ops.rope_pairs(x, d["cos"], d["sin"])
    rx.assert_full_exact(d["_x"], rx.to_bf16_exact(rx.rope_pairs_want(c)), c.view("x").numel(), name)
    rx.TOTALS["poison"] += c.poison_count()


def _caches(c):
    out = []
    for _ in range(2):
        buf, idx = rx.cache_bufs(c.nblocks, c.Hkv, c.D)
        buf = buf.cuda()
        out.append((buf, buf[idx]))
    return out


def _check_cache(c, buf, want64, what):
    full = torch.full(buf.shape, rx.SENTINEL, dtype=BF16)
    full[1:1 + c.nblocks] = want64.to(BF16)
    rx.assert_full_exact(buf, full, full != rx.SENTINEL, what)


@pytest.mark.parametrize("name", ["kvw_small", "kvw_big"])
def test_kv_write(cuda, name):
    """Shuffled slots, every seventh -1, strided k / v: written slots exact, the rest of the cache its sentinel."""
    c = rx.make_grid(name)
    d = c.place("cuda")
    (kb, kc), (vb, vc) = _caches(c)
    ops.kv_write(d["k"].unflatten(1, (c.Hkv, c.D)), d["v"].unflatten(1, (c.Hkv, c.D)), kc, vc, c.slots.cuda())
    kw, vw = rx.kvw_want(c)
    _check_cache(c, kb, kw, name + " k")
    _check_cache(c, vb, vw, name + " v")
    rx.TOTALS["poison"] += c.poison_count()


@pytest.mark.parametrize("name", ["rqc_small_64", "rqc_small_128", "rqc_big"])
def test_rope_qkv_cache(cuda, name):
    """bf16 cache, D 64 / 128, GQA, slot -1 rows: q rotated in place, k / v in qkv unchanged, rotated k and v in the
    cache, the cache elsewhere its sentinel (the big shape: 2 099 200 loop items, three trips of 4096 x 256)."""
    c = rx.make_grid(name)
    d = c.place("cuda")
    (kb, kc), (vb, vc) = _caches(c)
    ops.rope_qkv_cache(d["x"], c.pos.cuda(), d["cos"], d["sin"], kc, vc, c.slots.cuda(), c.H, c.Hkv)
    full, kw, vw = rx.made(("rqc_want", name), lambda: rx.rqc_model(c))
    rx.assert_full_exact(d["_x"], rx.to_bf16_exact(full), c.T * c.H * c.D, name + " qkv")
    _check_cache(c, kb, kw, name + " k")
    _check_cache(c, vb, vw, name + " v")
    rx.TOTALS["poison"] += c.poison_count()


@pytest.mark.parametrize("name", [n for n in rx.GRID_CASES if n.startswith("sched")])
def test_sched_step(cuda, name):
    """sched_step and sched_step_rows, cfg on / off: pred 2 exact, pred 0 / 1 by the ulp rule; idle rows, the poison
    around the latents and model_out unchanged."""
    c = rx.make_grid(name)
    d = c.place("cuda")
    if c.B:
        ops.sched_step_rows(d["mo"], d["lat"].view(c.B, -1), c.cfg, c.guidance, c.pred, c.rows_params.cuda())
    else:
        ops.sched_step(d["mo"], d["lat"], c.cfg, c.guidance, c.pred, c.a_t, c.a_prev, c.dt)
    y, terms, active = rx.sched_want(c)
    idx = c.idx["lat"]
    assert torch.equal(d["_mo"].cpu(), c.bufs["mo"])
    if c.pred == 2:
        full = c.bufs["lat"].clone()
        full[idx] = rx.to_bf16_exact(y)
        rx.assert_full_exact(d["_lat"], full, c.n, name)
    else:
        got = d["lat"].cpu()
        rx.assert_smooth(got[active], y[active], terms[active], name)
        rx.assert_exact(got[~active], c.view("lat")[~active], name + " idle rows")
        rx.assert_around(d["_lat"], c.bufs["lat"], idx, name)
    rx.TOTALS["poison"] += c.poison_count()


@pytest.mark.parametrize("D", [8, 2048, 2056, 4096])
def test_softmax(cuda, D):
    """|y - y64| <= ulp_bf16(y64), every element; the rows around unchanged."""
    c = rx.make_grid(f"softmax_D{D}")
    d = c.place("cuda")
    ops.softmax_(d["x"], c.scale)
    y = torch.softmax(c.f64("x") * c.scale, -1)
    rx.assert_within(d["x"], y, rx.ulp_bf16(y), c.name)
    rx.assert_around(d["_x"], c.bufs["x"], c.idx["x"], c.name)
    rx.TOTALS["poison"] += c.poison_count()


def test_token_feedback(cuda):
    """n = 1000 (no multiple of 256), negative rowmap entries keep the host's id, the ids around n unchanged."""
    g = rx._gen(4100)
    n = 1000
    buf = torch.randint(0, 32000, (n + 16,), generator=g, dtype=torch.int32)
    prev = torch.randint(0, 32000, (300,), generator=g, dtype=torch.int32)
    rowmap = torch.randint(-1, 300, (n,), generator=g, dtype=torch.int32)
    rowmap[::5] = -1
    dev = buf.cuda()
    ops.token_feedback(dev[8:8 + n], rowmap.cuda(), prev.cuda())
    want = buf.clone()
    want[8:8 + n] = torch.where(rowmap >= 0, prev[rowmap.clamp_min(0).long()], buf[8:8 + n])
    rx.assert_exact(dev.cpu(), want, "token_feedback")


# ----------------------------------------------------------------------------- binding checks
def test_binding_checks(cuda):
    """Every check added to csrc/bindings.cpp with these tests refuses its bad call."""
    dev = "cuda"
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    x = z(4, 2, 64)
    for rot in (0, 31, 66, -2):
        with pytest.raises(RuntimeError, match="rot_dim"):
            K().rope(x, i(4), f(8, 32), f(8, 32), rot, True)
    with pytest.raises(RuntimeError, match=r"max_pos, rot_dim / 2"):   # a [max_pos, Dh / 2] table with rot_dim < Dh
        K().rope(x, i(4), f(8, 32), f(8, 32), 32, True)
    with pytest.raises(RuntimeError, match=r"max_pos, rot_dim / 2"):
        K().rope(x, i(4), f(8, 32), f(8, 16), 64, True)
    with pytest.raises(RuntimeError, match="contiguous"):
        K().rope(x, i(4), f(8, 64)[:, :32], f(8, 32), 64, True)
    with pytest.raises(RuntimeError, match="positions must have T"):
        K().rope(x, i(3), f(8, 32), f(8, 32), 64, True)
    k, cache = z(4, 2, 64), z(3, 2, 64, 64)
    with pytest.raises(RuntimeError, match="slots must have T"):
        K().kv_write(k, k, cache, cache.clone(), i(3))
    with pytest.raises(RuntimeError, match="must match the cache"):
        K().kv_write(k, z(4, 2, 32), cache, cache.clone(), i(4))
    with pytest.raises(RuntimeError, match="must match the cache"):
        K().kv_write(k, k, z(3, 4, 64, 64), z(3, 4, 64, 64), i(4))
    with pytest.raises(RuntimeError, match=r"blocks, Hkv, 64, D"):
        K().kv_write(k, k, z(3, 2, 32, 64), z(3, 2, 32, 64), i(4))
    with pytest.raises(RuntimeError, match="D % 8"):
        K().kv_write(z(1, 1, 12), z(1, 1, 12), z(3, 1, 64, 12), z(3, 1, 64, 12), i(1))
    y = z(4, 64)
    with pytest.raises(RuntimeError, match="bias must have D"):
        K().bias_act(y, z(32), None, torch.empty_like(y), 0, 1.0)
    with pytest.raises(RuntimeError, match="bfloat16"):
        K().bias_act(y, f(64), None, torch.empty_like(y), 0, 1.0)
    with pytest.raises(RuntimeError, match="bfloat16"):
        K().bias_act(y, None, f(4, 64), torch.empty_like(y), 0, 1.0)
    wide = z(2, 5, 2 * 64 + 4)
    with pytest.raises(RuntimeError, match="16-byte aligned"):   # token stride 132, batch stride 660
        K().rope_pairs(wide[:, :, :128].unflatten(2, (2, 64)), f(5, 32), f(5, 32))
    with pytest.raises(RuntimeError, match=r"out must be \[ids"):
        K().embedding(i(4), z(10, 64), z(3, 64))
    with pytest.raises(RuntimeError, match=r"out must be \[ids"):
        K().embedding(i(4), z(10, 64), z(4, 32))
    with pytest.raises(RuntimeError, match="positions / slots must have T"):
        K().rope_qkv_cache(z(4, 4 * 64), i(4), f(8, 32), f(8, 32), z(3, 1, 64, 64), z(3, 1, 64, 64), i(3), 2, 1)


def test_zz_totals(cuda):
    """What this file's checks looked at in this process: printed for the record."""
    print("TOTALS compared {compared} canaries {canaries} poison {poison}".format(**rx.TOTALS))
    print(f"row norms: worst (|y - y64| - ulp) / (2^-24 M) = {rx.WORST['rownorm_k']:.2f} of K = {rx.K}")
    assert rx.TOTALS["compared"] > 0
