"""Cases, fp64 oracles, rules and index-model mutants for the row-wise and element-wise kernels (norm.hip row norms and
GroupNorm statistics, dit.hip qk_norm_rope, elementwise.hip, attention.hip kv_write / rope_qkv_cache).

Plain helpers for tests/test_rowwise_exact_{cpu,gpu}.py (no fixtures, no pytest settings); the poison / canary layout
and the assert helpers are those of tests/gemm_exact.py; TOTALS counts what this module's checks looked at.

Why: these kernels were judged by close() (0.1 % of the elements may be out of tolerance) and GroupNorm statistics by
assert_close(1e-3).  One wrong last row, a 16-byte vector left out of a row's statistics, a pixel dropped at a stats
block boundary, a grid-stride loop that never takes its second trip: all pass those rules.

Two rules, every element compared:

1. EXACT (torch.equal) where the arithmetic can be exact.  Inputs are small integers, RoPE tables hold dyadic values
   k / 64 with |k| <= 64 (one (cos, sin) pair per (position, column): ``rope_table``), scalars are dyadic.  Every fp32
   operation is then exact and the output is bf16(fp64 result) bit for bit.
2. ONE bf16 ULP of an fp64 oracle of the same bf16 inputs where a square root, exponential or activation is involved.
   Row norms: |y - y64| <= ulp_bf16(y64) + K 2^-24 M with M = rstd64 |w + w_offset| (|x| + |mean64|) + |b|, the size
   of the terms that cancel.  K = 4 x the floor, the largest |y32 - y64| / (2^-24 M) of a plain fp32 torch evaluation
   of the same formula (unrounded) over all committed row-norm cases: measured floor 7.15 (at
   ln_D2056_r37_spike_first) -> K_FLOOR = 7.5, K = 30 (cap 256 = 1/256 of a bf16 ulp of M).  The inputs are integers
   times a power of two per row, so the row sums that give the mean are exact in fp32 in any order; the margin of 4
   covers the order of the variance sum and rsqrtf.
   Residual: h = bf16(x + r) must be ``residual_out`` bit for bit, and y = norm(h).
   Softmax: |y - y64| <= ulp_bf16(y64) (logit spread <= 20).  sched_step pred 0 / 1, SiLU, GELU: gemm_exact's
   ulp_bf16(y64) + 1e-6 (sum of |terms|).  GroupNorm (scale, shift), integer inputs, every sum below 2^24 (partial sums
   exact, finalize in double): |sc - sc64| <= 4 2^-24 |sc64|, |sh - sh64| <= 8 2^-24 (|beta| + |mean64 sc64|).

Every operand is a view inside a +-1024 poison buffer; every output a view inside a sentinel buffer (or, in place,
inside its poison buffer), and all that surrounds the view must survive bit for bit.

GroupNorm statistics, extra HW per C (more than one stats block, ppb no multiple of 4 P; ``gn_num_blocks`` mirrors
norm.hip): C 8 -> HW 2051 (2 blocks of 1026, P 256), 64 -> 300 (2 x 150, P 32), 96 -> 200 (2 x 100, P 21), 320 -> 100
(3 x 34, P 6), 2048 -> 27 (6 x 5, P 1), 2560 -> 9 (2 x 5, P 1, two channel vectors per thread), 4096 -> 5 (2 x 3, P 1).
"""
import torch

import gemm_exact as ge
from gemm_exact import (BF16, POISON, SENTINEL, _gen, _ints, _poison, embed_rows, embed_vec,  # noqa: F401
                        to_bf16_exact, ulp_bf16)

TOTALS = {"compared": 0, "canaries": 0, "poison": 0}   # what the checks of this module have looked at
WORST = {"rownorm_k": 0.0}   # the largest (|y - y64| - ulp) / (2^-24 M) a row-norm check has seen (<= K to pass)
LIMIT = ge.LIMIT
U24 = 2.0 ** -24
K_FLOOR = 7.5           # measured 7.15 (tests/test_rowwise_exact_cpu.py::test_k_floor), rounded up
K = 4 * K_FLOOR         # 30
K_CAP = 256.0
CAP = 2048 * 256        # elementwise.hip / kv_write: grid cap x block
CAP_RQC = 4096 * 256    # rope_qkv_cache
_made = {}


def made(key, fn):
    """Build once per key, share, never modify."""
    if key not in _made:
        _made[key] = fn()
    return _made[key]


class Case(ge.Case):
    def off(self, name):
        return self.view(name).storage_offset()


def rows_out(rows, D, before=1, after=8):
    """Contiguous output view buf[before:before + rows] of a sentinel buffer."""
    return torch.full((before + rows + after, D), SENTINEL, dtype=BF16), (slice(before, before + rows), slice(0, D))


def cols_out(rows, D, before=8, after=8):
    """Output as a column slice of a wider sentinel buffer (with sentinel rows around)."""
    return (torch.full((1 + rows + 8, before + D + after), SENTINEL, dtype=BF16),
            (slice(1, 1 + rows), slice(before, before + D)))


def _counted_here(fn):
    """gemm_exact's assert helper, counting into this module's TOTALS instead of its own."""
    def wrapped(got, *a, **kw):
        TOTALS["compared"] += got.numel()
        keep = ge.TOTALS["compared"]
        try:
            return fn(got, *a, **kw)
        finally:
            ge.TOTALS["compared"] = keep
    return wrapped


assert_exact = _counted_here(ge.assert_exact)
assert_smooth = _counted_here(ge.assert_smooth)


def assert_within(got, y64, tol, what=""):
    """|got - y64| <= tol, every element."""
    TOTALS["compared"] += got.numel()
    g = got.double().cpu()
    assert g.shape == y64.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(y64.shape)}"
    bad = ~((g - y64).abs() <= tol)
    if bool(bad.any()):
        raise AssertionError(ge._report(g, y64, bad, what))


def assert_around(got_full, before_full, idx, what=""):
    """Everything of the buffer outside the view ``idx`` is what it was (canaries / poison / untouched data)."""
    got = got_full.cpu()
    mask = torch.ones(before_full.shape, dtype=torch.bool)
    mask[idx] = False
    TOTALS["canaries"] += int(mask.sum())
    hit = mask & ~(got.double() == before_full.double())
    if bool(hit.any()):
        raise AssertionError(ge._report(got.double(), before_full.double(), hit, f"{what}: canary overwritten"))


def assert_full_exact(got_full, want_full, written, what=""):
    """The whole buffer equals ``want_full``; ``written`` (bool mask or count) tells results from canaries."""
    n = int(written.sum()) if isinstance(written, torch.Tensor) else int(written)
    TOTALS["compared"] += n
    TOTALS["canaries"] += want_full.numel() - n
    want_full = want_full.to(got_full.device)
    if torch.equal(got_full, want_full):
        return
    g, w = got_full.double().cpu(), want_full.double().cpu()
    bad = ~(g == w)
    if isinstance(written, torch.Tensor) and bool((bad & ~written).any()):
        raise AssertionError(ge._report(g, w, bad & ~written, f"{what}: canary overwritten"))
    raise AssertionError(ge._report(g, w, bad, what))


def rope_table(g, max_pos, half, before=1, after=1):
    """(cos, sin) fp32 [max_pos, half] with values k / 64, |k| <= 64, a different pair at every (position, column);
    each a contiguous view between poison rows."""
    n = torch.arange(max_pos * half)
    assert max_pos * half <= 129 * 129
    kc = n % 129 - 64
    ks = ((n // 129) * 37 + 11) % 129 - 64
    out = []
    for k in (kc, ks):
        buf = _poison(g, before + max_pos + after, half)
        buf[before:before + max_pos] = (k.float() / 64).view(max_pos, half)
        out.append((buf, (slice(before, before + max_pos),)))
    return out


def _add_table(c, g, max_pos, half):
    (cb, ci), (sb, si) = rope_table(g, max_pos, half)
    c.add("cos", cb, ci, dtype=torch.float32)
    c.add("sin", sb, si, dtype=torch.float32)


# ----------------------------------------------------------------------------- row norms
D8ROW = [64 * k for k in range(1, 9)]                         # 8-rows-per-wave kernel, NV 1..8
DWAVE = [8, 72, 520, 1000, 1032, 2056, 4104, 8192]            # wave-per-row kernel, MAXC 1, 1, 2, 2, 4, 8, 16, 16
ROWS = (1, 5, 37)
FAMILIES = ("random", "spike_first", "spike_last", "one_lane")
VARIANTS = {"rms": dict(norm="rms"), "rms_off1": dict(norm="rms", w_offset=1.0), "ln": dict(norm="ln", b=True),
            "ln_plain": dict(norm="ln", w=False)}
EPS = {"rms": 1e-6, "ln": 1e-5}


def is_row8(D):
    return D % 64 == 0 and D <= 512


def _row_values(g, rows, D, family, wide=False):
    """Integers times 2^k per row (k in -6..6): bf16 numbers whose row sums are exact in fp32."""
    k = torch.randint(-6, 7, (rows, 1), generator=g)
    if family == "random":
        lim = 255 if wide else 100
        m = _ints(g, -lim, lim, rows, D) + (0 if wide else _ints(g, -60, 60, rows, 1))
    else:
        m = torch.zeros(rows, D) if family == "one_lane" else _ints(g, -1, 1, rows, D)
        spike = _ints(g, 128, 255, rows, 8) * (torch.randint(0, 2, (rows, 8), generator=g) * 2 - 1)
        if family == "spike_first":
            m[:, :8] = spike
        else:
            m[:, D - 8:] = spike
    return torch.ldexp(m, k), k


def rownorm_case(name, norm, rows, D, family, seed, w=True, b=False, w_offset=0.0, residual=False, layout="rows",
                 mod=0):
    """x [rows, D] between poison rows (``rows``: contiguous) or as a column slice of a wider poison matrix
    (``cols``); w / b [D] inside poison vectors; residual [rows, D] contiguous; mod = rows_per_mod: scale / shift
    [G, D] as two strided column chunks of one [G + 2, 2 D + 24] poison tensor, the last group partial."""
    g = _gen(seed)
    c = Case(name, kind="rownorm", norm=norm, rows=rows, D=D, family=family, w_offset=1.0 if mod else w_offset,
             eps=1e-6 if mod else EPS[norm], layout=layout, mod=mod, residual=residual)
    x, k = _row_values(g, rows, D, family, wide=residual)
    if layout == "cols":
        buf = _poison(g, 1 + rows + 1, D + 16)
        buf[1:1 + rows, 8:8 + D] = x
        c.add("x", buf, (slice(1, 1 + rows), slice(8, 8 + D)))
    else:
        c.add("x", *embed_rows(g, x, 1, 1))
    if residual:
        # the row's own 2^k: x + r is an integer of up to 9 bits times 2^k, so bf16(x + r) rounds
        c.add("r", *embed_rows(g, torch.ldexp(_ints(g, -255, 255, rows, D), k), 1, 1))
    if mod:
        G = (rows + mod - 1) // mod
        buf = _poison(g, G + 2, 2 * D + 24)
        buf[1:1 + G, 8:8 + D] = _ints(g, -16, 16, G, D) / 8
        buf[1:1 + G, 16 + D:16 + 2 * D] = _ints(g, -16, 16, G, D) / 4
        c.add("w", buf, (slice(1, 1 + G), slice(8, 8 + D)))
        c.add("b", buf.clone(), (slice(1, 1 + G), slice(16 + D, 16 + 2 * D)))
        c.G = G
    else:
        if w:
            c.add("w", *embed_vec(g, _ints(g, -64, 64, D) / 32))
        if b:
            c.add("b", *embed_vec(g, _ints(g, -32, 32, D) / 16))
    return c


def rownorm_out(c):
    return cols_out(c.rows, c.D) if c.layout == "cols" else rows_out(c.rows, c.D)


def rownorm_h(c):
    """The normalised input as the kernel holds it: x, or bf16(x + r) (one fp32 add, exact here, one rounding)."""
    if not c.residual:
        return c.view("x")
    s = c.f64("x") + c.f64("r")
    assert bool((s.float().double() == s).all())
    return s.float().to(BF16)


def _row_params(c, t, dt):
    """w / b as [rows, D] or [D] (None if absent) in dtype dt; the modulation rows of ``layernorm_mod`` expanded."""
    v = c.view(t)
    if v is None:
        return None
    v = v.to(dt)
    return v[torch.arange(c.rows) // c.mod] if c.mod else v


def rownorm_eval(c, h, dt):
    """The formula, plainly, in dtype dt: (y, M)."""
    x = h.to(dt)
    w, b = _row_params(c, "w", dt), _row_params(c, "b", dt)
    if c.norm == "rms":
        mean = torch.zeros(c.rows, 1, dtype=dt)
        rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + c.eps)
    else:
        mean = x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + c.eps)
    wf = (w + c.w_offset) if w is not None else torch.ones(1, dtype=dt)
    y = (x - mean) * rstd * wf
    M = rstd * wf.abs() * (x.abs() + mean.abs())
    if b is not None:
        y, M = y + b, M + b.abs()
    return y, M


def rownorm_want(c):
    """(h bf16, y64, tolerance): computed once per case."""
    def f():
        h = rownorm_h(c)
        y64, M = rownorm_eval(c, h, torch.float64)
        return h, y64, ulp_bf16(y64) + K * U24 * M
    return made(("rownorm_want", c.name), f)


def rownorm_floor(c):
    """max |y32 - y64| / (2^-24 M) of the fp32 evaluation (M = 0: y32 must equal y64)."""
    h = rownorm_h(c)
    y64, M = rownorm_eval(c, h, torch.float64)
    y32, _ = rownorm_eval(c, h, torch.float32)
    err = (y32.double() - y64).abs()
    assert bool((err[M == 0] == 0).all())
    return float((err[M > 0] / (U24 * M[M > 0])).max()) if bool((M > 0).any()) else 0.0


def check_rownorm(c, out_full, idx, res_full=None, res_idx=None, what=""):
    """The rule on the output view, ``residual_out`` bit-exact, and all canaries of both buffers."""
    h, y64, tol = rownorm_want(c)
    what = what or c.name
    assert_within(out_full[idx], y64, tol, what)
    over = ((out_full[idx].double().cpu() - y64).abs() - ulp_bf16(y64)) / (tol - ulp_bf16(y64)).clamp_min(1e-300) * K
    WORST["rownorm_k"] = max(WORST["rownorm_k"], float(over.max()))   # how much of K 2^-24 M the outputs use
    assert_around(out_full, rownorm_out(c)[0], idx, what)
    if c.residual:
        assert_exact(res_full[res_idx].cpu(), h, what + " residual_out")
        assert_around(res_full, rows_out(c.rows, c.D)[0], res_idx, what + " residual_out")
    TOTALS["poison"] += c.poison_count()


def run_rownorm(c, K_, device="cuda", use_ops=None):
    """Through the native op (or ops.rmsnorm(out=...) with ``use_ops``): (out buffer, idx, residual_out buffer, idx)."""
    d = c.place(device)
    obuf, idx = rownorm_out(c)
    obuf = obuf.to(device)
    out = obuf[idx]
    rbuf = ridx = rout = None
    if c.residual:
        rbuf, ridx = rows_out(c.rows, c.D)
        rbuf = rbuf.to(device)
        rout = rbuf[ridx]
    if c.mod:
        K_.layernorm_mod(d["x"], d["w"], d["b"], out, c.mod, c.eps)
    elif use_ops is not None:
        y, _ = use_ops.rmsnorm(d["x"], d.get("w"), c.eps, w_offset=c.w_offset, out=out)
        assert y.data_ptr() == out.data_ptr()
    elif c.norm == "rms":
        K_.rmsnorm(d["x"], d.get("w"), out, d.get("r"), rout, c.eps, c.w_offset)
    else:
        K_.layernorm(d["x"], d.get("w"), d.get("b"), out, d.get("r"), rout, c.eps)
    return obuf, idx, rbuf, ridx


def rownorm_model(c, mut=None):
    """The row norms by explicit index over the flat buffers, as the kernels address them (fp64 arithmetic, one
    rounding to bf16); ``mut``: one addressing mistake.  Returns (out buffer, residual_out buffer or None)."""
    rows, D = c.rows, c.D
    row8 = is_row8(D)
    xv = c.view("x")
    xflat = c.bufs["x"].double().flatten()
    xs = D if mut == "x_stride_D" else xv.stride(0)
    r_, col = torch.arange(rows)[:, None], torch.arange(D)[None, :]
    x = xflat[(c.off("x") + r_ * xs + col).clamp_max(xflat.numel() - 1)]
    obuf, idx = rownorm_out(c)
    oflat = obuf.double().flatten()
    o_off, os_ = obuf[idx].storage_offset(), obuf[idx].stride(0)
    rflat = None
    if c.residual:
        x = (x + c.bufs["r"].double().flatten()[c.off("r") + r_ * D + col]).float().to(BF16).double()
        rbuf, ridx = rows_out(rows, D)
        rflat = rbuf.double().flatten()
        r_off = rbuf[ridx].storage_offset()
        rflat[r_off + r_ * D + col] = x
        if mut == "res_dead_lanes" and row8:     # the dead lanes of the last wave store their mirrored row
            dead = torch.arange(rows, (rows + 7) // 8 * 8)[:, None]
            rflat[r_off + dead * D + col] = x[rows - 1]
    n = D - 8 if mut == "stats_short" else D
    xs_ = x[:, :n]
    s1, s2 = xs_.sum(-1, keepdim=True), (xs_ * xs_).sum(-1, keepdim=True)
    dup = torch.ones(rows, 1, dtype=torch.float64)
    if mut == "mirror_stats" and row8 and rows % 8:   # the last live row's reduction takes in the mirroring lanes
        dup[rows - 1] = 2.0
    if c.norm == "rms":
        mean = torch.zeros(rows, 1, dtype=torch.float64)
        rstd = 1.0 / torch.sqrt(s2 * dup / D + c.eps)
    else:
        mean = s1 * dup / D
        rstd = 1.0 / torch.sqrt(((xs_ - mean) ** 2).sum(-1, keepdim=True) * dup / D + c.eps)
    wrow = r_
    if mut == "mod_per_wave":                     # the modulation row of the wave's (block's) first row
        wrow = r_ // 8 * 8 if row8 else r_ // 4 * 4
    wcol = col.expand(rows, D).clone()
    if mut == "w_neighbour":                      # the last chunk's w read one 16-byte vector early
        first = (D - 1) // 64 * 64 if row8 else (D - 1) // 512 * 512
        wcol[:, first:] -= 8

    def param(t):
        if not c.has(t):
            return None
        flat = c.bufs[t].double().flatten()
        base = c.off(t) + ((wrow // c.mod) * c.view(t).stride(0) if c.mod else 0)
        return flat[(base + wcol).clamp(0, flat.numel() - 1)]
    w, b = param("w"), param("b")
    y = (x - mean) * rstd * ((w + c.w_offset) if w is not None else 1.0)
    if b is not None:
        y = y + b
    if mut == "out_stride_D":
        os_ = D
    oflat[o_off + r_ * os_ + col] = y.float().to(BF16).double()
    out = oflat.view(obuf.shape).to(BF16)
    return out, (None if rflat is None else rflat.view(rbuf.shape).to(BF16))


def rownorm_cases():
    """{name: kwargs} of every committed row-norm case."""
    cases, seed = {}, 1000
    for vn, v in VARIANTS.items():
        for D in D8ROW + DWAVE:
            for rows in ROWS:
                for fam in FAMILIES:
                    seed += 1
                    cases[f"{vn}_D{D}_r{rows}_{fam}"] = dict(v, rows=rows, D=D, family=fam, seed=seed)
    for norm in ("rms", "ln"):
        for D in (64, 320, 520, 4104):
            for rows in ROWS:
                seed += 1
                cases[f"{norm}_res_D{D}_r{rows}"] = dict(norm=norm, rows=rows, D=D, family="random", seed=seed,
                                                         residual=True, b=norm == "ln")
        for D in (320, 520, 8192):
            for rows in (5, 37):
                seed += 1
                cases[f"{norm}_cols_D{D}_r{rows}"] = dict(norm=norm, rows=rows, D=D, family="random", seed=seed,
                                                          layout="cols", b=norm == "ln")
    for D in (320, 3072):
        for rpm, rows in ((1, 5), (3, 37), (77, 100)):    # 37 = 12 x 3 + 1, 100 = 77 + 23: the last group is partial
            for layout in ("rows", "cols"):
                seed += 1
                cases[f"mod_D{D}_rpm{rpm}_{layout}"] = dict(norm="ln", rows=rows, D=D, family="random", seed=seed,
                                                           mod=rpm, layout=layout)
    return cases


ROWNORM_CASES = rownorm_cases()


def make_rownorm(name):
    return made(("rownorm", name), lambda: rownorm_case(name, **ROWNORM_CASES[name]))


# ----------------------------------------------------------------------------- qk_norm_rope
def qknr_case(name, rows, H, D, S, seed, qw=False, kw=False, table=False):
    """Packed x [rows, 3 H D] inside a poison buffer with 16 padding columns (ld > 3 H D) and a row before / behind."""
    g = _gen(seed)
    c = Case(name, kind="qknr", rows=rows, H=H, D=D, S=S, eps=1e-6)
    W = 3 * H * D
    c.add("x", *embed_rows(g, _ints(g, -8, 8, rows, W), 1, 1, W + 16))
    if qw:
        c.add("qw", *embed_vec(g, _ints(g, -64, 64, D) / 32))
    if kw:
        c.add("kw", *embed_vec(g, _ints(g, -64, 64, D) / 32))
    if table:
        _add_table(c, g, S, D // 2)
    return c


def qknr_want(c):
    """(fp64 full buffer, tolerance full buffer (0 where exact), written mask)."""
    buf = c.bufs["x"].double().clone()
    tol = torch.zeros_like(buf)
    written = torch.zeros(buf.shape, dtype=torch.bool)
    rows, H, D = c.rows, c.H, c.D
    pos = torch.arange(rows) % c.S
    for j, wn in enumerate(("qw", "kw")):
        cols = slice(j * H * D, (j + 1) * H * D)
        t = buf[1:1 + rows, cols].reshape(rows, H, D).clone()
        m = t.abs()
        if c.has(wn):
            w = c.f64(wn)
            rstd = 1.0 / torch.sqrt((t * t).mean(-1, keepdim=True) + c.eps)
            t, m = t * rstd * w, m * rstd * w.abs()
        if c.has("cos"):
            co, si = c.f64("cos")[pos][:, None, :], c.f64("sin")[pos][:, None, :]
            a, b, ma, mb = t[..., 0::2].clone(), t[..., 1::2].clone(), m[..., 0::2].clone(), m[..., 1::2].clone()
            t[..., 0::2], t[..., 1::2] = a * co - b * si, b * co + a * si
            m[..., 0::2] = m[..., 1::2] = ma * co.abs() + mb * si.abs() + mb * co.abs() + ma * si.abs()
        buf[1:1 + rows, cols] = t.reshape(rows, H * D)
        if c.has(wn):
            tol[1:1 + rows, cols] = (ulp_bf16(t) + K * U24 * m).reshape(rows, H * D)
        written[1:1 + rows, cols] = c.has(wn) or c.has("cos")
    return buf, tol, written


def check_qknr(c, got_full, what=""):
    buf, tol, written = made(("qknr_want", c.name), lambda: qknr_want(c))
    exact = tol == 0
    g = got_full.cpu().double()
    TOTALS["compared"] += int(written.sum())
    TOTALS["canaries"] += int((~written).sum())
    want_exact = to_bf16_exact(torch.where(exact, buf, torch.zeros_like(buf))).double()
    bad = torch.where(exact, g != want_exact, ~((g - buf).abs() <= tol))
    if bool(bad.any()):
        raise AssertionError(ge._report(g, buf, bad, what or c.name))
    TOTALS["poison"] += c.poison_count()


QKNR_CASES = {}
for _D in (64, 128):
    for _H in (1, 3):
        for _n, _q, _k in (("both", True, True), ("q", True, False), ("k", False, True), ("none", False, False)):
            for _t in (True, False):
                QKNR_CASES[f"qknr_D{_D}_H{_H}_{_n}_{'rope' if _t else 'norope'}"] = dict(
                    rows=7, H=_H, D=_D, S=3, qw=_q, kw=_k, table=_t, seed=2000 + len(QKNR_CASES))


def make_qknr(name):
    return made(("qknr", name), lambda: qknr_case(name, **QKNR_CASES[name]))


# ----------------------------------------------------------------------------- GroupNorm statistics
GN_CG = [(8, 1), (8, 8), (64, 32), (96, 24), (320, 32), (2048, 32), (2560, 32), (4096, 128)]
GN_HW = (1, 7, 100)
GN_HW_EXTRA = {8: 2051, 64: 300, 96: 200, 320: 100, 2048: 27, 2560: 9, 4096: 5}
GN_TWO = {(320, 32): 88, (2048, 32): 520, (2560, 32): 1288, (4096, 128): 1000}   # C1, no multiple of C / G
GN_EPS = 1e-5


def gn_num_blocks(N, HW, C):
    """csrc/kernels/norm.hip gn_num_blocks."""
    by_size = HW * C * 2 // (16 << 10)
    nb = min((2048 + N - 1) // N, by_size, HW, 256)
    return max(nb, 1)


def gn_geometry(N, HW, C):
    """(NB, ppb, P) of launch_groupnorm_stats."""
    nb = gn_num_blocks(N, HW, C)
    C8 = C // 8
    return nb, (HW + nb - 1) // nb, (256 // C8 if C8 <= 256 else 1)


def gn_case(name, N, HW, C, G, seed, C1=0):
    """x [N, HW, C1 or C] (x2 [N, HW, C - C1]) integers in -3..3 between a poison image before and behind, probes of
    magnitude 8..15 at the first and last pixel of every stats block and of the image; gamma k / 8, beta k / 4."""
    g = _gen(seed)
    c = Case(name, kind="gn", N=N, HW=HW, C=C, G=G, C1=C1 or C)
    x = _ints(g, -3, 3, N, HW, C)
    nb, ppb, _ = gn_geometry(N, HW, C)
    px = sorted({p for blk in range(nb) for p in (blk * ppb, min(HW, (blk + 1) * ppb) - 1) if 0 <= p < HW})
    probe = _ints(g, 8, 15, N, len(px), C) * (torch.randint(0, 2, (N, len(px), C), generator=g) * 2 - 1)
    x[:, px] = probe
    c.add("x", *ge.embed_lead(g, x[..., :c.C1].contiguous()))
    if C1:
        c.add("x2", *ge.embed_lead(g, x[..., C1:].contiguous()))
    c.add("gamma", *embed_vec(g, _ints(g, -16, 16, C) / 8))
    c.add("beta", *embed_vec(g, _ints(g, -16, 16, C) / 4))
    return c


def gn_x64(c):
    return torch.cat([c.f64("x"), c.f64("x2")], -1) if c.has("x2") else c.f64("x")


def gn_sums64(x):
    """x [N, HW, G, Cg] fp64 -> [N, G, 2] (sum, sum of squares)."""
    return torch.stack([x.sum((1, 3)), (x * x).sum((1, 3))], -1)


def gn_finish64(c, sums):
    """(scale, shift, tolerance of scale, tolerance of shift) from the [N, G, 2] sums, fp64."""
    Cg = c.C // c.G
    cnt = c.HW * Cg
    mean = sums[..., 0] / cnt
    var = (sums[..., 1] / cnt - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    mean_c, rstd_c = mean.repeat_interleave(Cg, 1), rstd.repeat_interleave(Cg, 1)
    sc = rstd_c * c.f64("gamma")
    sh = c.f64("beta") - mean_c * sc
    return sc, sh, 4 * U24 * sc.abs(), 8 * U24 * (c.f64("beta").abs() + (mean_c * sc).abs())


def gn_want(c):
    return made(("gn_want", c.name), lambda: gn_finish64(c, gn_sums64(gn_x64(c).view(c.N, c.HW, c.G, -1))))


def check_gn(c, scale, shift, what=""):
    sc, sh, tsc, tsh = gn_want(c)
    assert_within(scale, sc, tsc, (what or c.name) + " scale")
    assert_within(shift, sh, tsh, (what or c.name) + " shift")


def gn_model_sums(c, mut=None):
    """The [N, G, 2] sums as gn_stats_kernel collects them: per block and pixel lane the 4-deep loop and its tail,
    per thread one channel vector (two when C / 8 > 256), sources by flat index."""
    N, HW, C, G, C1 = c.N, c.HW, c.C, c.G, c.C1
    nb, ppb, P = gn_geometry(N, HW, C)
    C2, Cg = C - C1, C // G
    pix = []
    for blk in range(nb):
        p0, p1 = blk * ppb, min(HW, blk * ppb + ppb)
        if mut == "last_pixel_dropped":
            p1 -= 1
        if mut == "boundary_twice":
            p1 = min(HW, p1 + 1)
        for pl in range(P):
            p = p0 + pl
            while p + 3 * P < p1:
                pix += [p, p + P, p + 2 * P, p + 3 * P]
                p += 4 * P
            while p < p1:
                pix.append(p)
                p += P
    pix = torch.tensor(pix, dtype=torch.long)
    ch = torch.arange(C)
    f1 = c.bufs["x"].double().flatten()
    n_ = torch.arange(N)[:, None, None]
    p_, c_ = pix[None, :, None], ch[None, None, :]
    v = f1[c.off("x") + (n_ * HW + p_) * C1 + c_.clamp_max(C1 - 1)]
    if c.has("x2"):
        f2 = c.bufs["x2"].double().flatten()
        ld2 = C1 if mut == "x2_stride_c1" else C2
        i2 = c.off("x2") + n_ * HW * C2 + p_ * ld2 + (c_ - C1).clamp_min(0)
        v2 = f2[i2.clamp_max(f2.numel() - 1)]
        if mut == "span_group_x_only":           # the group that holds channel C1 sums its x channels only
            v2 = torch.where((c_ // Cg == C1 // Cg), torch.zeros_like(v2), v2)
        v = torch.where(c_ < C1, v, v2)
    if mut == "second_vector_dropped":
        v = torch.where(c_ >= 2048, torch.zeros_like(v), v)
    return gn_sums64(v.view(N, len(pix), G, Cg))


def gn_names():
    names = {}
    for C, G in GN_CG:
        for HW in GN_HW + (GN_HW_EXTRA[C],):
            if HW in GN_HW and HW == GN_HW_EXTRA[C]:
                continue
            for N in (1, 3):
                names[f"gn_C{C}_G{G}_HW{HW}_N{N}"] = dict(N=N, HW=HW, C=C, G=G, seed=3000 + len(names))
        if (C, G) in GN_TWO:
            for HW in (7, GN_HW_EXTRA[C]):
                names[f"gn2_C{C}_G{G}_HW{HW}_N3"] = dict(N=3, HW=HW, C=C, G=G, C1=GN_TWO[(C, G)],
                                                         seed=3000 + len(names))
    return names


GN_CASES = gn_names()


def make_gn(name):
    return made(("gn", name), lambda: gn_case(name, **GN_CASES[name]))


# ----------------------------------------------------------------------------- grid-stride kernels: trips
def trip_mutant(before, want, item, cap, mut):
    """``want`` as a grid-stride loop with a mistake leaves it: ``item`` is, per element of the buffer, the loop
    index i that writes it (-1: none).  skip_second_trip: items cap <= i < 2 cap keep what the buffer held."""
    assert mut == "skip_second_trip"
    skipped = (item >= cap) & (item < 2 * cap)
    assert bool(skipped.any()), "the case has no second trip"
    return torch.where(skipped, before, want)


# ----------------------------------------------------------------------------- gated_act / bias_act / embedding
def gated_case(name, rows, F, seed, act=None, smooth=False):
    """x [rows, 2 F] strided (ld 2 F + 8) between poison rows; integers (exact: relu) or bf16 normals (smooth)."""
    g = _gen(seed)
    c = Case(name, kind="gated", rows=rows, F=F, act=act, smooth=smooth)
    x = torch.randn(rows, 2 * F, generator=g).to(BF16).float() * 2 if smooth else _ints(g, -8, 8, rows, 2 * F)
    c.add("x", *embed_rows(g, x, 1, 1, 2 * F + 8))
    return c


def gated_want(c, gate_first):
    x = c.f64("x")
    a, gt = x[:, :c.F], x[:, c.F:]
    y = ge.act64(a, c.act) * gt if gate_first else a * ge.act64(gt, c.act)
    return y, (a * gt).abs()


def gated_items(c):
    r, col = torch.arange(c.rows)[:, None], torch.arange(c.F)[None, :]
    return r * (c.F // 8) + col // 8


def bias_act_case(name, rows, D, seed, act=None, alpha=0.5, bias=True, residual=True, smooth=False):
    g = _gen(seed)
    c = Case(name, kind="bias_act", rows=rows, D=D, act=act, alpha=alpha, smooth=smooth)
    mk = (lambda *s: torch.randn(*s, generator=g).to(BF16).float() * 2) if smooth else (lambda *s: _ints(g, -8, 8, *s))
    c.add("x", *embed_rows(g, mk(rows, D), 1, 1))
    if bias:
        c.add("bias", *embed_vec(g, mk(D)))
    if residual:
        c.add("residual", *embed_rows(g, mk(rows, D), 1, 1))
    return c


def bias_act_want(c):
    z = c.f64("x") * c.alpha
    zabs = z.abs()
    if c.has("bias"):
        z, zabs = z + c.f64("bias"), zabs + c.f64("bias").abs()
    y = ge.act64(z, c.act)
    if c.has("residual"):
        y, zabs = y + c.f64("residual"), zabs + c.f64("residual").abs()
    return y, zabs


def embedding_case(name, T, D, seed, vocab=50):
    g = _gen(seed)
    c = Case(name, kind="embedding", T=T, D=D, vocab=vocab)
    c.add("table", *embed_rows(g, _ints(g, -100, 100, vocab, D), 1, 1))
    c.ids = torch.randint(0, vocab, (T,), generator=g, dtype=torch.int32)
    return c


def flat8_items(rows, D):
    return (torch.arange(rows * D) // 8).view(rows, D)


# ----------------------------------------------------------------------------- rope / rope_pairs
def rope_case(name, T, H, Dh, rot, neox, seed, Hkv=0, max_pos=40):
    """q [T, H, Dh] as a view of packed rows [T, (H + 2 Hkv) Dh] (+ 8 padding columns) between poison rows; the k / v
    columns hold integers that must not change."""
    g = _gen(seed)
    c = Case(name, kind="rope", T=T, H=H, Dh=Dh, rot=rot, neox=neox, Hkv=Hkv)
    W = (H + 2 * Hkv) * Dh
    c.add("x", *embed_rows(g, _ints(g, -8, 8, T, W), 1, 1, W + 8))
    _add_table(c, g, max_pos, rot // 2)
    c.pos = torch.randint(0, max_pos, (T,), generator=g, dtype=torch.int32)
    return c


def rope_view(c, xrows):
    """[T, H, Dh] view of the packed rows' q columns."""
    return xrows[:, :c.H * c.Dh].unflatten(1, (c.H, c.Dh))


def _table_flat(c, name):
    return c.bufs[name].double().flatten(), c.off(name)


def rope_model(c, mut=None, items=False):
    """rope_kernel by flat index (fp64): the full buffer after the call; ``items``: the loop index per element."""
    T, H, Dh, rot = c.T, c.H, c.Dh, c.rot
    half = rot // 2
    flat = c.bufs["x"].double().flatten().clone()
    neox = True if mut == "neox_for_pairs" else c.neox
    jn = Dh // 2 if mut == "past_rot" else half
    ts = H * Dh if mut == "tok_stride" else c.view("x").stride(0)
    t, h, j = torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(jn), indexing="ij")
    base = c.off("x") + t * ts + h * Dh
    i0, i1 = (base + j, base + j + half) if neox else (base + 2 * j, base + 2 * j + 1)
    if items:
        it = torch.full((flat.numel(),), -1, dtype=torch.long)
        i = (t * H + h) * half + j
        it[i0], it[i1] = i, i
        return it.view(c.bufs["x"].shape)
    cs = Dh // 2 if mut == "cos_stride" else half
    p = c.pos.long()[t]
    cf, co = _table_flat(c, "cos")
    sf, so = _table_flat(c, "sin")
    ci = (p * cs + j)
    cv, sv = cf[(co + ci).clamp_max(cf.numel() - 1)], sf[(so + ci).clamp_max(sf.numel() - 1)]
    a, b = flat[i0], flat[i1]
    flat[i0], flat[i1] = a * cv - b * sv, b * cv + a * sv
    return flat.view(c.bufs["x"].shape)


def rope_pairs_case(name, B, T, H, Dh, seed):
    """x [B, T, H, Dh] with a batch stride of (T + 1) rows and a token stride of H Dh + 8."""
    g = _gen(seed)
    c = Case(name, kind="rope_pairs", B=B, T=T, H=H, Dh=Dh)
    W = H * Dh
    buf = _poison(g, B, T + 1, W + 8)
    buf[:, :T, :W] = _ints(g, -8, 8, B, T, W)
    c.add("x", buf, (slice(None), slice(0, T), slice(0, W)))
    _add_table(c, g, T, Dh // 2)
    return c


def rope_pairs_want(c):
    x = c.bufs["x"].double().clone()
    v = x[:, :c.T, :c.H * c.Dh].reshape(c.B, c.T, c.H, c.Dh)
    co, si = c.f64("cos")[None, :, None, :], c.f64("sin")[None, :, None, :]
    a, b = v[..., 0::2].clone(), v[..., 1::2].clone()
    v[..., 0::2], v[..., 1::2] = a * co - b * si, b * co + a * si
    x[:, :c.T, :c.H * c.Dh] = v.reshape(c.B, c.T, -1)
    return x


def rope_pairs_items(c):
    it = torch.full(c.bufs["x"].shape, -1, dtype=torch.long)
    b, t, w = torch.meshgrid(torch.arange(c.B), torch.arange(c.T), torch.arange(c.H * c.Dh), indexing="ij")
    it[:, :c.T, :c.H * c.Dh] = ((b * c.T + t) * c.H + w // c.Dh) * (c.Dh // 8) + (w % c.Dh) // 8
    return it


# ----------------------------------------------------------------------------- kv_write / rope_qkv_cache
def _slots(g, T, nblocks, neg_every=7):
    s = torch.randperm(nblocks * 64, generator=g)[:T].to(torch.int32)
    s[::neg_every] = -1
    return s


def cache_bufs(nblocks, Hkv, D):
    """A contiguous sentinel cache [nblocks, Hkv, 64, D] between a sentinel block before and behind."""
    return torch.full((nblocks + 2, Hkv, 64, D), SENTINEL, dtype=BF16), (slice(1, 1 + nblocks),)


def kvw_case(name, T, Hkv, D, seed):
    g = _gen(seed)
    c = Case(name, kind="kvw", T=T, Hkv=Hkv, D=D, nblocks=(T + 63) // 64 + 1)
    for n in ("k", "v"):
        c.add(n, *embed_rows(g, _ints(g, -100, 100, T, Hkv * D), 1, 1, Hkv * D + 8))
    c.slots = _slots(g, T, c.nblocks)
    return c


def kv_scatter(c, cache, src, mut=None, items=None):
    """src [T, Hkv, D] fp64 into the flat cache by the kernels' destination arithmetic."""
    T, Hkv, D = src.shape
    t, h, e = torch.meshgrid(torch.arange(T), torch.arange(Hkv), torch.arange(D), indexing="ij")
    slot = c.slots.long()[t]
    ok = slot >= 0
    if mut == "slot_neg_written":
        ok, slot = torch.ones_like(ok), slot.clamp_min(0)
    blk, off = slot >> 6, slot & 63
    if mut == "block_offset_confused":
        blk, off = (slot & 63) % c.nblocks, (slot >> 6) % 64
    if mut == "v_second8_dropped":
        ok = ok & (e % 16 < 8)
    dst = ((blk * Hkv + h) * 64 + off) * D + e
    flat = cache.view(-1)
    flat[dst[ok]] = src[ok]
    if items is not None:
        items[0].view(-1)[dst[ok]] = items[1][ok]


def kvw_want(c, mut=None, want_items=False):
    """(k cache, v cache) fp64 [nblocks, Hkv, 64, D] (sentinel where nothing is written)."""
    out = []
    for n in ("k", "v"):
        cache = torch.full((c.nblocks, c.Hkv, 64, c.D), SENTINEL, dtype=torch.float64)
        src = c.f64(n).reshape(c.T, c.Hkv, c.D)
        it = None
        if want_items:
            t, h, e = torch.meshgrid(torch.arange(c.T), torch.arange(c.Hkv), torch.arange(c.D), indexing="ij")
            it = (torch.full(cache.shape, -1, dtype=torch.long), (t * c.Hkv + h) * (c.D // 8) + e // 8)
        kv_scatter(c, cache, src, mut if (n == "v" or mut != "v_second8_dropped") else None, it)
        out.append(it[0] if want_items else cache)
    return out


def rqc_case(name, T, H, Hkv, D, seed, max_pos=40):
    g = _gen(seed)
    c = Case(name, kind="rqc", T=T, H=H, Hkv=Hkv, D=D, nblocks=(T + 63) // 64 + 1)
    W = (H + 2 * Hkv) * D
    c.add("x", *embed_rows(g, _ints(g, -8, 8, T, W), 1, 1, W + 8))
    _add_table(c, g, max_pos, D // 2)
    c.pos = torch.randint(0, max_pos, (T,), generator=g, dtype=torch.int32)
    c.slots = _slots(g, T, c.nblocks)
    return c


def rqc_model(c, mut=None, chunk=4096):
    """rope_qkv_cache: (qkv full buffer, k cache, v cache) fp64; q rotated in place, rotated k and v scattered."""
    T, H, Hkv, D = c.T, c.H, c.Hkv, c.D
    half = D // 2
    full = c.bufs["x"].double().clone()
    kc = torch.full((c.nblocks, Hkv, 64, D), SENTINEL, dtype=torch.float64)
    vc = kc.clone()
    cos, sin = c.f64("cos"), c.f64("sin")
    all_slots = c.slots
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        rows = full[1 + t0:1 + t1, :(H + 2 * Hkv) * D].reshape(t1 - t0, H + 2 * Hkv, D)
        p = c.pos.long()[t0:t1]
        co, si = cos[p][:, None, :], sin[p][:, None, :]
        qk = rows[:, :H + Hkv]
        a, b = qk[..., :half], qk[..., half:]
        rot = torch.cat([a * co - b * si, b * co + a * si], -1)
        c.slots = all_slots[t0:t1]
        kv_scatter(c, kc, qk[:, H:] if mut == "k_unrotated" else rot[:, H:],
                   mut if mut in ("slot_neg_written", "block_offset_confused") else None)
        kv_scatter(c, vc, rows[:, H + Hkv:], mut)
        full[1 + t0:1 + t1, :H * D] = rot[:, :H].reshape(t1 - t0, H * D)
    c.slots = all_slots
    return full, kc, vc


def rqc_items(c):
    """Loop index per element of (qkv full buffer, k cache, v cache): int32, -1 where nothing is written."""
    T, H, Hkv, D = c.T, c.H, c.Hkv, c.D
    heads, ph, half = H + 2 * Hkv, D // 16, D // 2
    full = torch.full(c.bufs["x"].shape, -1, dtype=torch.int32)
    t, hh, e = torch.meshgrid(torch.arange(T, dtype=torch.int32), torch.arange(heads, dtype=torch.int32),
                              torch.arange(D, dtype=torch.int32), indexing="ij")
    i = (t * heads + hh) * ph + torch.where(hh >= H + Hkv, e // 16, (e % half) // 8)
    full[1:1 + T, :H * D] = i[:, :H].reshape(T, H * D)
    out = [full]
    for lo in (H, H + Hkv):
        it = torch.full((c.nblocks, Hkv, 64, D), -1, dtype=torch.int32)
        cache = torch.zeros(it.shape, dtype=torch.float64)
        kv_scatter(c, cache, torch.zeros(T, Hkv, D, dtype=torch.float64), None, (it, i[:, lo:lo + Hkv]))
        out.append(it)
    return out


# ----------------------------------------------------------------------------- sched_step / softmax / token_feedback
def sched_case(name, n, seed, cfg, pred, B=0, guidance=7.5):
    """latents [n] (or [B, n / B]) and model_out [(2) n] contiguous between poison rows of 8; pred 2: integers, dt
    dyadic; pred 0 / 1: bf16 normals."""
    g = _gen(seed)
    c = Case(name, kind="sched", n=n, cfg=cfg, pred=pred, B=B, guidance=guidance, a_t=0.5625, a_prev=0.765625, dt=-0.25)
    mk = (lambda *s: _ints(g, -8, 8, *s)) if pred == 2 else (lambda *s: torch.randn(*s, generator=g).to(BF16).float())
    c.add("lat", *embed_vec(g, mk(n)))
    c.add("mo", *embed_vec(g, mk(2 * n if cfg else n)))
    if B:
        rp = torch.tensor([[0.25 + 0.0625 * b, 0.5 + 0.0625 * b, -0.125 * (b + 1)] for b in range(B)])
        rp[1::3, 0] = -1.0       # idle rows
        c.rows_params = rp
    return c


def sched_want(c):
    """(y64 [n], sum of |terms| [n], active mask [n])."""
    n = c.n
    x, e = c.f64("lat"), c.f64("mo")
    if c.cfg:
        eabs = e[:n].abs() + abs(c.guidance) * (e[n:].abs() + e[:n].abs())
        e = e[:n] + c.guidance * (e[n:] - e[:n])
    else:
        eabs = e.abs()
    if c.B:
        rp = c.rows_params.double().repeat_interleave(n // c.B, 0)
        a_t, a_prev, dt = rp[:, 0], rp[:, 1], rp[:, 2]
        active = a_t >= 0
        a_t = a_t.clamp_min(0.25)
    else:
        a_t, a_prev, dt = (torch.full((n,), v, dtype=torch.float64) for v in (c.a_t, c.a_prev, c.dt))
        active = torch.ones(n, dtype=torch.bool)
    if c.pred == 2:
        y, terms = x + dt * e, x.abs() + dt.abs() * eabs
    else:
        sa, s1a, sp, s1p = a_t.sqrt(), (1 - a_t).sqrt(), a_prev.sqrt(), (1 - a_prev).sqrt()
        if c.pred == 0:
            y = sp * (x - s1a * e) / sa + s1p * e
            terms = sp * (x.abs() + s1a * eabs) / sa + s1p * eabs
        else:
            y = sp * (sa * x - s1a * e) + s1p * (sa * e + s1a * x)
            terms = sp * (sa * x.abs() + s1a * eabs) + s1p * (sa * eabs + s1a * x.abs())
    return torch.where(active, y, x), terms, active


def sched_step_mutant(c, mut):
    """pred 2 with the loop stepping by gridDim.x only: item i runs min(i, cap - 1) // 2048 + 1 times (in place)."""
    assert mut == "step_griddim" and c.pred == 2 and not c.B
    y, _, _ = sched_want(c)
    x = c.f64("lat")
    i = torch.arange(c.n) // 8
    times = (i.clamp_max(CAP - 1) // 2048 + 1).double()
    return x + times * (y - x)


def softmax_case(name, rows, D, seed, scale=0.5):
    """bf16 logits in [-20, 20) (scaled spread <= 20) between poison rows."""
    g = _gen(seed)
    c = Case(name, kind="softmax", rows=rows, D=D, scale=scale)
    c.add("x", *embed_rows(g, (torch.rand(rows, D, generator=g) * 40 - 20).to(BF16).float(), 1, 1))
    return c


GRID_CASES = {
    # small odd shapes, and > 2 x the grid cap in loop items (three trips), the latter all exact
    "gated_small": (gated_case, dict(rows=37, F=72, act="relu", seed=4001)),
    "gated_small_silu": (gated_case, dict(rows=37, F=72, act="silu", smooth=True, seed=4002)),
    "gated_small_gelu": (gated_case, dict(rows=37, F=72, act="gelu", smooth=True, seed=4003)),
    "gated_big": (gated_case, dict(rows=2057, F=4096, act="relu", seed=4004)),           # 1 053 184 items
    "bias_act_small": (bias_act_case, dict(rows=37, D=72, seed=4011)),
    "bias_act_small_plain": (bias_act_case, dict(rows=37, D=72, bias=False, residual=False, alpha=2.0, seed=4012)),
    "bias_act_small_silu": (bias_act_case, dict(rows=37, D=72, act="silu", smooth=True, seed=4013)),
    "bias_act_small_gelu": (bias_act_case, dict(rows=37, D=72, act="gelu", smooth=True, residual=False, seed=4014)),
    "bias_act_big": (bias_act_case, dict(rows=4099, D=2056, seed=4015)),                  # 1 053 443 items
    "embedding_small": (embedding_case, dict(T=37, D=72, seed=4021)),
    "embedding_big": (embedding_case, dict(T=1031, D=8192, seed=4022)),                   # 1 055 744 items
    "rope_small_neox": (rope_case, dict(T=37, H=3, Dh=64, rot=64, neox=True, Hkv=1, seed=4031)),
    "rope_small_pairs": (rope_case, dict(T=37, H=3, Dh=64, rot=64, neox=False, Hkv=1, seed=4032)),
    "rope_small_neox_half": (rope_case, dict(T=37, H=3, Dh=64, rot=32, neox=True, Hkv=1, seed=4033)),
    "rope_small_pairs_half": (rope_case, dict(T=37, H=3, Dh=64, rot=32, neox=False, Hkv=1, seed=4034)),
    "rope_big": (rope_case, dict(T=1031, H=16, Dh=128, rot=128, neox=True, Hkv=1, seed=4035)),   # 1 055 744 items
    "rope_pairs_small": (rope_pairs_case, dict(B=3, T=37, H=3, Dh=64, seed=4041)),
    "rope_pairs_big": (rope_pairs_case, dict(B=8, T=517, H=32, Dh=64, seed=4042)),        # 1 058 816 items
    "kvw_small": (kvw_case, dict(T=37, Hkv=3, D=64, seed=4051)),
    "kvw_big": (kvw_case, dict(T=8200, Hkv=8, D=128, seed=4052)),                         # 1 049 600 items
    "rqc_small_64": (rqc_case, dict(T=37, H=4, Hkv=2, D=64, seed=4061)),
    "rqc_small_128": (rqc_case, dict(T=37, H=6, Hkv=2, D=128, seed=4062)),
    "rqc_big": (rqc_case, dict(T=65600, H=2, Hkv=1, D=128, seed=4063)),                   # 2 099 200 items
    "sched_small": (sched_case, dict(n=8 * 37, cfg=True, pred=2, seed=4071)),
    "sched_small_nocfg": (sched_case, dict(n=8 * 37, cfg=False, pred=2, seed=4072)),
    "sched_small_eps": (sched_case, dict(n=8 * 37, cfg=True, pred=0, seed=4073)),
    "sched_small_v": (sched_case, dict(n=8 * 37, cfg=False, pred=1, seed=4074)),
    "sched_big": (sched_case, dict(n=8 * 1048700, cfg=True, pred=2, seed=4075)),          # 1 048 700 items
    "sched_rows_small": (sched_case, dict(n=5 * 8 * 37, B=5, cfg=True, pred=2, seed=4081)),
    "sched_rows_small_eps": (sched_case, dict(n=5 * 8 * 37, B=5, cfg=False, pred=0, seed=4082)),
    "sched_rows_small_v": (sched_case, dict(n=5 * 8 * 37, B=5, cfg=True, pred=1, seed=4083)),
    "sched_rows_big": (sched_case, dict(n=5 * 8 * 209741, B=5, cfg=True, pred=2, seed=4084)),   # 1 048 705 items
}
for _D in (8, 2048, 2056, 4096):
    GRID_CASES[f"softmax_D{_D}"] = (softmax_case, dict(rows=5, D=_D, seed=4090 + _D))
BIG = [n for n in GRID_CASES if n.endswith("_big")]


def make_grid(name):
    fn, kw = GRID_CASES[name]
    return made(("grid", name), lambda: fn(name, **kw))


def grid_items(c):
    """Number of loop items of the case's kernel launch."""
    k = c.kind
    if k == "gated":
        return c.rows * (c.F // 8)
    if k == "bias_act":
        return c.rows * (c.D // 8)
    if k == "embedding":
        return c.T * (c.D // 8)
    if k == "rope":
        return c.T * c.H * (c.rot // 2)
    if k == "rope_pairs":
        return c.B * c.T * c.H * (c.Dh // 8)
    if k == "kvw":
        return c.T * c.Hkv * (c.D // 8)
    if k == "rqc":
        return c.T * (c.H + 2 * c.Hkv) * (c.D // 16)
    if k == "sched":
        return c.n // 8
    raise ValueError(k)
