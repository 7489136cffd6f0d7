"""Inputs for which the GEMM and conv kernels must be bit-exact, an fp64 oracle, the zero-tolerance rule and mutants.

Plain helper functions for tests/test_gemm_exact_{cpu,gpu}.py and tests/gemm_exact_worker.py (no fixtures, no pytest
settings).

Why: the suite judges every GEMM / conv kernel by a relative Frobenius error (< 1e-2 / < 2e-2) or by close() with a
0.1 % allowance.  Both average over the tensor: one wrong row, one column quad without its bias, one image corner that
reads a neighbour pass.  Here the operands are small integers (x in -3..3, w in -2..2, bias / temb / residual in
-8..8, gate in {-2, -1, 1, 2}, alpha / res_alpha in {1, 0.5, 2}) with sum_k |x||w| |alpha| + |bias| + |temb| +
|res_alpha residual| < 2^24 for every output element.  Every fp32 operation of the kernels (MFMA accumulation in any
order, split-K slabs, skinny partials, the epilogue's acc * alpha + bias, * gate, + res_alpha * residual) is then exact,
and the one rounding to bf16 (RNE) makes the output equal bf16(fp64 result) bit for bit: tolerance zero, every element
compared, whatever the tile shape, split count or MFMA order.

Every operand is a view into a larger buffer of +-1024 ("poison": finite, so only a read that contributes shows), and
a GEMM output is a view ``buf[r0:r0 + M, :N]`` of a buffer prefilled with a sentinel ("canaries") that must survive.

Smooth activations (SiLU, GELU) are not exact; their few cases use |y - y64| <= ulp_bf16(y64) + 1e-6 |z| with the
exact pre-activation z (for a GLU pair z = value * gate pre-activation): one bf16 ulp covers any fp32 evaluation with a
relative error below 2^-9 plus the final rounding, the absolute term the 1.5e-7 erf bound documented in
csrc/kernels/common.h (times |z| / 2) and the fp32 relative error of the SiLU quotient.
"""
import math

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn
POISON = 1024.0
POISON_F8 = 256.0
SENTINEL = 24576.0          # exact in bf16, far above any |output| of a committed case
LIMIT = float(2 ** 24)
TOTALS = {"compared": 0, "canaries": 0, "poison": 0}   # what the checks of this process have looked at


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _gates(g, *shape):
    return torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, shape, generator=g)]


def _poison(g, *shape, value=POISON):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * value


class Case:
    """Operands by name: ``bufs[name]`` is the poison buffer, ``idx[name]`` the index of the operand's view in it."""

    def __init__(self, name, **meta):
        self.name = name
        self.bufs, self.idx, self.dtype = {}, {}, {}
        self.__dict__.update(meta)

    def add(self, name, buf, idx, dtype=BF16):
        self.bufs[name], self.idx[name], self.dtype[name] = buf.to(dtype), idx, dtype

    def has(self, name):
        return name in self.bufs

    def view(self, name):
        """The operand on the CPU (a view of its poison buffer), None if the case has none."""
        return self.bufs[name][self.idx[name]] if name in self.bufs else None

    def f64(self, name):
        v = self.view(name)
        return None if v is None else v.double()

    def place(self, device):
        """{name: view} with every buffer copied to ``device`` (the views alias the copies as on the CPU)."""
        out = {}
        for name, buf in self.bufs.items():
            b = buf.to(device)
            out[name] = b[self.idx[name]]
            out["_" + name] = b
        return out

    def poison_count(self):
        return sum(b.numel() - b[self.idx[n]].numel() for n, b in self.bufs.items())


def embed_rows(g, t, before, after, ld=None, value=POISON):
    """t [..., R, C] as the view buf[..., before:before + R, :C] of a poison buffer [..., before + R + after, ld]."""
    *lead, R, C = t.shape
    ld = ld or C
    buf = _poison(g, *lead, before + R + after, ld, value=value)
    idx = tuple([slice(None)] * len(lead) + [slice(before, before + R), slice(0, C)])
    buf[idx] = t
    return buf, idx


def embed_vec(g, t, before=8, after=8):
    """t [n] at a 16-byte aligned offset of a poison vector."""
    buf = _poison(g, before + t.numel() + after)
    buf[before:before + t.numel()] = t
    return buf, (slice(before, before + t.numel()),)


def embed_lead(g, t, before=1, after=1):
    """t [n, ...] (contiguous) between poison slices along dim 0: images of a batch, weight slices."""
    buf = _poison(g, before + t.shape[0] + after, *t.shape[1:])
    buf[before:before + t.shape[0]] = t
    return buf, (slice(before, before + t.shape[0]),)


def embed_cols(g, t, before=8, after=8):
    """t [R, C] as a column slice of a wider poison matrix (row stride a multiple of 8)."""
    R, C = t.shape
    width = (before + C + after + 7) // 8 * 8
    buf = _poison(g, R, width)
    buf[:, before:before + C] = t
    return buf, (slice(None), slice(before, before + C))


# ----------------------------------------------------------------------------- activations, the two rules
def act64(z, act):
    if act is None:
        return z
    if act == "relu":
        return z.clamp_min(0)
    if act == "silu":
        return z * torch.sigmoid(z)
    if act == "gelu":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    raise ValueError(act)


def to_bf16_exact(y64):
    """bf16(fp64 result), one rounding: the value must be an fp32 number already (it is, below 2^24)."""
    y32 = y64.float()
    assert bool((y32.double() == y64).all()), "the fp64 result is not an fp32 number: the case is not exact"
    return y32.to(BF16)


def ulp_bf16(v):
    """Spacing of bf16 at |v| (fp64 in, fp64 out; 0 at 0)."""
    _, e = torch.frexp(v.abs())
    u = torch.ldexp(torch.ones_like(v), (e - 8).clamp_min(-133))
    return torch.where(v == 0, torch.zeros_like(v), u)


def _report(got, want, bad, what, n_show=5):
    idx = bad.nonzero()[:n_show].tolist()
    shown = ", ".join(f"{tuple(i)}: got {float(got[tuple(i)]):.6g}, want {float(want[tuple(i)]):.6g}" for i in idx)
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first {shown}"


def assert_exact(got, want, what=""):
    """torch.equal, every element; on a miss the count and the first few (index, got, want)."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    TOTALS["compared"] += got.numel()
    want = want.to(got.device)
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    raise AssertionError(_report(g, w, ~(g == w), what))


def assert_canaries(outbuf, full_want, what=""):
    """The whole output buffer: the view holds the result, everything around it still the sentinel."""
    full_want = full_want.to(outbuf.device)
    TOTALS["canaries"] += int((full_want == SENTINEL).sum())
    if torch.equal(outbuf, full_want):
        return
    g, w = outbuf.double(), full_want.double()
    hit = (w == SENTINEL) & ~(g == w)
    if bool(hit.any()):
        raise AssertionError(_report(g, w, hit, f"{what}: canary overwritten"))
    raise AssertionError(_report(g, w, ~(g == w), what))


def assert_smooth(got, y64, zabs, what=""):
    """|y - y64| <= ulp_bf16(y64) + 1e-6 |z|, every element."""
    TOTALS["compared"] += got.numel()
    g = got.double().cpu()
    assert g.shape == y64.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(y64.shape)}"
    bad = ~((g - y64).abs() <= ulp_bf16(y64) + 1e-6 * zabs)
    if bool(bad.any()):
        raise AssertionError(_report(g, y64, bad, what))


def frobenius(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


def close_bad_share(a, b, atol=5e-2, rtol=2e-2):
    """Share of elements outside close()'s tolerance (tests/test_kernels_gpu.py accepts < 1e-3)."""
    a, b = a.float(), b.float()
    return ((a - b).abs() > atol + rtol * b.abs()).float().mean().item()


# ----------------------------------------------------------------------------- GEMM cases
def _ld8(n):
    """A row stride behind n columns: the next multiple of 8 plus 8 (the view's rows stay 16-byte aligned)."""
    return (n + 7) // 8 * 8 + 8


def gemm_case(name, M, N, K, seed, B=0, bias=False, residual=None, alpha=1.0, res_alpha=1.0, rows_per_gate=0,
              glu=False, sparse=False, residual_rows=0, slices=0, fp8=False, x_after=8, ldcs=None, bias_lo=-8,
              mx=False):
    """x [M, K] (or [B, M, K]) and w [N, K] as views with poison rows behind M / N and poison columns behind K
    (lda = K + 8, ldw = K + 16); bias [N] inside a poison vector; residual "own" ([M or residual_rows, N'] with ldr >=
    N' + 8, a multiple of 8) or "inplace" (the output view starts as the residual); gate [rows / rows_per_gate, N'].
    slices > 0:
    ``linear_wslices`` weights [slices, N, K] between poison slices and a per-slice bias.  fp8: w8 integer-valued e4m3
    = w * 2^k with w_scale = 2^-k per row (k in 0..2), ldw = K + 16 bytes.  mx: w drawn from the signed e2m1 grid times
    2^e (e in {0, 1} per group of 32), which ``quantize_mxfp4`` round-trips; the kernel takes the packed pair
    (``c.wq``, ``c.w_scale``: contiguous, as the binding requires), the oracle the same values as "w"."""
    g = _gen(seed)
    lo = 1 if sparse else 3
    c = Case(name, kind="gemm", M=M, N=N, K=K, B=B, alpha=alpha, res_alpha=res_alpha, rows_per_gate=rows_per_gate,
             glu=glu, residual_rows=residual_rows, slices=slices, fp8=fp8, sparse=sparse, w_scale=None, mx=mx,
             No=N // 2 if glu else N)
    lead = (B,) if B else ()
    c.add("x", *embed_rows(g, _ints(g, -lo, lo, *lead, M, K), 0, x_after, K + 8))
    wl = 1 if sparse else 2
    if slices:
        c.add("w", *embed_lead(g, _ints(g, -wl, wl, slices, N, K)))
        c.add("bias2d", *embed_rows(g, _ints(g, -8, 8, slices, N), 1, 1, N + 8))
    elif fp8:
        w = _ints(g, -wl, wl, N, K)
        k = torch.randint(0, 3, (N,), generator=g)
        c.w_int = w
        c.w_scale = torch.ldexp(torch.ones(N), -k)
        c.add("w", *embed_rows(g, w * torch.ldexp(torch.ones(N), k)[:, None], 1, 1, K + 16, value=POISON_F8), dtype=F8)
    elif mx:
        from shai_amd.ops import reference as ref
        grid = torch.tensor(ref.MXFP4_VALUES + tuple(-v for v in ref.MXFP4_VALUES[1:]))
        w = grid[torch.randint(0, len(grid), (N, K), generator=g)]
        e = torch.randint(0, 2, (N, K // 32, 1), generator=g)
        w = (w.view(N, K // 32, 32) * torch.ldexp(torch.ones(N, K // 32, 1), e)).view(N, K)
        c.wq, c.w_scale = ref.quantize_mxfp4(w)
        c.add("w", *embed_rows(g, w, 1, 1, K + 16))
    else:
        c.add("w", *embed_rows(g, _ints(g, -wl, wl, N, K), 1, 1, K + 16))
    if bias:
        c.add("bias", *embed_vec(g, _ints(g, bias_lo, 8, N)))
    if residual is not None:
        rr = residual_rows or M
        c.add("residual", *embed_rows(g, _ints(g, -8, 8, *lead, rr, c.No), 1, 1, _ld8(c.No)))
    c.res_inplace = residual == "inplace"
    if rows_per_gate:
        rows = (B or 1) * M
        c.add("gate", *embed_rows(g, _gates(g, (rows + rows_per_gate - 1) // rows_per_gate, c.No), 1, 1, _ld8(c.No)))
    c.ldcs = ldcs or [c.No]
    return c


def gemm_weight64(c):
    """The weights as the kernel must read them, fp64 [N, K] ([slices, N, K])."""
    if c.fp8:
        return c.f64("w") * c.w_scale.double()[:, None]
    return c.f64("w")


def gemm_z64(c, x=None, w=None, bias=None):
    """alpha * x w^T + bias (+ the slice's bias2d): the exact pre-activation, fp64 [.., M, N]."""
    x = c.f64("x") if x is None else x
    w = gemm_weight64(c) if w is None else w
    if c.slices:
        z = torch.einsum("smk,snk->smn", x.view(c.slices, c.M // c.slices, c.K), w)
        return (z + c.f64("bias2d")[:, None, :]).reshape(c.M, c.N)
    z = c.alpha * torch.matmul(x, w.t())
    bias = c.f64("bias") if bias is None else bias
    return z if bias is None else z + bias


def gemm_finish64(c, z, act=None, gate_rows=None, residual=None):
    """The epilogue after the pre-activation, fp64: activation (GLU: value * act(gate)), * gate row (gate_rows: the
    gate row of every flattened output row, default (b M + m) // rows_per_gate), + res_alpha * residual (broadcast
    over residual_rows)."""
    y = z[..., 0::2] * act64(z[..., 1::2], act) if c.glu else act64(z, act)
    if c.rows_per_gate:
        if gate_rows is None:
            gate_rows = torch.arange(y.numel() // y.shape[-1]) // c.rows_per_gate
        y = (y.reshape(-1, y.shape[-1]) * c.f64("gate")[gate_rows]).reshape(y.shape)
    r = c.f64("residual") if residual is None else residual
    if r is not None:
        if c.residual_rows:
            r = r[torch.arange(c.M) % c.residual_rows]
        y = y + c.res_alpha * r
    return y


def gemm_bound(c):
    """sum_k |x||w| |alpha| + |bias| (times |gate|) + |res_alpha residual|: below 2^24 for an exact case."""
    x, w = c.f64("x").abs(), gemm_weight64(c).abs()
    if c.slices:
        z = torch.einsum("smk,snk->smn", x.view(c.slices, c.M // c.slices, c.K), w)
        return float((z + c.f64("bias2d").abs()[:, None, :]).max())
    z = abs(c.alpha) * torch.matmul(x, w.t())
    if c.has("bias"):
        z = z + c.f64("bias").abs()
    if c.glu:
        z = z[..., 0::2] * z[..., 1::2].clamp_min(1)
    if c.rows_per_gate:
        z = z * 2
    if c.has("residual"):
        z = z + abs(c.res_alpha) * c.f64("residual").abs().max()
    return float(z.max())


def gemm_want(c, act=None):
    """(bf16 expected output, fp64 result, |z| of the smooth rule)."""
    z = gemm_z64(c)
    y = gemm_finish64(c, z, act)
    zabs = (z[..., 0::2] * z[..., 1::2]).abs() if c.glu else z.abs()
    exact = act in (None, "relu")
    return (to_bf16_exact(y) if exact else y.float().to(BF16)), y, zabs


def out_buffer(c, ldc, device, before=8, after=3):
    """(buffer, view): a sentinel buffer [.., before + M + after, ldc] and the output view [.., before:before + M, :N'];
    an in-place residual is copied into the view."""
    lead = (c.B,) if c.B else ()
    buf = torch.full((*lead, before + c.M + after, ldc), SENTINEL, dtype=BF16)
    idx = tuple([slice(None)] * len(lead) + [slice(before, before + c.M), slice(0, c.No)])
    if c.res_inplace:
        buf[idx] = c.view("residual")
    buf = buf.to(device)
    return buf, buf[idx], idx


def full_want(c, want, ldc, before=8, after=3):
    lead = (c.B,) if c.B else ()
    buf = torch.full((*lead, before + c.M + after, ldc), SENTINEL, dtype=BF16)
    buf[tuple([slice(None)] * len(lead) + [slice(before, before + c.M), slice(0, c.No)])] = want
    return buf


def col_partials64(y):
    """[M, N] fp64 -> [M / 128, N, 2] (sum, sum of squares) per 128-row block."""
    M, N = y.shape
    f = y.reshape(M // 128, 128, N)
    return torch.stack([f.sum(1), (f * f).sum(1)], -1)


def row_moments64(y, eps):
    mean = y.mean(-1)
    var = (y * y).mean(-1) - mean * mean
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], -1)


TAILS = dict(M=300, N=328, K=136, bias=True, residual="inplace", alpha=0.5, res_alpha=2.0)
SKINNY_M = (1, 33, 64)
GEMM_CASES = {
    # M tail (300 = 256 + 44), N tail on the wide store path (328 = 256 + 72, a multiple of 4), last K-tile of 8
    "tails": dict(TAILS, seed=1, ldcs=[328, 336, 333]),
    # one row past a 256-row tile, N not a multiple of 4; ldc 322 / 325: narrow stores, 324 / 328: wide stores up to
    # the ragged last quad (where a 16-byte store would hit the canaries behind column N)
    "narrow_store": dict(M=257, N=322, K=72, bias=True, residual="own", seed=2, ldcs=[322, 324, 328, 325]),
    # 258 row tiles (the last with 44 rows): the persistent configs walk more than one tile per workgroup
    "many_tiles": dict(M=65836, N=72, K=64, bias=True, seed=3, ldcs=[72, 77]),
    # strided 3-D views, rows_per_gate 150: the gate row is the flattened (b M + m) // 150
    "gate_batched": dict(B=3, M=300, N=384, K=256, bias=True, rows_per_gate=150, seed=4, ldcs=[384, 390]),
    # GroupNorm partials / LayerNorm moments of 1.5 row tiles (|y| <= 256: x, w in -1..1); 128 poison rows behind M.
    # The bias is drawn from 1..8, not -8..8: the moments' rule is relative (rtol 1e-5), and the kernels return the
    # mean as k0 + sum(y - k0) / N with k0 the row's first value (csrc/kernels/norm.hip row_moments_kernel: shifted
    # sums, so the variance does not cancel), whose absolute error is one fp32 ulp of |k0| -- measured 7.6e-7 on
    # the GPU, a relative 6.1e-5 of a row mean of 0.0125 with a zero-mean bias.  With row means of 2 and more nothing
    # cancels in the mean either, which is the premise of the relative rule.
    "stats_half_tile": dict(M=384, N=320, K=320, bias=True, residual="own", sparse=True, x_after=128, bias_lo=1,
                            seed=5),
    # the same on whole 256-row tiles: the shape at which the v4 epilogue itself writes the statistics (M % 256 == 0,
    # N a multiple of the 320-wide tile) -- at M = 384 a pass over the stored output does
    "stats_full_tiles": dict(M=512, N=320, K=320, bias=True, residual="own", sparse=True, bias_lo=1, seed=6),
    "bias2d_slices": dict(M=768, N=72, K=64, slices=3, seed=7),
    "res_rows": dict(M=512, N=320, K=320, bias=True, residual="own", residual_rows=256, res_alpha=2.0, seed=8),
    "res_rows_64": dict(M=512, N=320, K=320, bias=True, residual="own", residual_rows=64, seed=9),
    "ws_plain": dict(M=300, N=640, K=320, seed=10, ldcs=[640, 648]),
    "ws_bias": dict(M=300, N=640, K=320, bias=True, alpha=2.0, seed=11, ldcs=[640, 648]),
    "ws_residual": dict(M=300, N=640, K=320, bias=True, residual="inplace", res_alpha=0.5, seed=12, ldcs=[640, 648]),
    "glu_tails": dict(M=300, N=328, K=136, bias=True, glu=True, seed=13, ldcs=[164, 167]),
    "glu_ws": dict(M=300, N=640, K=320, bias=True, glu=True, seed=14, ldcs=[320]),
}
for _m in SKINNY_M:
    GEMM_CASES[f"skinny_{_m}"] = dict(M=_m, N=328, K=1096, bias=True, residual="own", alpha=0.5, res_alpha=2.0,
                                      seed=20 + _m, ldcs=[328, 333])
    # K 1096 -> 1104: the fp8 skinny path needs K % 16 == 0
    GEMM_CASES[f"skinny8_{_m}"] = dict(M=_m, N=328, K=1104, bias=True, residual="own", fp8=True, seed=120 + _m,
                                       ldcs=[328, 333])
# MXFP4: K 1096 -> 1088 (K % 32 == 0; 8.5 of the kernel's 128-wide K steps); the tile GEMM at (300, 328, 256)
GEMM_CASES["fp4_skinny_33"] = dict(M=33, N=328, K=1088, bias=True, residual="own", mx=True, seed=201, ldcs=[328, 333])
GEMM_CASES["fp4_tile"] = dict(M=300, N=328, K=256, bias=True, residual="own", alpha=0.5, res_alpha=2.0, mx=True,
                              seed=202, ldcs=[328, 333])
PARTIALS_CASES = ("stats_half_tile", "stats_full_tiles")
_made = {}


def make_gemm(name):
    """The committed GEMM case (CPU tensors), built once per name and shared, never modified."""
    if name not in _made:
        _made[name] = gemm_case(name, **GEMM_CASES[name])
    return _made[name]


# ----------------------------------------------------------------------------- conv cases
def conv_case(name, N, H, W, C, C2, Co, k, stride, pad, seed, kind="conv", temb=None, res=False, gn=False, norm=False,
              sparse=False, bias=True):
    """x (x2) [N, H, W, C] between a poison image before and behind the batch, each source in its own buffer; the
    packed weight [Co, k k Cin] between poison rows; temb [N, Co] between poison rows ("rows") or as a column slice
    of a wider poison matrix ("cols"); residual between poison images.  kind "up": nearest-2x upsample + 3x3, "up2":
    the same by output phase (``w_up2``).  norm: integer GroupNorm scale in {1, 2} / shift in -2..2 per (image,
    channel), as one [2, N, Cin] fp32 allocation."""
    g = _gen(seed)
    lo, wl = (1, 1) if sparse else (3, 2)
    up = kind != "conv"
    cin = C + C2
    OH = ((2 * H if up else H) + 2 * pad - k) // stride + 1
    OW = ((2 * W if up else W) + 2 * pad - k) // stride + 1
    c = Case(name, kind=kind, N=N, H=H, W=W, C=C, C2=C2, Co=Co, k=k, stride=stride, pad=pad, up=up, OH=OH, OW=OW,
             gn=gn, sparse=sparse, cin=cin)
    c.add("x", *embed_lead(g, _ints(g, -lo, lo, N, H, W, C)))
    if C2:
        c.add("x2", *embed_lead(g, _ints(g, -lo, lo, N, H, W, C2)))
    c.add("w", *embed_lead(g, _ints(g, -wl, wl, Co, k * k * cin)))
    if bias:
        c.add("bias", *embed_vec(g, _ints(g, -8, 8, Co)))
    if temb == "rows":
        c.add("temb", *embed_lead(g, _ints(g, -8, 8, N, Co)))
    elif temb == "cols":
        c.add("temb", *embed_cols(g, _ints(g, -8, 8, N, Co)))
    if res:
        c.add("residual", *embed_lead(g, _ints(g, -8, 8, N, OH, OW, Co)))
    if norm:
        ss = torch.stack([_ints(g, 1, 2, N, cin), _ints(g, -2, 2, N, cin)])
        c.add("norm", ss, (slice(None),), dtype=torch.float32)
    return c


def conv_input64(c, mut=None):
    """cat(x, x2) after the integer norm, fp64 [N, H, W, Cin] (the padding is added after this: it stays 0)."""
    x = c.f64("x")
    if c.C2:
        x2 = c.f64("x2")
        if mut == "concat_off8":   # the split 8 channels early: the second source starts at C - 8
            x = torch.cat([x[..., :c.C - 8], x2, torch.zeros(*x.shape[:-1], 8, dtype=x.dtype)], -1)
        else:
            x = torch.cat([x, x2], -1)
    if c.has("norm"):
        ss = c.view("norm").double()
        x = x * ss[0][:, None, None, :] + ss[1][:, None, None, :]
    return x


def conv_finish64(c, y):
    """+ bias + temb + residual on the fp64 conv result [N, OH, OW, Co]."""
    if c.has("bias"):
        y = y + c.f64("bias")
    if c.has("temb"):
        y = y + c.f64("temb")[:, None, None, :]
    if c.has("residual"):
        y = y + c.f64("residual")
    return y


def conv_y64(c, absolute=False):
    """The oracle: fp64 F.conv2d on the integers (absolute: the magnitude bound sum |x||w| + |bias| + ...)."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    x = f(conv_input64(c))
    if c.up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    w = f(c.f64("w")).reshape(c.Co, c.k, c.k, c.cin).permute(0, 3, 1, 2)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride=c.stride, padding=c.pad).permute(0, 2, 3, 1)
    if not absolute:
        return conv_finish64(c, y)
    for n in ("bias", "temb", "residual"):
        if c.has(n):
            t = c.f64(n).abs()
            y = y + (t[:, None, None, :] if n == "temb" else t)
    return y


def conv_model(c, mut=None, images=None):
    """The conv as an explicit-index im2col + GEMM in fp64, one switch per addressing mistake (``mut``); images: the
    output images to compute (default all).  Returns [len(images), OH, OW, Co] before bias / temb / residual."""
    x = conv_input64(c, mut)
    N, H, W, cin = x.shape
    Z = N * H * W                                   # the index of the zero row (padding)
    flat = torch.cat([x.reshape(Z, cin), torch.zeros(1, cin, dtype=x.dtype)])
    IH, IW = (2 * H, 2 * W) if c.up else (H, W)
    images = list(range(N)) if images is None else images
    n = torch.tensor(images).repeat_interleave(c.OH * c.OW)
    r = torch.arange(c.OH * c.OW).repeat(len(images))
    oy, ox = r // c.OW, r % c.OW
    cols = []
    for kh in range(c.k):
        for kw in range(c.k):
            iy = oy * c.stride - c.pad + kh + (1 if mut == "stride_origin" else 0)
            ix = ox * c.stride - c.pad + kw
            row_ok, col_ok = (iy >= 0) & (iy < IH), (ix >= 0) & (ix < IW)
            ok = row_ok & col_ok
            if c.up and mut == "upsample_src":
                sy, sx = ((iy + 1) // 2).clamp(0, H - 1), ((ix + 1) // 2).clamp(0, W - 1)
            elif c.up:
                sy, sx = iy // 2, ix // 2
            else:
                sy, sx = iy, ix
            idx = (n * H + sy) * W + sx
            if mut == "left_wrap":           # image 0: column -1 is the last pixel of the row above
                ok = ok | ((ix == -1) & row_ok & (n == 0) & (idx >= 0))
            if mut == "top_prev_image":      # row -1 is the last row of the image before
                ok = ok | ((iy == -1) & col_ok & (n > 0))
            if mut == "corner_leak" and kh == 0 and kw == 0:   # pixel (0, 0, 0)'s padded corner tap reads (0, 0, 0)
                first = (n == 0) & (oy == 0) & (ox == 0)
                idx, ok = torch.where(first, torch.zeros_like(idx), idx), ok | first
            a = flat[torch.where(ok, idx, torch.full_like(idx, Z))]
            if mut == "norm_pad":            # the norm's shift applied to the zero padding
                a = torch.where(ok[:, None], a, c.view("norm").double()[1][n])
            cols.append(a)
    w = c.f64("w")
    if mut == "taps_transposed":
        w = w.reshape(c.Co, c.k, c.k, cin).transpose(1, 2).reshape(c.Co, -1)
    y = torch.cat(cols, 1) @ w.t()
    return y.reshape(len(images), c.OH, c.OW, c.Co)


def phase_model(c, swap=False):
    """The upsample conv by output phase in fp64 (ops.reference.conv2d_up2_phases's arithmetic on the packed phase
    weights); swap: the phase's px / py exchanged when its weight slice is picked."""
    from shai_amd.ops import reference as ref
    x = c.f64("x")
    N, H, W, C = x.shape
    wp = ref.pack_up2_phase_weight(c.view("w"), C).double().reshape(2, 2, c.Co, 2, 2, C)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(N, 2 * H, 2 * W, c.Co, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            ws = wp[px, py] if swap else wp[py, px]
            acc = 0
            for a in range(2):
                for b in range(2):
                    acc = acc + xp[:, py + a:py + a + H, px + b:px + b + W] @ ws[:, a, b].t()
            y[:, py::2, px::2] = acc
    return y


CONV_CASES = {
    # four images share a 256-row tile, 64-row tail: a pad tap that wraps to the previous row / image fails
    # (a one-corner leak scores a relative Frobenius error of 0.017 - 0.023 here, depending on the draw; seed 231 is a
    # draw the suite's < 2e-2 accepts, which tests/test_gemm_exact_cpu.py shows)
    "image_edges": dict(N=5, H=8, W=8, C=64, C2=0, Co=64, k=3, stride=1, pad=1, seed=231),
    "stride2": dict(N=3, H=12, W=12, C=128, C2=0, Co=96, k=3, stride=2, pad=1, seed=32),
    "concat_unequal": dict(N=2, H=16, W=16, C=64, C2=128, Co=64, k=3, stride=1, pad=1, seed=33),
    "one_by_one_concat": dict(N=2, H=16, W=16, C=64, C2=64, Co=64, k=1, stride=1, pad=0, seed=34),
    "up_nine_taps": dict(N=2, H=8, W=8, C=128, C2=0, Co=64, k=3, stride=1, pad=1, kind="up", seed=35),
    "phase_groups": dict(N=4, H=8, W=8, C=64, C2=0, Co=64, k=3, stride=1, pad=1, kind="up2", gn=True, sparse=True,
                         seed=36),
    "phase_temb": dict(N=2, H=16, W=16, C=128, C2=0, Co=64, k=3, stride=1, pad=1, kind="up2", temb="cols", gn=True,
                       sparse=True, seed=37),
    "fat_epilogue": dict(N=2, H=16, W=16, C=128, C2=0, Co=320, k=3, stride=1, pad=1, temb="rows", res=True, gn=True,
                         sparse=True, seed=38),
    "walk": dict(N=17, H=64, W=64, C=64, C2=0, Co=64, k=3, stride=1, pad=1, seed=39),
    "norm_prologue": dict(N=2, H=16, W=16, C=64, C2=64, Co=64, k=3, stride=1, pad=1, norm=True, seed=40),
}
HALO_CASES = {
    "halo_plain": dict(N=2, H=16, W=16, C=64, C2=0, Co=128, k=3, stride=1, pad=1, temb="rows", res=True, gn=True,
                       sparse=True, seed=41),
    "halo_concat": dict(N=1, H=32, W=32, C=64, C2=64, Co=160, k=3, stride=1, pad=1, seed=42),
}


def make_conv(name):
    if name not in _made:
        _made[name] = conv_case(name, **dict(CONV_CASES, **HALO_CASES)[name])
    return _made[name]


def run_conv(c, ops, device="cuda"):
    """The case through ops.conv2d on ``device``: (output, GroupNorm partials or None)."""
    d = c.place(device)
    kw = {}
    if c.kind == "up2":
        assert ops.up2_phases_ok(d["x"], c.k, c.k, c.stride, c.pad, temb=d.get("temb")), f"{c.name}: not phased"
        kw["w_up2"] = ops.pack_up2_phase_weight(d["w"], c.C)
    if c.has("norm"):
        kw["norm"] = (d["norm"][0], d["norm"][1], None)
    y = ops.conv2d(d["x"], d["w"], d.get("bias"), c.k, c.k, c.stride, c.pad, upsample=c.up, x2=d.get("x2"),
                   temb=d.get("temb"), residual=d.get("residual"), stats="gn" if c.gn else None, **kw)
    return y if c.gn else (y, None)


def check_conv(c, y, gp, what=""):
    """Zero tolerance on every output pixel, and on the GroupNorm partials where the case returns them."""
    y64 = conv_y64(c)
    assert_exact(y.cpu(), to_bf16_exact(y64), f"{what} {c.name}")
    if c.gn:
        assert gp is not None, f"{what} {c.name}: no GroupNorm partials returned"
        want = col_partials64(y64.reshape(-1, c.Co))
        assert_exact(gp.double().cpu(), want, f"{what} {c.name} GroupNorm partials")
    TOTALS["poison"] += c.poison_count()
