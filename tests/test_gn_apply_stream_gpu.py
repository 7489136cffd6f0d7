"""The streaming GroupNorm(+SiLU) apply pass (csrc/kernels/norm.hip gn_apply_kernel): one run of pixels of one image
per workgroup, several loads in flight per thread.

Shapes sit where the run / slab indexing can go wrong: one vector, images far smaller than a run, prime HW, a tail
past the unroll, the 8 x 8 level (C / 8 = 160 and 240 vectors per pixel), two sources, C / 8 above 256 (two slabs).
The kernel writes into a view of a larger buffer pre-filled with a sentinel, which must be intact on both sides.

silu off is checked EXACTLY: for bf16 x and bf16-representable scale / shift the fp64 expression x * scale + shift is
exact (8 x 8-bit significands, exponents far inside fp64's range), so its rounding to fp32 is the fused
multiply-add's rounding, and the bf16 rounding after it is the kernel's.  silu on uses the project's bound for this op.
"""
import pytest
import torch

import shai_amd.ops as ops
from shai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 0), (3, 5, 8, 8), (7, 3, 24, 16), (2, 37, 40, 0), (1, 4099, 320, 0), (5, 64, 1280, 0),
          (3, 64, 1280, 640), (2, 1000, 640, 320), (2, 4096, 320, 320),
          (2, 9, 2056, 2064)]  # beyond the issue's list: C / 8 = 515, three slabs of unequal width
GUARD = 4096        # bf16 elements on each side of the output view
SENTINEL = 0x5A5A   # bf16 bit pattern of the guards


def close(a, b, atol, rtol=2e-2):
    """tests/test_kernels_gpu.py's bound: fewer than 0.1 % of the elements outside atol + rtol |b|."""
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    assert torch.isfinite(a).all(), "non-finite output"
    assert bad < 1e-3, f"{bad*100:.3f}% elements out of tolerance; max err {err.max().item():.4g}"


_cases = {}


def case(shape):
    """Inputs and both references of a shape, made once and shared by the tests (never written to)."""
    if shape not in _cases:
        N, HW, C1, C2 = shape
        g = torch.Generator(device="cuda").manual_seed(N * 7919 + HW * 31 + C1 + 3 * C2)
        C = C1 + C2
        x = torch.randn(N, HW, C1, device="cuda", generator=g).bfloat16()
        x2 = torch.randn(N, HW, C2, device="cuda", generator=g).bfloat16() if C2 else None
        sc = (torch.randn(N, C, device="cuda", generator=g) * 1.5).bfloat16().float()
        sh = (torch.randn(N, C, device="cuda", generator=g) * 1.5).bfloat16().float()
        xc = torch.cat([x, x2], -1) if C2 else x
        exact = (xc.double() * sc.double()[:, None, :] + sh.double()[:, None, :]).float().to(torch.bfloat16)
        silu = ref.groupnorm_apply(xc, sc, sh, True)
        _cases[shape] = (x, x2, sc, sh, exact, silu)
    return _cases[shape]


def run_guarded(x, x2, sc, sh, silu):
    """The binding writing into the middle of a sentinel-filled buffer; returns the output after checking the guards."""
    N, HW = x.shape[0], x.shape[1]
    C = x.shape[2] + (x2.shape[2] if x2 is not None else 0)
    n = N * HW * C
    buf = torch.empty(n + 2 * GUARD, dtype=torch.bfloat16, device=x.device)
    raw = buf.view(torch.int16)
    raw.fill_(SENTINEL)
    out = buf[GUARD:GUARD + n].view(N, HW, C)
    ops._K().groupnorm_apply(x, x2, sc, sh, out, silu)
    torch.cuda.synchronize()
    assert bool((raw[:GUARD] == SENTINEL).all()), "wrote before the output"
    assert bool((raw[GUARD + n:] == SENTINEL).all()), "wrote past the output"
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply_exact_without_silu(cuda, shape):
    x, x2, sc, sh, exact, _ = case(shape)
    y = run_guarded(x, x2, sc, sh, False)
    diff = (y.view(torch.int16) != exact.view(torch.int16))
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} elements differ from the fused multiply-add"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply_silu_matches_reference(cuda, shape):
    x, x2, sc, sh, _, silu = case(shape)
    close(run_guarded(x, x2, sc, sh, True), silu, 2e-2)


@pytest.mark.parametrize("C1,C2", [(64, 0), (64, 64)], ids=["one-source", "two-source"])
def test_conv_norm_path_equals_apply_then_conv(cuda, C1, C2):
    """conv2d(norm=...) runs the same apply pass inside the operator: bit-equal to the pass followed by the conv."""
    g = torch.Generator(device="cuda").manual_seed(11 + C2)
    N, H, Cin, Cout = 2, 16, C1 + C2, 64
    x = torch.randn(N, H, H, C1, device="cuda", generator=g).bfloat16()
    x2 = torch.randn(N, H, H, C2, device="cuda", generator=g).bfloat16() if C2 else None
    w = ops.pack_conv_weight((torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / (9 * Cin) ** 0.5).bfloat16())
    b = torch.randn(Cout, device="cuda", generator=g).bfloat16()
    sc = torch.randn(N, Cin, device="cuda", generator=g) * 0.5 + 1.0
    sh = torch.randn(N, Cin, device="cuda", generator=g) * 0.5
    prev = ops.set_halo_conv(0, -1)  # the default routing: apply pass + tuned conv
    try:
        fused = ops.conv2d(x, w, b, 3, 3, 1, 1, x2=x2, norm=(sc, sh, "silu"))
        xn = ops.groupnorm_apply(x, sc, sh, True, x2=x2)
        two = ops.conv2d(xn, w, b, 3, 3, 1, 1)
    finally:
        ops.set_halo_conv(prev, -1)
    assert torch.equal(fused.view(torch.int16), two.view(torch.int16))
