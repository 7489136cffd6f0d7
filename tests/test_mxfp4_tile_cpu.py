"""MXFP4 weights above 64 rows off the GPU: the CPU route is the dequantise route under both values of
``ops.MXFP4_PREFILL``, ``_mxfp4_route`` keeps its argument checks, and the build keeps the fp4 tile GEMM in its
no-scratch check."""
import ast
import os

import pytest
import torch

from shai_amd import ops
from shai_amd.ops import reference as ref
from test_mxfp4_cpu import group_scaled_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("switch", ["fused", "dequant"])
def test_cpu_route_is_unchanged(monkeypatch, switch):
    monkeypatch.setattr(ops, "MXFP4_PREFILL", switch)
    torch.manual_seed(0)
    wq, s = ops.quantize_mxfp4(group_scaled_weights(96, 256, 1))
    wd = ops.dequant_mxfp4(wq, s)
    x = torch.randn(300, 256).bfloat16()
    b = torch.randn(96).bfloat16()
    r = torch.randn(300, 96).bfloat16()
    y = ops.linear(x, wq, b, residual=r, w_scale=s)
    torch.testing.assert_close(y.float(), ref.linear(x, wd, b, None, r).float(), atol=0, rtol=0)
    out = torch.empty(300, 96, dtype=torch.bfloat16)
    ops.gemm_into(x, wq, out, b, residual=r, w_scale=s, force_cfg=1301)
    want = ref.gemm_into(x, wd, torch.empty(300, 96, dtype=torch.bfloat16), b, None, r)
    torch.testing.assert_close(out.float(), want.float(), atol=0, rtol=0)
    fp32 = x.float() @ ops.dequant_mxfp4(wq, s, dtype=torch.float32).t() + b.float() + r.float()
    assert ((y.float() - fp32).norm() / fp32.norm()).item() < 1e-2


def test_switch_and_cap_defaults():
    assert ops.MXFP4_PREFILL in ("fused", "dequant")
    assert os.environ.get("SHAI_MXFP4_PREFILL") is not None or ops.MXFP4_PREFILL == "fused"
    assert isinstance(ops.MXFP4_FUSED_MAX_ROWS, int) and ops.MXFP4_FUSED_MAX_ROWS >= 0


def test_route_keeps_its_argument_checks():
    wq, s = ops.quantize_mxfp4(group_scaled_weights(32, 128, 2))
    x = torch.randn(300, 128).bfloat16()
    with pytest.raises(ValueError, match="w_scale"):
        ops.linear(x, wq)
    with pytest.raises(ValueError, match="K = 128"):
        ops.linear(torch.randn(300, 64).bfloat16(), wq, w_scale=s)
    with pytest.raises(ValueError, match="w_scale"):
        ops.gemm_into(x, wq, torch.empty(300, 32, dtype=torch.bfloat16))


def test_build_checks_the_tile_gemm_for_scratch():
    """Static: csrc/build.py compiles gemm_fp4.hip and names it in NO_SCRATCH (a spilling config fails the build)."""
    src = open(os.path.join(ROOT, "csrc", "build.py")).read()
    consts = {}
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and node.targets[0].id in ("KERNEL_SRCS", "NO_SCRATCH"):
            consts[node.targets[0].id] = ast.literal_eval(node.value)
    assert "kernels/gemm_fp4.hip" in consts["KERNEL_SRCS"]
    assert consts["NO_SCRATCH"].get("kernels/gemm_fp4.hip") == "gemm_fp4_kernel"
    assert os.path.exists(os.path.join(ROOT, "csrc", "kernels", "gemm_fp4.hip"))
