"""Child process of tests/test_gemm_exact_gpu.py::test_conv_forced: every conv case of tests/gemm_exact.py, and the
weight-slice GEMM, under the tile config and split-K count the parent forced through SHAI_GEMM_FORCE /
SHAI_GEMM_FORCE_SPLITS (read once per process).  A case the forced config does not support takes the library's own
choice and is checked all the same.  Exit status 0 = every output element and every GroupNorm partial equals the fp64
oracle; the last line reports what was compared."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import gemm_exact as ge  # noqa: E402
import shai_amd.ops as ops  # noqa: E402


def main():
    what = f"cfg {os.environ.get('SHAI_GEMM_FORCE', '-')} splits {os.environ.get('SHAI_GEMM_FORCE_SPLITS', '1')}"
    for name in ge.CONV_CASES:
        c = ge.make_conv(name)
        y, gp = ge.run_conv(c, ops)
        torch.cuda.synchronize()
        ge.check_conv(c, y, gp, what)
        print(f"{what} {name}: {y.numel()} elements exact", flush=True)
    c = ge.make_gemm("bias2d_slices")
    d = c.place("cuda")
    y = ops.linear_wslices(d["x"], d["w"], d["bias2d"], c.M // c.slices)
    ge.assert_exact(y, ge.gemm_want(c)[0], f"{what} bias2d_slices")
    ge.TOTALS["poison"] += c.poison_count()
    print(f"{what} bias2d_slices: {y.numel()} elements exact", flush=True)
    print("TOTALS compared {compared} canaries {canaries} poison {poison}".format(**ge.TOTALS), flush=True)


if __name__ == "__main__":
    main()
