"""v4 implicit-GEMM conv (gemm_8ph.hip): per-segment staging offsets against the fp32 reference conv.

The conv's DMA staging keeps one running source offset per piece and recomputes the im2col address only when the K
position enters a new (filter tap, source tensor) segment.  tools/conv_segment_hashes.py holds the cases, the smallest
shapes at which that state can go wrong (N, H, W, Cin [+ Cin2] -> Cout, NHWC, bf16 randn):

* (5, 8, 8, 64 -> 64) 3x3: the tap changes on every K-tile, four images per 256-row tile, a 64-row M tail;
* (2, 16, 16, 128 -> 320) 3x3: two K-tiles per tap; forced splits 4 start at K-tiles 5 / 10 / 15 (mid-tap, tap boundary);
* (2, 16, 16, 64 + 128 -> 64) 3x3 concat: source and channel stride switch inside every tap;
* (3, 12, 12, 128 -> 96) 3x3 stride 2: M and N tails; (2, 16, 16, 64 + 64 -> 64) 1x1 two-source;
* phase conv (w_up2): (2, 16, 16, 128 -> 64) with per-image bias, SiLU and GroupNorm partials, (4, 8, 8, 64 -> 64) image
  groups, and (1, 16, 16, 320 -> 64), whose forced splits 3 start inside a tap (the host clamps the split count to the
  problem's maximum, 2 for the first and 1 for the second: their splits fall on tap boundaries);
* (2, 8, 8, 128 -> 64) nearest-2x upsample over nine taps; (17, 64, 64, 64 -> 64): 272 tiles, the persistent configs re-seed
  the state per output tile; the second shape again with time embedding + residual + GroupNorm partials.

Every case runs on each v4 config, unsplit and with forced split counts 3 and 4, each (config, splits) pair in its own
process (SHAI_GEMM_FORCE / SHAI_GEMM_FORCE_SPLITS are read once per process).  Tolerances are those of
tests/test_gemm3_gpu.py: relative Frobenius error < 2e-2, < 1e-2 for the phase conv; partials as
test_up2_phase_conv_forced.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "conv_segment_hashes.py")


def _run(cfg, splits):
    env = dict(os.environ, SHAI_GEMM_FORCE=str(cfg), SHAI_GEMM_FORCE_SPLITS=str(splits))
    return subprocess.run([sys.executable, TOOL, "--child", "--check"], env=env, capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("splits", [1, 3, 4])
@pytest.mark.parametrize("cfg", [9, 10, 11, 12])
def test_conv_segments_forced(cuda, cfg, splits):
    from tools.conv_segment_hashes import CASES
    r = _run(cfg, splits)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAIL" not in r.stdout
    # no case dropped: every case printed its output hash and its error figure
    for case in CASES:
        assert f" {case[0]} out " in r.stdout and f"# {case[0]}: rel " in r.stdout, case[0]
