"""The host decisions of the MXFP4 / NF4 GEMM paths (support checks, K-group / tile / split heuristics, workspace sizes)
against the recorded table of tests/q4_host_cases.py.  Host arithmetic only: the kernels library loads without a GPU and
nothing is launched."""
import itertools

import pytest
import torch

from q4_host_cases import MS, NKS, Q4_HOST_DECISIONS


@pytest.fixture(scope="module")
def probe():
    from shai_amd import native
    if not native.kernels_available():
        pytest.fail("the kernels library is not built / does not load: run python csrc/build.py")
    return torch.ops.shai.q4_host_decisions


def test_table_is_complete():
    keys = set(itertools.product(("mxfp4", "nf4"), MS, NKS, (0, 1), (0, 1)))
    assert {(f, m, (n, k), g, r) for f, m, n, k, g, r in Q4_HOST_DECISIONS} == keys


def test_host_decisions_match_the_recorded_table(probe):
    bad = {}
    for (fmt, m, n, k, glu, rms), want in Q4_HOST_DECISIONS.items():
        got = tuple(probe(fmt, m, n, k, bool(glu), bool(rms)))
        if got != want:
            bad[(fmt, m, n, k, glu, rms)] = (got, want)
    assert not bad, f"{len(bad)} of {len(Q4_HOST_DECISIONS)} rows differ, first: {next(iter(bad.items()))}"
