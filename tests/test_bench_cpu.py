"""bench.py driver contract on the CPU: ``--gpus N`` outside a launcher re-runs itself as N ranks under
torch.distributed.run and rank 0 prints ONE JSON line whose n_gpus is N (dry-run mode: tiny SD2.1 config
over gloo -- the launcher / rendezvous / barrier / max-over-ranks plumbing, not a measurement)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 2])
def test_bench_self_launch_reports_n_gpus(n):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1",
                        "--warmup", "0", "--batch", "1", "--inference-steps", "2", "--latency-runs", "1",
                        "--cpu-dry-run", "--full"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["steps"] == 1 and d["warmup"] == 0
    assert d["config"]["parallelism"] == f"dp{n}" and d["config"]["global_batch"] == n
    assert d["value"] > 0 and "DRY RUN" in d["data"]
    assert d["p50_latency_ms_bs1"] > 0  # --full: the single-request latency runs happened


def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain run skips the --full extras (p50_latency_ms_bs1 is null), --steps sets the number of timed steps,
    and --dump-outputs writes the last timed step's images, identical from run to run with the same arguments."""
    import numpy as np
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    got = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                            "--warmup", "0", "--batch", "1", "--inference-steps", "2", "--cpu-dry-run",
                            "--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, timeout=600,
                           env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["p50_latency_ms_bs1"] is None
        assert d["value"] == pytest.approx(1 * 2 / (2 * d["ms_per_step"] / 1000), rel=1e-2)
        assert os.listdir(tmp_path / name) == ["images.npy"]
        got.append(np.load(tmp_path / name / "images.npy"))
    assert got[0].dtype == np.float32 and got[0].shape == (1, 64, 64, 3) and np.isfinite(got[0]).all()
    assert np.array_equal(got[0], got[1])


def test_dump_outputs_samples_large_arrays_within_budget(tmp_path, monkeypatch):
    """An output over the size budget is written as a fixed sample: same indices on every call, float32,
    inside the budget; a small one is written whole."""
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("shai_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10 ** 6
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1000)
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100).to(torch.bfloat16)
    small = np.arange(12, dtype=np.float64).reshape(3, 4)
    for d in ("a", "b"):
        bench._dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (500,) and np.array_equal(a, b)
    assert np.isin(a, big.float().numpy()).all() and (np.diff(a) >= 0).all() and len(np.unique(a)) > 100
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small)
    assert a.nbytes + s.nbytes <= 4 * 1000


def test_bench_rejects_world_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu-dry-run"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)
