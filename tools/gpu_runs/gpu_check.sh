#!/bin/bash
# Full GPU test suite, then the given bench workloads (default: sd21 + mistral) with --full (the single-request
# p50 latency next to the headline figure).  Each step has its own time limit; the script stops at the first
# failing step.  Logs go to $SHAI_OUT_DIR (default: out/).
#   bash tools/gpu_runs/gpu_check.sh [workload ...]
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
OUT="${SHAI_OUT_DIR:-out}"
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
  > "$OUT/pytest_gpu.log" 2>&1
rc=$?
tail -3 "$OUT/pytest_gpu.log"
[ $rc -eq 0 ] || { grep -E "FAILED|Error" "$OUT/pytest_gpu.log" | head -20; exit $rc; }
[ $# -gt 0 ] || set -- sd21 mistral
for wl in "$@"; do
  timeout -k 10 900 python -u bench.py --full --workload $wl > "$OUT/bench_$wl.log" 2>&1
  rc=$?
  echo "== $wl rc=$rc"; tail -1 "$OUT/bench_$wl.log" | cut -c1-600
  [ $rc -eq 0 ] || exit $rc
done
