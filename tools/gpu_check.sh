#!/bin/bash
# One GPU session: parity tests, then (only if no fault/timeout) bench + rocprof.
# Each GPU step has its own time limit; a fault, abort, segfault or timeout ends the script.
# Output goes to $JDS_OUT (default bench_out/ in the repository root).
set -u
cd "$(dirname "$0")/.."
ROOT=$(pwd); OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"
export TMPDIR=/tmp
ok() { case "$1" in 0|1) return 0;; *) echo "stopping: rc=$1"; exit "$1";; esac; }
STAGE="${1:-all}"

if [ "$STAGE" = all ] || [ "$STAGE" = tests ]; then
  timeout -k 10 900 python -m pytest tests -m gpu -q -p no:cacheprovider > "$OUT/pytest_gpu.log" 2>&1
  rc=$?; echo "pytest-gpu rc=$rc"; tail -5 "$OUT/pytest_gpu.log"; ok $rc
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
  rc=$?; echo "smoke rc=$rc"; tail -3 "$OUT/smoke.log"; ok $rc
fi
if [ "$STAGE" = all ] || [ "$STAGE" = bench ]; then
  timeout -k 10 600 python bench.py --full --steps 20 --warmup 3 > "$OUT/bench.json" 2> "$OUT/bench.err"
  rc=$?; echo "bench rc=$rc"; cat "$OUT/bench.json"; tail -3 "$OUT/bench.err"; [ $rc -eq 0 ] || exit $rc
fi
if [ "$STAGE" = all ] || [ "$STAGE" = prof ]; then
  cd /tmp
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv \
    -- python3 "$ROOT/bench.py" --full --steps 20 --warmup 3 --no-cpu-baseline --no-north-star --no-parity \
    > "$OUT/prof.log" 2>&1
  rc=$?; echo "rocprof rc=$rc"; tail -3 "$OUT/prof.log"; [ $rc -eq 0 ] || exit $rc
fi
echo done
