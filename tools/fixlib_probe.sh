#!/bin/bash
# k_fix_fwd / forward kernel durations for each library build in tools/bin/ab (rocprofv3 kernel stats),
# with the --full line's parity.  Output goes to $JDS_OUT (default bench_out/ in the repository root).
cd "$(dirname "$0")/.."
ROOT=$(pwd); OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"; export TMPDIR=/tmp; cd /tmp
for L in ${LIBS:-A W5 W6 W7}; do
  JDS_LIB_PATH=$ROOT/tools/bin/ab/libjds_$L.so timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT/fl$L" -o run --output-format csv \
    -- python3 "$ROOT/bench.py" --full --steps 20 --warmup 3 --no-cpu-baseline --no-north-star --no-entropy > "$OUT/fl$L.log" 2>&1 || exit $?
  python3 - "$OUT/fl$L/run_kernel_stats.csv" "$L" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    n = r['Name']
    if 'k_fix_fwd' in n or 'k_fwd32' in n or 'k_inv2' in n:
        print(sys.argv[2], n.split('(')[0][:28], r['Calls'], round(float(r['AverageNs']) / 1e3, 1))
PY
  grep -o '"parity[^}]*}' "$OUT/fl$L.log" || true
done
