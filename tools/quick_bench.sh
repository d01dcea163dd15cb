#!/bin/bash
# Bench line (no CPU legs) + rocprofv3 kernel stats of the same command.
# Output goes to $JDS_OUT (default bench_out/ in the repository root).
cd "$(dirname "$0")/.."; ROOT=$(pwd); OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"; export TMPDIR=/tmp
TAG=${TAG:-quick}
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-north-star --no-entropy --no-host-path ${BENCH_ARGS:-} > "$OUT/$TAG.json" 2>"$OUT/$TAG.err"
rc=$?; [ $rc -eq 0 ] || { tail -5 "$OUT/$TAG.err"; exit $rc; }
python3 -c "import json;d=json.load(open('$OUT/$TAG.json'));print(d['value'], d['ms_per_step'], d['kernels_ms'], d.get('fixups_last_step'), d.get('parity'))"
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run --output-format csv \
  -- python3 "$ROOT/bench.py" --full --no-cpu-baseline --no-north-star --no-entropy --no-host-path --no-parity ${BENCH_ARGS:-} > "$OUT/prof_$TAG.log" 2>&1
rc=$?; [ $rc -eq 0 ] || { tail -5 "$OUT/prof_$TAG.log"; exit $rc; }
f=$(find "$OUT/prof_$TAG" -name '*kernel_stats.csv' | head -1)
python3 - "$f" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
for r in rows[:8]:
    print(f"{r['Name'][:70]:70s} calls={r['Calls']:>5} avg_us={float(r['AverageNs'])/1e3:9.1f} pct={r['Percentage']}")
PY
