#!/bin/bash
# Full GPU session: all -m gpu tests, smoke, bench with all legs, sweep bench,
# rocprofv3 kernel stats of the headline bench.  Each step under its own limit;
# a failure stops the script.  Output goes to $JDS_OUT (default bench_out/ in
# the repository root).
cd "$(dirname "$0")/.."; ROOT=$(pwd); OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"; export TMPDIR=/tmp
TAG=${TAG:-rc}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider > "$OUT/pytest_$TAG.log" 2>&1
rc=$?; tail -3 "$OUT/pytest_$TAG.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke_$TAG.log" 2>&1
rc=$?; tail -1 "$OUT/smoke_$TAG.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"
rc=$?; [ $rc -eq 0 ] || { tail -5 "$OUT/bench_$TAG.err"; exit $rc; }
python3 -c "import json;d=json.load(open('$OUT/bench_$TAG.json'));print('bench', d['value'], d['ms_per_step'], d['kernels_ms'], d['roofline']['frac'], d['fixups_last_step'])"
timeout -k 10 300 python bench.py --sweep --full --no-cpu-baseline --no-north-star > "$OUT/sweep_$TAG.json" 2> "$OUT/sweep_$TAG.err"
rc=$?; [ $rc -eq 0 ] || { tail -5 "$OUT/sweep_$TAG.err"; exit $rc; }
python3 -c "import json;d=json.load(open('$OUT/sweep_$TAG.json'));print('sweep', d['value'], d['ms_per_step'], d.get('parity'))"
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run --output-format csv \
  -- python3 "$ROOT/bench.py" > "$OUT/prof_$TAG.log" 2>&1
rc=$?; [ $rc -eq 0 ] || { tail -5 "$OUT/prof_$TAG.log"; exit $rc; }
echo done
