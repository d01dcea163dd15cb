#!/bin/bash
# GPU parity tests + a steady-state bench line (each under its own limit).
# Output goes to $JDS_OUT (default bench_out/ in the repository root).
cd "$(dirname "$0")/.."; OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 600 python -m pytest tests -m gpu -x -q -p no:cacheprovider > "$OUT/pytest_gpu.log" 2>&1
rc=$?; tail -3 "$OUT/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-north-star --no-entropy ${BENCH_ARGS:-} > "$OUT/quick.json" 2>"$OUT/quick.err"
rc=$?; [ $rc -eq 0 ] || { tail -5 "$OUT/quick.err"; exit $rc; }
python3 -c "import json;d=json.load(open('$OUT/quick.json'));print(d['value'], d['ms_per_step'], d['kernels_ms'], d.get('parity'))"
