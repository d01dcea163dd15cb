#!/bin/bash
# Bench line per library variant (tools/bin/ab/libjds_<name>.so; "base" = the
# in-tree build), no parity/CPU legs: kernels_ms and ms_per_step side by side.
# Usage: BENCH_ARGS="..." tools/var_bench.sh name [name ...]
# Output goes to $JDS_OUT (default bench_out/ in the repository root).
cd "$(dirname "$0")/.."; OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"
for v in "$@"; do
  lib=$PWD/tools/bin/ab/libjds_$v.so; [ "$v" = base ] && lib=$PWD/jpeg-dsp-studio_amd/jds/libjds.so
  JDS_LIB_PATH=$lib timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-north-star --no-entropy --no-host-path --no-parity \
    ${BENCH_ARGS:-} > "$OUT/var_$v.json" 2> "$OUT/var_$v.err" || { echo "$v failed"; tail -3 "$OUT/var_$v.err"; exit 1; }
  python3 -c "import json,sys;d=json.load(open('$OUT/var_$v.json'));print('$v', d['ms_per_step'], d['kernels_ms'], d.get('fixups_last_step'))"
done
