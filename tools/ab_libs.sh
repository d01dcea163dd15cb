#!/bin/bash
# Same-box A/B of library variants on the headline bench line (kernel legs only).
# usage: tools/ab_libs.sh TAG "lib1 lib2 ..." [bench args...]   (lib "default" = jds/libjds.so;
# others are paths under tools/bin/ab/).  Two interleaved passes; prints value and per-kernel ms.
# Output goes to $JDS_OUT (default bench_out/ in the repository root).
cd "$(dirname "$0")/.."; OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"
TAG=$1; LIBS=$2; shift 2
for pass in 1 2; do
  for lib in $LIBS; do
    if [ "$lib" = default ]; then unset JDS_LIB_PATH; else export JDS_LIB_PATH=$PWD/$lib; fi
    timeout -k 10 300 python -u bench.py --full --steps 30 --warmup 5 --no-north-star --no-host-path --no-entropy \
      --no-cpu-baseline --no-parity "$@" > "$OUT/${TAG}_one.json" 2>> "$OUT/${TAG}.err" \
      || { echo "rc=$? $lib"; tail -5 "$OUT/${TAG}.err"; exit 1; }
    python3 -c "
import json; d=json.load(open('$OUT/${TAG}_one.json'))
print('$pass', '$lib'.split('/')[-1], d['value'], d['ms_per_step'], d['kernels_ms'], d.get('fixups_last_step'))" | tee -a "$OUT/${TAG}.txt"
  done
done
