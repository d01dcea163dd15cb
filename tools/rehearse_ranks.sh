#!/bin/bash
# Rehearse bench.py's N > 1 path on a one-GPU box: 2 ranks share the GPU over gloo
# (RCCL refuses two ranks on one device).  The driver's 8-GPU runs use nccl.
# The headline leg goes through bench.py's own launcher (--gpus 2 without
# torchrun: it starts the ranks itself; JDS_BENCH_REHEARSE=1 allows sharing the
# one GPU); the sweep leg through torchrun as the driver launches it.  Both with
# --full: the per-rank parity gather is part of the rehearsal.
# Output goes to $JDS_OUT (default bench_out/ in the repository root).
cd "$(dirname "$0")/.."; OUT=$(realpath -m "${JDS_OUT:-bench_out}"); mkdir -p "$OUT"
JDS_BENCH_REHEARSE=1 timeout -k 10 300 python bench.py --gpus 2 --full --steps 5 --warmup 2 --frames 16 --no-cpu-baseline \
  > "$OUT/rehearse_main.json" 2> "$OUT/rehearse_main.err" || { tail -20 "$OUT/rehearse_main.err"; exit 1; }
grep '^{' "$OUT/rehearse_main.json" | cut -c1-400
export JDS_BENCH_BACKEND=gloo JDS_BENCH_SHARE_GPU=1
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29518 bench.py --gpus 2 --sweep --full --steps 2 --warmup 1 --frames 8 \
  > "$OUT/rehearse_sweep.json" 2> "$OUT/rehearse_sweep.err" || { tail -20 "$OUT/rehearse_sweep.err"; exit 1; }
grep '^{' "$OUT/rehearse_sweep.json" | cut -c1-400
