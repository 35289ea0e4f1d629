#!/bin/bash
# Round 6, first GPU pass: the GPU suite after the ADVICE fixes / build-hash guard / asm audit,
# then bench.py --gpus 2 WITHOUT torchrun (the parent spawns both ranks; gloo, one GPU).
set -e
mkdir -p bench_out
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > bench_out/r06a_gpu_tests.log 2>&1
SRNN_DIST_BACKEND=gloo timeout -k 10 500 python3 bench.py --full --gpus 2 --steps 3 --warmup 2 --no-gen --no-cpu \
  > bench_out/r06a_spawn2.json 2> bench_out/r06a_spawn2.err
echo ok
