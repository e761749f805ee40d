#!/bin/bash
# Config-4 rehearsal on ONE MI355X (GPU box): `bench.py --gpus 8` self-launches 8 ranks, all on
# device 0 (APE_BENCH_DEVICE=0), each with its contiguous share of the blocks.  Default: the
# configuration's full size, 1,048,576 x 64 KiB blocks = 131,072 per rank, ~24 GiB of device
# memory per rank (192 GiB in all).  It exercises the N > 1 path end to end; the 8-GPU number
# itself stays unmeasured (8 ranks share one GPU here).  --full: every shard verified and the
# CPU baseline timed by rank 0.
#   usage: bash tools/gpu_rehearse8.sh TAG [BLOCKS]    (writes under $OUT, default bench_out/)
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
TAG=${1:-r6}
NB=${2:-1048576}
APE_BENCH_DEVICE=0 timeout -k 10 900 python3 -u bench.py --gpus 8 --blocks $NB --full > "$OUT/rehearse8_$TAG.json" 2> "$OUT/rehearse8_$TAG.err" || { tail -20 "$OUT/rehearse8_$TAG.err"; exit 1; }
cat "$OUT/rehearse8_$TAG.json"
