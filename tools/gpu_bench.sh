#!/bin/bash
# Full bench.py line (--full) + rocprofv3 kernel stats of the plain run (round profile).
# usage: bash tools/gpu_bench.sh TAG    (writes under $OUT, default bench_out/)
set -o pipefail
TAG=${1:-r2}
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python3 -u bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err" || exit 1
cat "$OUT/bench_$TAG.json"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run --output-format csv -- python3 -u bench.py > "$OUT/bench_prof_$TAG.json" 2> "$OUT/bench_prof_$TAG.err" || exit 1
cat "$OUT/bench_prof_$TAG.json"
