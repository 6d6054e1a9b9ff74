#!/bin/bash
# kernel trace + stats of the sampling leg alone (bench.py with one training step)
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${GM2_OUT:-bench_out}; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1 TMPDIR=/tmp
T=${1:-s}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$T -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-f32-line --no-c5 > $OUT/prof_$T.log 2>&1
echo "rc=$?" >> $OUT/prof_$T.log
