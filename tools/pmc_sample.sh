#!/bin/bash
# FETCH_SIZE / WRITE_SIZE passes (each its own --pmc run) over the bench's sample leg decoding from
# the TRAINED v1 checkpoint (10 epochs, as the bench line): per-launch bytes of the sampling kernels
# on the bench's own workload (tools/pmc.py; the v1 training launches of the checkpoint share
# kernel names with the C2 step, so only the sampling kernels' rows of this summary are meaningful)
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${GM2_OUT:-bench_out}; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1 TMPDIR=/tmp
T=${1:-s}
S="bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-f32-line --no-c5 --no-presets --no-c1 --sample-genomes 131072"
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_sfetch_$T -o run --output-format csv -- python3 $S > $OUT/pmc_sfetch_$T.log 2>&1 || exit $?
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pmc_swrite_$T -o run --output-format csv -- python3 $S > $OUT/pmc_swrite_$T.log 2>&1
echo "rc=$?" >> $OUT/pmc_sfetch_$T.log
