#!/bin/bash
# GEMM microbench + one SQ counter pass over it
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${GM2_OUT:-bench_out}; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1 TMPDIR=/tmp
TAG=${1:-g}
timeout -k 10 300 python3 tools/gemm_bench.py 20 > $OUT/gemm_$TAG.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES --kernel-include-regex "gemm_store" -d $OUT/pmc_gemm_$TAG -o run --output-format csv -- python3 tools/gemm_bench.py 2 > $OUT/pmc_gemm_$TAG.log 2>&1
echo "pmc rc=$?" >> $OUT/gemm_$TAG.log
