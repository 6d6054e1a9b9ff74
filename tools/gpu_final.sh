#!/bin/bash
# round-end check of HEAD: every -m gpu test, smoke(), the default bench line, a kernel-trace summary,
# then the 2-rank bench rehearsal through bench.py's own launcher (gloo, both ranks on the one GPU)
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${GM2_OUT:-bench_out}; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1 TMPDIR=/tmp
T=${1:-z}
timeout -k 10 700 python3 -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 240 --timeout-method thread -rf > $OUT/gpu_tests_$T.log 2>&1
rc=$?; echo "pytest rc=$rc" >> $OUT/gpu_tests_$T.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$T.log 2>&1 || exit $?
timeout -k 10 400 python3 bench.py --full > $OUT/bench_$T.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$T -o run --output-format csv -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-f32-line --sample-genomes 262144 > $OUT/prof_$T.log 2>&1
rc=$?; echo "prof rc=$rc" >> $OUT/prof_$T.log
[ $rc -ne 0 ] && exit $rc
GM2_DIST_BACKEND=gloo timeout -k 10 400 python3 bench.py --full --gpus 2 --steps 5 --warmup 2 --no-sample --no-c5 > $OUT/bench2_$T.log 2>&1
rc=$?; echo "bench2 rc=$rc" >> $OUT/bench2_$T.log
exit $rc
