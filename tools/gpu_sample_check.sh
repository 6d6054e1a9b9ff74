# sampling-path GPU check: the sampling / decode / golden tests, the bench's sample leg, and a kernel
# trace of a 262,144-genome sample leg
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${GM2_OUT:-bench_out}; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1 TMPDIR=/tmp
timeout -k 10 400 python3 -u -m pytest tests -m gpu -x -v -p no:cacheprovider --timeout 200 --timeout-method thread -rf -s -k "split or sampl or decode or golden or count" > $OUT/gpu_sel_c.log 2>&1 || exit $?
timeout -k 10 400 python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-f32-line --no-c5 > $OUT/bench_c.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_c -o run --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-f32-line --no-c5 --sample-genomes 262144 > $OUT/prof_c.log 2>&1
