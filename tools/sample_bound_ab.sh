# sampling tests + same-box A/B of the single-product tier's gate (GM2_SINGLE_BOUND) and the tier off
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${GM2_OUT:-bench_out}; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1 TMPDIR=/tmp
timeout -k 10 400 python3 -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 200 --timeout-method thread -rf -k "split or sampl or decode or golden or count" > $OUT/gpu_sel_sb.log 2>&1 || exit $?
: > $OUT/ab_sb.log
for v in "GM2_SINGLE_BOUND=0.25" "GM2_SINGLE_BOUND=0.1" "GM2_SINGLE_BOUND=0.05" "GM2_SINGLE_BOUND=0"; do
  env $v timeout -k 10 400 python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-f32-line --no-c5 > $OUT/bench_sb.log 2>&1 || exit $?
  echo "$v $(grep -h '"sample"' $OUT/bench_sb.log | python3 -c 'import sys,json; d=json.loads(sys.stdin.read())["sample"]; print(d["genomes_per_s"], d["single_tiles"], d["split_tiles"], d["exact_tiles"], d["band_elements"], d["roofline"]["launch_ms"])')" >> $OUT/ab_sb.log
done
