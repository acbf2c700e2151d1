# long-block timing probe: the full bench with and without the CPU baseline legs
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${LP_OUT:-bench_out/lp2}; mkdir -p "$OUT"
timeout -k 10 600 python -u bench.py --full --skip-cpu --steps 20 --warmup 5 > "$OUT/full_skipcpu.json" 2> "$OUT/full_skipcpu.err" || exit $?
timeout -k 10 600 python -u bench.py --full --steps 20 --warmup 5 > "$OUT/full.json" 2> "$OUT/full.err" || exit $?
