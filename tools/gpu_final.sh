# Round-end check on the GPU box (repo root): the GPU tests, smoke(), the default bench and the
# driver's 20-step bench (both with --full: every line), then a rocprofv3 --stats pass over the
# bench.  Optional tag argument; output files $OUT/final<tag>_* (OUT defaults to bench_out).
set -e
T=${1:-}
OUT=${OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p "$OUT"
timeout -k 10 1000 python -u -m pytest -x -q --timeout 200 --timeout-method thread -m gpu tests > "$OUT/final${T}_gpu_tests.log" 2>&1
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/final${T}_smoke.log" 2>&1
timeout -k 10 600 python -u bench.py --full > "$OUT/final${T}_bench.json" 2> "$OUT/final${T}_bench.err"
timeout -k 10 600 python -u bench.py --full --steps 20 --warmup 5 > "$OUT/final${T}_bench_steps20.json" 2> "$OUT/final${T}_bench_steps20.err"
if [ -n "${ROCPROF:-}" ]; then
  timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/final${T}_prof" -o run -- python3 bench.py --full --steps 200 --warmup 20 --no-cpu > "$OUT/final${T}_bench_rocprof_run.json" 2> "$OUT/final${T}_rocprof.err"
fi
