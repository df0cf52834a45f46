# rocprofv3 kernel-trace summary of a short full bench run (round-1 profile).
# Run from the repository root on the GPU box; results go under $OUT (default prof_out/).
set -u
OUT=${OUT:-prof_out}; mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
TAG=${TAG:-prof}
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$PWD/$OUT/$TAG" -o run -- python bench.py --full --steps 10 --warmup 2 --no-cpu ${BENCH_ARGS:-} > "$OUT/$TAG.log" 2>&1
rc=$?; echo rc=$rc; grep '^{' "$OUT/$TAG.log" | cut -c1-400
cut -d, -f1-5 "$OUT/$TAG/run_kernel_stats.csv" | head -12
