# rocprofv3 passes of bench.py for tools/summarize_profile.py, written under OUT_DIR (relative to the repository root, or absolute).
# Usage: bash tools/profile_bench.sh OUT_DIR
OUT=${1:?usage: bash tools/profile_bench.sh OUT_DIR}
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- python3 bench.py --legs main --cpu-sample 0 > "$OUT/bench_trace.log" 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/fetch" -- python3 bench.py --legs main --steps 4 --warmup 1 --pre-roll 0 --cpu-sample 0 --min-timed 0 > "$OUT/bench_fetch.log" 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/write" -- python3 bench.py --legs main --steps 4 --warmup 1 --pre-roll 0 --cpu-sample 0 --min-timed 0 > "$OUT/bench_write.log" 2>&1
rocprofv3 --pmc SQ_INSTS_VALU_MFMA_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d "$OUT/mfma" -- python3 bench.py --legs main --steps 4 --warmup 1 --pre-roll 0 --cpu-sample 0 --min-timed 0 > "$OUT/bench_mfma.log" 2>&1
find "$OUT" -name "*.csv" | head -30
du -sh "$OUT"
# BASELINE configs 2-4: one kernel trace per configuration (the kernels of different models share their names)
for c in 2 3 4; do
  rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/cfg$c" -- python3 bench.py --full --legs configs --only-config $c > "$OUT/bench_cfg$c.log" 2>&1
done
