set -x
REPO=$(cd "$(dirname "$0")/.." && pwd)
: "${OUT:?set OUT to the directory the outputs go to}"
cd "$REPO"
timeout 300 python bench.py --full --steps 2 --warmup 1 > "$OUT"/g_bench.json 2> "$OUT"/g_bench.err
tail -c 300 "$OUT"/g_bench.json
timeout 200 python bench.py --full --algo cpo --no-cpu-baseline --steps 3 --warmup 1 > "$OUT"/g_bench_cpo.json 2>/dev/null
tail -c 400 "$OUT"/g_bench_cpo.json
timeout 150 python tools/ma_bench.py --episodes 3 2>/dev/null | tail -1 > "$OUT"/g_ma_bench.json
cat "$OUT"/g_ma_bench.json
export TMPDIR=/tmp
cd /tmp && rm -rf /tmp/prof /tmp/pmcf /tmp/pmcw
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -- python "$REPO"/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > /tmp/prof.log 2>&1
timeout 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d /tmp/pmcf -- python "$REPO"/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --learning-iters 1 > /tmp/pmcf.log 2>&1
timeout 200 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d /tmp/pmcw -- python "$REPO"/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --learning-iters 1 > /tmp/pmcw.log 2>&1
cd "$REPO"
python tools/kernel_trace_summary.py /tmp/prof "$OUT"/g_kernel_stats.csv "$OUT"/g_gae.json "rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline" | tail -25
F=$(find /tmp/pmcf -name "*counter_collection.csv" | head -1); W=$(find /tmp/pmcw -name "*counter_collection.csv" | head -1)
echo "F=$F W=$W"
if [ -n "$F" ] && [ -n "$W" ]; then python tools/pmc_summary.py "$F" "$W" "$OUT"/g_gae_pmc.json | tail -30; else tail -5 /tmp/pmcf.log /tmp/pmcw.log; fi
