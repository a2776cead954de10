# GPU box: the round's closing runs on the final build (gpurun_out/r04 -> profiles/r04).
cd $GRAFT_REPO_ROOT
O=$GRAFT_REPO_ROOT/gpurun_out/r04
mkdir -p $O
timeout 900 python bench.py --full --steps ${BENCH_STEPS:-3} --warmup 1 > $O/bench_default.json 2> $O/bench_default.err
tail -c 400 $O/bench_default.json
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
python -m pytest tests -m gpu -q --timeout 900 2>&1 | tail -6 > $O/pytest_gpu_final.log; tail -3 $O/pytest_gpu_final.log
