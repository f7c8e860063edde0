#!/usr/bin/env bash
# Round-2 closing GPU pass: full GPU suite, smoke, the default bench, a
# kernel-trace of the bench, and per-workload kernel profiles (trace + PMC
# passes, tools/profile.sh) for the traffic summaries.
#   tools/gpu_r2final.sh <tag>
set -uo pipefail
root=${GRAFT_REPO_ROOT:-$(pwd)}
tag=${1:-r2f}
out=$root/gpurun_out/$tag; mkdir -p $out
cd $root
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > $out/gpu_tests.log 2>&1 || { tail -30 $out/gpu_tests.log; exit 1; }
tail -2 $out/gpu_tests.log
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $out/smoke.log 2>&1 || { tail -20 $out/smoke.log; exit 1; }
tail -1 $out/smoke.log
timeout -k 10 300 python -u bench.py --full > $out/bench.json 2> $out/bench.err || { tail -20 $out/bench.err; exit 1; }
echo "bench done"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/bench_trace -o run --output-format csv -- python3 $root/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --file-path none > $out/bench_trace.log 2>&1 || { tail -20 $out/bench_trace.log; exit 1; }
echo "bench trace done"
cd $root
for wl in uniform zipf text; do
  bash tools/profile.sh all $wl ${tag}_all_$wl > /dev/null 2>&1 || { echo "profile $wl failed"; exit 1; }
  echo "profile $wl done"
done
bash tools/profile.sh indexless zipf ${tag}_idx_zipf > /dev/null 2>&1 || { echo "profile idx failed"; exit 1; }
echo "r2final done"
