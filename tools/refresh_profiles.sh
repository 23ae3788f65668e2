#!/bin/bash
# usage (on the GPU box): OUT=<output directory> bash tools/refresh_profiles.sh <tag>   e.g. r04
# rocprofv3 kernel-trace summary of the bench command, the PMC passes (counters in their own runs, never combined with
# tracing), traffic.json from them -- and THEN the bench line, so that it carries the counters of this very build;
# everything lands under $OUT/<tag>_*, from where the summaries are copied to profiles/.
set -e
TAG=${1:-r05}
cd "$(dirname "$0")/.."
R=$(pwd); mkdir -p "${OUT:?set OUT to the directory the profiles go to}"; OUT=$(cd "$OUT" && pwd)
python -c "import importlib; importlib.import_module('3dgs_amd._lib').build()"   # once, before anything touches the GPU
export GSPLAT_NO_BUILD=1
(
  export GSPLAT_BENCH_TRAIN_STEP=0   # the profiled runs: the headline workload's kernels only,
  # no child processes under the profiler (the C++ reference host, the one-rank RCCL rehearsal), and only the headline
  # view's launches in the per-kernel averages (no alternating views)
  export GSPLAT_BENCH_REFERENCE_HOST=0 GSPLAT_BENCH_EXCHANGE_HOST_COST=0 GSPLAT_BENCH_ALTERNATING=0
  cd /tmp && export TMPDIR=/tmp
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats -- python3 $R/bench.py --full --no-cpu-baseline --no-extra-workloads > $OUT/${TAG}_stats.log 2>&1
  cd $R
  cp "$(ls -t $OUT/${TAG}_stats/*/*kernel_stats.csv | head -1)" $OUT/${TAG}_kernel_stats.csv
  bash profiles/run_pmc.sh $OUT/${TAG}_pmc > $OUT/${TAG}_pmc.log 2>&1
  python3 profiles/summarize_pmc.py $OUT/${TAG}_pmc > $OUT/${TAG}_pmc_summary.json
  # r05: the same counters and kernel summary on the garden-shaped workload (a trained capture's density: large splats,
  # lists of ~1150 entries, 40 % culled), whose roofline entries the bench line carries next to the uniform scene's
  bash profiles/run_pmc.sh $OUT/${TAG}_pmc_garden1200k garden1200k > $OUT/${TAG}_pmc_garden1200k.log 2>&1
  python3 profiles/summarize_pmc.py $OUT/${TAG}_pmc_garden1200k > $OUT/${TAG}_pmc_summary_garden1200k.json
  (cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats_garden1200k -- python3 $R/tools/workload_stats.py garden1200k 30 > $OUT/${TAG}_stats_garden1200k.log 2>&1)
  cp "$(ls -t $OUT/${TAG}_stats_garden1200k/*/*kernel_stats.csv | head -1)" $OUT/${TAG}_garden1200k_kernel_stats.csv
  python3 profiles/make_traffic.py $OUT/${TAG}_pmc_summary.json garden1200k=$OUT/${TAG}_pmc_summary_garden1200k.json > $OUT/${TAG}_traffic.json
)
cp $OUT/${TAG}_traffic.json profiles/traffic.json   # (on the box's copy of the tree: bench.py reads it from there)
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
head -12 $OUT/${TAG}_kernel_stats.csv
