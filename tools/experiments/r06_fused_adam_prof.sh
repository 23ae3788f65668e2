#!/bin/bash
# r06: per-kernel times of the training iteration, optimizer step inside the backward against behind it
# usage: OUT=<output directory> bash tools/experiments/r06_fused_adam_prof.sh
cd "$(dirname "$0")/../.."
R=$(pwd); mkdir -p "${OUT:?set OUT to the directory the profile goes to}"; OUT=$(cd "$OUT" && pwd)
export GSPLAT_NO_BUILD=1 GSPLAT_BENCH_REFERENCE_HOST=0 GSPLAT_BENCH_EXCHANGE_HOST_COST=0 GSPLAT_BENCH_ALTERNATING=0
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r06_adam_prof -- python3 $R/bench.py --full --steps 40 --warmup 5 --no-cpu-baseline --no-extra-workloads > $OUT/r06_adam_prof.log 2>&1)
f=$(ls -t $OUT/r06_adam_prof/*/*kernel_stats.csv | head -1)
python3 - "$f" <<'PY'
import csv,sys
for r in csv.DictReader(open(sys.argv[1])):
    n=r['Name']
    if any(k in n for k in ('preprocess_bwd','optimizer_','loss_','render_bwd','sh_adam_dir')):
        print(f"{n[:110]:110s} calls {r['Calls']:>4s} avg_us {float(r['AverageNs'])/1e3:8.1f}")
PY
