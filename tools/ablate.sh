#!/bin/bash
# usage: tools/ablate.sh <tag> <EXTRA flags...>: rebuilds, with the flags on the GPU box, the objects whose sources read
# gs_render.h's build switches (of the Makefile's SRCS: those that include gs_render.h or gs_context.h) and runs the bench
tag=$1; shift
(cd 3dgs_amd/csrc && touch $(grep -lE '#include "gs_(render|context)\.h"' $(make -s print-srcs))) || exit 1
make -C 3dgs_amd/csrc -s EXTRA="$*" > gpurun_out/ablate_build_$tag.log 2>&1 || exit 1
timeout -k 10 200 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$tag', round(d['value'],1), d['stage_ms'])"
