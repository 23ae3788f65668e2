#!/bin/bash
# usage: tools/ab/build_seg_variants.sh "<entries> <split_min>" ...: tools/ab/libseg<entries>m<split_min>.so, the library with
# every object whose source includes gs_render.h (where GS_SEG_ENTRIES / GS_SEG_SPLIT_MIN are read; gs_render.h: TileSegments)
# built for that segment length / split threshold.  The library's objects are the Makefile's SRCS (make print-srcs).
cd "$(dirname "$0")/../../3dgs_amd/csrc" || exit 1
make -s || exit 1
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -munsafe-fp-atomics -mllvm -amdgpu-atomic-optimizer-strategy=None -Wno-unused-function"
srcs=$(make -s print-srcs) || exit 1
# (gs_context.h includes gs_render.h: sources that include either)
seg_srcs=$(grep -lE '#include "gs_(render|context)\.h"' $srcs)
for v in "$@"; do
  set -- $v; tag=seg$1m$2
  objs=""
  for s in $srcs; do
    n=${s%.hip}
    case " $(echo $seg_srcs) " in
      *" $s "*) hipcc $FLAGS -DGS_SEG_ENTRIES=$1 -DGS_SEG_SPLIT_MIN=$2 -c -o /tmp/seg_${n}_$tag.o $s & objs="$objs /tmp/seg_${n}_$tag.o" ;;
      *) objs="$objs $n.o" ;;
    esac
  done
  wait
  g++ -O2 -std=c++17 -fPIC -DGS_BUILD_FLAGS="\"variant:$tag\"" -c -o /tmp/seg_version_$tag.o gs_version.cpp &&
  hipcc --offload-arch=gfx950 -shared -o ../../tools/ab/lib$tag.so /tmp/seg_version_$tag.o $objs || { echo "FAILED: $tag"; exit 1; }
done
