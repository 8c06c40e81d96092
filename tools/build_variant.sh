#!/bin/bash
# build an engine variant next to the shipped library: tools/build_variant.sh NAME -DFLAG=... [-DFLAG=...]
#   -> tools/scratch/libxck_NAME.so   (select it with XCK_LIB=...; tools/variant_bench.sh times every variant found there)
set -e
name=$1; shift
REPO=$(cd "$(dirname "$0")/.." && pwd)
src=$REPO/xcltk_amd/csrc; out=$REPO/tools/scratch; mkdir -p $out/obj_$name
# what the library links and which of it are the engine's units: the Makefile's own lists (OBJS, ENGINE_UNITS)
objs=$(make -s -C $src print-objs); units=$(make -s -C $src print-engine-units)
shared=""; link=""
for o in $objs; do
  case " $units " in *" ${o%.o} "*) link="$link $out/obj_$name/$o";; *) shared="$shared $o"; link="$link $src/$o";; esac
done
make -C $src -j4 $shared > /dev/null
# (every unit of the engine gets the variant's flags: -DXCK_BAF_SPLIT=0 is read by the join, the pipeline's split_mode() and the finish)
for u in $units; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Wno-unused-value -I$REPO/include "$@" -c $src/$u.hip -o $out/obj_$name/$u.o 2>> $out/obj_$name/build.log
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libxck_$name.so $link -lz -lpthread
rm -rf $out/obj_$name
echo "built $out/libxck_$name.so ($*)"
