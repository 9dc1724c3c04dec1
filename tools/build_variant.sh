#!/bin/bash
# A variant of the library with compile-time knobs, built here (hipcc cross-compiles) so that it travels to the GPU box:
#   tools/build_variant.sh <name> -DRB_FOO=1 ...   ->  renderbaby_amd/variants/lib_<name>.so   (use with RB_LIBRARY_PATH)
# The three device translation units (rb_debug.hip: k_triangle_trip compares the variant's own triangle trip) and the three host files that share their knobs are rebuilt; the rest comes from the last `make`.
#   RB_VARIANT_UNITS="rb_probe_light.hip rb_probe_depth.hip rb_probe_visibility.hip" tools/build_variant.sh <name>
# rebuilds those sources of renderbaby_amd/csrc instead (a hand mutant of the baked-probe kernels, profiles/probe_edges_mutants.txt).
set -e
cd "$(dirname "$0")/.."
name="$1"; shift
mkdir -p renderbaby_amd/variants build/obj
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function"
# rb_build.hip: RB_SPH_LEAF ...; rb_bvh.cpp: host-side knobs, RB_CHUNK_TRIS ...
units=${RB_VARIANT_UNITS:-"rb_kernels.hip rb_debug.hip rb_query.hip rb_build.hip rb_bvh.cpp rb_runtime.cpp rb_accel.cpp"}
objs=""
skip=""
for u in $units; do
    /opt/rocm/bin/hipcc $FLAGS "$@" -c -o build/obj/${u%.*}.$name.o renderbaby_amd/csrc/$u
    objs="$objs build/obj/${u%.*}.$name.o"
    skip="$skip|/$u\\.o\$"
done
# every other object is the last `make`'s
rest=$(ls build/obj/*.hip.o build/obj/*.cpp.o | grep -v -E "${skip#|}")
/opt/rocm/bin/hipcc -fPIC --offload-arch=gfx950 -shared -o renderbaby_amd/variants/lib_$name.so $objs $rest -ldl
echo "renderbaby_amd/variants/lib_$name.so"
