#!/bin/bash
# The host twin of point queries (mi_point_query_host) under AddressSanitizer + UndefinedBehaviorSanitizer: the host library's
# sources and tools/sanitize_point_query.c (a stand-alone program with its own main) built with -fsanitize=address,undefined into
# one executable, which is run from the repository root. CPU only; nothing is loaded into python.
#   tools/sanitize_point_query.sh
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build/san
H=$R/ipu_ray_lib_amd/csrc/host
SAN="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
gcc -std=c11 $SAN -Wall -I $R/include -c -o $R/build/san/sanitize_point_query.o $R/tools/sanitize_point_query.c
g++ -std=c++17 $SAN -ffp-contract=off -fno-fast-math -Wall -o $R/build/san/sanitize_point_query $R/build/san/sanitize_point_query.o \
    $H/bvh_sah.cpp $H/lbvh.cpp $H/glb_reader.cpp $H/dae_reader.cpp $H/scene_builtin.cpp $H/scene_api.cpp $H/nif_assets.cpp $H/walk_table.cpp $H/point_query_host.cpp $H/box_query_host.cpp $H/tri_query_host.cpp $H/obox_query_host.cpp $H/capsule_query_host.cpp $H/frustum_query_host.cpp $H/pose_host.cpp -ldl -lm
cd $R
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 $R/build/san/sanitize_point_query $R/assets/monkey_bust.glb
