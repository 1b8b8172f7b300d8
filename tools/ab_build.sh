#!/bin/bash
# Builds a variant of libcover_hip.so for same-box A/B runs (COVER_LIB_PATH=tools/ab/libcover_hip_<name>.so):
#   tools/ab_build.sh <name> <file.hip> [extra hipcc flags ...]     e.g.  tools/ab_build.sh pcdbg gemm_tiled.hip -DCOVER_PC_DEBUG
# <file.hip> is the file that holds the switch (gemm_tiled.hip: COVER_PC_*, gemm_stream.hip: COVER_SK_DEBUG, gemm_reduce.hip: COVER_RN_*,
# gemm_v3.hip: COVER_V3_*). Only that file is recompiled with the extra flags; the other objects are those of the default build (run
# `make` first). The object list is the Makefile's SRCS.
set -e
name=$1; src=$2; shift 2
cd "$(dirname "$0")/../cover_vla_amd/csrc"
srcs=$(sed -n 's/^SRCS *= *//p' Makefile)
case " $srcs " in *" $src "*) ;; *) echo "ab_build.sh: $src is not in the Makefile's SRCS" >&2; exit 1;; esac
mkdir -p ../../tools/ab /tmp/ab_$name
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable "$@" -c $src -o /tmp/ab_$name/${src%.hip}.o
objs=""
for s in $srcs; do
  if [ "$s" = "$src" ]; then objs="$objs /tmp/ab_$name/${s%.hip}.o"; else objs="$objs ${s%.hip}.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC $objs -o ../../tools/ab/libcover_hip_$name.so
ls -la ../../tools/ab/libcover_hip_$name.so
