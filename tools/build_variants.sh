#!/bin/bash
# Build kernel variants of libtray_amd.so for A/B timing (tools/ab_bench.py).
#   tools/build_variants.sh NAME "EXTRA HIPFLAGS" [NAME "FLAGS" ...]
# Each variant is tray_amd/Makefile's library (its translation units, its flags) plus
# the extra flags, built in and written to tray_amd/build/variants/NAME. A variant is
# always compiled afresh (make -B): its flags may differ from the last build of that name.
set -e
cd "$(dirname "$0")/../tray_amd"
while [ $# -ge 2 ]; do
  NAME=$1; FLAGS=$2; shift 2
  OUT=build/variants/$NAME
  make -s -B -j8 BUILD="$OUT" OUT="$OUT" EXTRA="$FLAGS" || { echo "compile failed: $NAME" >&2; exit 1; }
  echo "built $OUT/libtray_amd.so"
done
