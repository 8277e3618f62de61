#!/bin/bash
# oracle/build_ref.sh -- compile the reference's own benchmark drivers, UNCHANGED and
# straight from the reference checkout (LABSORT_REFERENCE), against this repo's drop-in
# headers (include/lab.h, include/utils.h) and liblabsort.so.  This is the
# "main.cpp/performanceTest.cpp link unchanged" check of the north_star.
#
# main.cpp / performanceTest.cpp include "include/lab.h" relative to their own
# directory, so each is compiled through a symlink placed next to a symlink of
# our include/ in a scratch directory; nothing from the reference is copied.
# Outputs: oracle/_ref/sort, oracle/_ref/performaceTest (git-ignored: binaries compiled
# from the reference stay out of history).  They find liblabsort.so through an $ORIGIN
# rpath, so a tree built where the reference is present can be moved as a whole to a
# machine without it: build() there rebuilds the library and keeps these two binaries.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REPO="$(cd "$HERE/.." && pwd)"
REF="${LABSORT_REFERENCE:-/root/reference/Sord Radix y Merge}"
PKG="radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd"
if [ ! -f "$REF/main.cpp" ]; then
    echo "build_ref: reference sources not present ($REF); keeping prebuilt binaries" >&2
    exit 0
fi
SCRATCH="$(mktemp -d /tmp/labsort_harness.XXXXXX)"
trap 'rm -rf "$SCRATCH"' EXIT
ln -s "$REPO/include" "$SCRATCH/include"
ln -s "$REF/main.cpp" "$SCRATCH/main.cpp"
ln -s "$REF/performanceTest.cpp" "$SCRATCH/performanceTest.cpp"
OUT="$HERE/_ref"
mkdir -p "$OUT"
# same flags as the reference Makefile:1-3 minus the nvcc-only ones
CXXFLAGS="-O3 -std=c++11"
LDFLAGS="-L$REPO/$PKG -llabsort -Wl,-rpath,\$ORIGIN/../../$PKG -lm -lpthread"
g++ $CXXFLAGS "$SCRATCH/main.cpp" -o "$OUT/sort" $LDFLAGS
g++ $CXXFLAGS "$SCRATCH/performanceTest.cpp" -o "$OUT/performaceTest" $LDFLAGS
echo "build_ref: built $OUT/sort $OUT/performaceTest"
