#!/bin/bash
# Build an experimental variant of the library:  tools/build_variant.sh NAME "-DFM_PF_SUM=3 ..."
# -> build/variants/libfmatch_NAME.so   (run it with: python tools/bench_variant.py build/variants/libfmatch_NAME.so ...)
# The translation units and the flags are the Makefile's own (its OUT, OBJDIR and EXTRA overridden), so a variant has
# every entry point of the library; objects are rebuilt from scratch because EXTRA is no prerequisite of theirs.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
OUT=$ROOT/build/variants
JOBS=$(nproc); [ "$JOBS" -gt 16 ] && JOBS=16
rm -rf "$OUT/obj_$NAME"
make -C "$ROOT/featurematching_amd/csrc" -j"$JOBS" OUT="$OUT/libfmatch_$NAME.so" OBJDIR="$OUT/obj_$NAME" EXTRA="$*" >&2
echo "$OUT/libfmatch_$NAME.so"
