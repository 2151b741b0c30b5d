#!/bin/bash
# A/B builds for timing experiments and mutation checks: tools/build_variant.sh NAME "-DRTX_SC_ABLATE=3 ..."  -> build/NAME.so
# run with RADTXFR_LIB=build/NAME.so (build/ is git-ignored but travels to the GPU box)
# The units are the Makefile's SRCS, so a variant exports every symbol _lib.load() checks.
set -e
NAME=$1; EXTRA=$2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/build/$NAME"
cd "$ROOT/radtxfr_amd/csrc"
SRCS=$(sed -n 's/^SRCS *= *//p' Makefile)
[ -n "$SRCS" ] || { echo "no SRCS line in radtxfr_amd/csrc/Makefile" >&2; exit 1; }
rm -f "$ROOT/build/$NAME.so" "$ROOT"/build/$NAME/*.o
pids=""
for f in $SRCS; do
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off $EXTRA -Wno-unused-function -c $f -o "$ROOT/build/$NAME/${f%.hip}.o" &
  pids="$pids $!"
done
for p in $pids; do wait $p || { echo "compile failed for variant $NAME" >&2; exit 1; }; done
hipcc -shared --offload-arch=gfx950 -o "$ROOT/build/$NAME.so" "$ROOT"/build/$NAME/*.o -ldl
echo "$ROOT/build/$NAME.so"
