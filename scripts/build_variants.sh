#!/bin/bash
# Build A/B variants of libsvo_amd.so into octree-raymarcher_amd/build/ (experiments only), through the Makefile's own
# build/libsvo_%.so rule: the same flags and sources as the shipped library, plus the variant's -D switches.
# usage: scripts/build_variants.sh name1:"-DFOO=1 -DBAR=2" name2:"..."
set -e
cd "$(dirname "$0")/.."
pids=()
for spec in "$@"; do
  name="${spec%%:*}"; defs="${spec#*:}"
  make -B -C octree-raymarcher_amd "build/libsvo_$name.so" "DEFS_$name=$defs" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
ls -la octree-raymarcher_amd/build/*.so
