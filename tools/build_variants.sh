#!/bin/bash
# Build A/B variants of librt_hip.so into tools/variants/: NAME="-DKNOB=V ..." pairs.
#   bash tools/build_variants.sh a_base "" b_knob "-DRT_QW_MAX=8"
# The sources and flags are the Makefile's (its `variant` target).
cd "$(dirname "$0")/../tipe-raytracer_amd" || exit 1
mkdir -p ../tools/variants
rm -f ../tools/variants/*.so
while [ $# -ge 2 ]; do
  make -s variant OUT="../tools/variants/$1.so" DEFS="$2" &
  shift 2
done
wait
ls ../tools/variants
