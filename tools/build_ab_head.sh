#!/bin/bash
# Build tools/variants/a_head.so from git HEAD (a scratch worktree) and
# tools/variants/b_work.so from the working tree, each with its own tree's
# Makefile (so each links its own source list), for RT_HIP_LIB A/B runs.
#   bash tools/build_ab_head.sh [ref]
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
REF=${1:-HEAD}
WT=/tmp/rt_ab_head
rm -rf "$WT"; git -C "$ROOT" worktree prune
git -C "$ROOT" worktree add -f --detach "$WT" "$REF" >/dev/null
mkdir -p "$ROOT/tools/variants"; rm -f "$ROOT"/tools/variants/*.so
build() { make -s -C "$1/tipe-raytracer_amd" librt_hip.so && cp "$1/tipe-raytracer_amd/librt_hip.so" "$ROOT/tools/variants/$2.so"; }
build "$WT" a_head & A=$!
build "$ROOT" b_work & B=$!
wait $A; wait $B
git -C "$ROOT" worktree remove --force "$WT"
ls "$ROOT/tools/variants"
