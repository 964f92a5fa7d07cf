#!/bin/bash
# Builds tools/materials_prep_check.cpp with the host sanitizers (address, undefined behaviour) and runs it: the host half of
# slrhip_set_materials without a GPU.  ROCM_PATH (default /opt/rocm) is not needed beyond hipcc on the PATH.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$(mktemp -d)"
trap 'rm -rf "$OUT"' EXIT
CSRC="$ROOT/slr_amd/csrc"
# (the shared headers hold device code: the sources are HIP translation units, and the sanitizers go to their host side only)
"${HIPCC:-hipcc}" --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -ffp-contract=off \
    "$ROOT/tools/materials_prep_check.cpp" "$CSRC/materials_prep.cpp" "$CSRC/scene_prep.cpp" "$CSRC/bvh.cpp" "$CSRC/sbvh.cpp" \
    "$CSRC/host_util.cpp" -fsanitize=address,undefined -lpthread -o "$OUT/materials_prep_check"
"$OUT/materials_prep_check"
