#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the HOST side of the deflate code (bt_deflate.hpp run by a team of one thread, bt_diag_deflate): a
# stand-alone program (tools/deflate_selfcheck.cpp), no GPU, nothing loaded into python.  Usage: tools/deflate_selfcheck.sh [build directory]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-$root/build/sanitize}"
mkdir -p "$out"
hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wall -Wno-unused-function -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  "$root/bayestyper_amd/csrc/bt_deflate.hip" "$root/tools/deflate_selfcheck.cpp" -fsanitize=address,undefined -lz -o "$out/deflate_selfcheck"
"$out/deflate_selfcheck"
