#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the HOST side of the BGZF route (bt_bgzf.hpp run by a team of one thread: bt_diag_bgzf, bt_diag_crc32;
# the tabix index builder): a stand-alone program (tools/bgzf_selfcheck.cpp), no GPU, nothing loaded into python.  Usage: tools/bgzf_selfcheck.sh [build directory]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-$root/build/sanitize}"
mkdir -p "$out"
hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wall -Wno-unused-function -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  "$root/bayestyper_amd/csrc/bt_bgzf.hip" "$root/tools/bgzf_selfcheck.cpp" "$root/bayestyper_amd/host/TabixIndex.cpp" -fsanitize=address,undefined -lz -o "$out/bgzf_selfcheck"
"$out/bgzf_selfcheck"
