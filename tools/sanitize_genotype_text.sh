#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the HOST side of the genotype text code (bt_genotype_text.hpp, bt_diag_genotype_text, bt_diag_format_g6):
# a stand-alone program (tools/sanitize_genotype_text.cpp), no GPU, nothing loaded into python.  Usage: tools/sanitize_genotype_text.sh [build directory]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-$root/build/sanitize}"
mkdir -p "$out"
(cd "$root" && python3 -c "
import sys
sys.path.insert(0, 'tests')
from _genotype_text import hand_written, make_string
make_string(2, hand_written(2)).tofile('$out/hand_written.words')")
hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wall -Wno-unused-function -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  "$root/bayestyper_amd/csrc/bt_genotype_text.hip" "$root/tools/sanitize_genotype_text.cpp" -fsanitize=address,undefined -o "$out/sanitize_genotype_text"
"$out/sanitize_genotype_text" "$out/hand_written.words"
