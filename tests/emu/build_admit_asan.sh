#!/bin/bash
# TEST INFRASTRUCTURE: build admit_block_asan — the device layer (kernels +
# tas_device) and tests/emu/admit_block_asan.cpp in one executable against the
# CPU SIMT emulator, with AddressSanitizer and UBSan.  The sources are the
# patched copies build_emu.sh makes (its sed block, into a directory of their
# own); the host layer is not linked.  The device layer's object takes minutes
# to compile and is kept until a source is newer.
# Output: tests/emu/_build/admit_block_asan.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="$HERE/_build"
A="$OUT/asan"
CXX="g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -pthread"
newest="$(ls -t "$ROOT"/kueue_oss_amd/csrc/*.h "$ROOT"/kueue_oss_amd/csrc/*.hip "$ROOT"/include/*.h \
  "$HERE/hip/hip_runtime.h" "$HERE/hip_emu.cpp" "$HERE/build_emu.sh" "$HERE/build_admit_asan.sh" | head -1)"
if [ ! -f "$A/device.o" ] || [ "$A/device.o" -ot "$newest" ]; then
  EMU_OUT="$A" EMU_SOURCES_ONLY=1 bash "$HERE/build_emu.sh"
  $CXX -I"$HERE" -I"$A/src" -c "$HERE/hip_emu.cpp" -o "$A/hip_emu.o" &
  $CXX -I"$HERE" -I"$A/src" -c "$A/src/tas_device.cpp" -o "$A/device.o"
  wait
fi
$CXX -I"$HERE" -I"$A/src" "$A/device.o" "$A/hip_emu.o" "$HERE/admit_block_asan.cpp" -o "$OUT/admit_block_asan"
echo "$OUT/admit_block_asan"
