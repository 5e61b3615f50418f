#!/bin/sh
# Builds tests/hip_emul/libmatch_emul.so: colmap_amd/csrc/feature_match.hip (unmodified) against the CPU stand-in headers
# of this directory, with ROCm's clang++ as the HOST compiler (like build_align.sh). mfma_i8.h, the stand-in of the int8
# matrix instruction, is force-included in front of the source.
# TEST INFRASTRUCTURE ONLY -- see hip/hip_runtime.h.
set -e
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
cxx=${HIP_EMUL_CXX:-/opt/rocm/lib/llvm/bin/clang++}
"$cxx" -O2 -g -std=c++17 -fPIC -shared -mavx2 -mfma -ffp-contract=off -fno-fast-math -fvisibility=hidden \
    -Wall -Wno-unknown-pragmas -Wno-unused-function -Wno-unknown-attributes -I "$here" -I "$root/colmap_amd/csrc" \
    -include "$here/mfma_i8.h" -x c++ "$root/colmap_amd/csrc/feature_match.hip" -o "$here/libmatch_emul.so"
