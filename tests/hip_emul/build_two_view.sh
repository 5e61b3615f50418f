#!/bin/sh
# Builds tests/hip_emul/libtwo_view_emul.so: colmap_amd/csrc/two_view.hip (unmodified) against the CPU stand-in headers
# of this directory, with ROCm's clang++ as the HOST compiler (like build_align.sh).
# TEST INFRASTRUCTURE ONLY -- see hip/hip_runtime.h.
set -e
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
cxx=${HIP_EMUL_CXX:-/opt/rocm/lib/llvm/bin/clang++}
"$cxx" -O2 -g -std=c++17 -fPIC -shared -mavx2 -mfma -ffp-contract=off -fno-fast-math -fvisibility=hidden \
    -Wall -Wno-unknown-pragmas -Wno-unused-function -Wno-unknown-attributes -I "$here" -I "$root/colmap_amd/csrc" \
    -x c++ "$root/colmap_amd/csrc/two_view.hip" -o "$here/libtwo_view_emul.so"
