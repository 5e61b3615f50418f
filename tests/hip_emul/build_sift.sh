#!/bin/sh
# Builds tests/hip_emul/libsift_emul.so: colmap_amd/csrc/sift.hip (unmodified) against the CPU stand-in headers of this
# directory (hipcub: sift/hipcub/hipcub.hpp, which has SortKeys), with ROCm's clang++ as the HOST compiler (like
# build_two_view.sh).
# TEST INFRASTRUCTURE ONLY -- see hip/hip_runtime.h.
set -e
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
cxx=${HIP_EMUL_CXX:-/opt/rocm/lib/llvm/bin/clang++}
"$cxx" -O2 -g -std=c++17 -fPIC -shared -mavx2 -mfma -ffp-contract=off -fno-fast-math -fvisibility=hidden \
    -Wall -Wno-unknown-pragmas -Wno-unused-function -Wno-unknown-attributes -I "$here/sift" -I "$here" -I "$root/colmap_amd/csrc" \
    -x c++ "$root/colmap_amd/csrc/sift.hip" -o "$here/libsift_emul.so"
