// hipcub.hpp of tests/hip_emul/sift -- TEST INFRASTRUCTURE ONLY (see ../../hip/hip_runtime.h): the one device-wide
// primitive colmap_amd/csrc/sift.hip uses, on the CPU. build_sift.sh puts this directory in front of tests/hip_emul on
// the include path, so that `#include <hipcub/hipcub.hpp>` of the unmodified source finds this file.
#pragma once
#include <algorithm>

#include "../../hip/hip_runtime.h"

namespace hipcub {
struct DeviceRadixSort {
  template <typename K>
  static hipError_t SortKeys(void* tmp, size_t& bytes, const K* kin, K* kout, int n, int = 0, int = 8 * (int)sizeof(K),
                             hipStream_t = nullptr) {
    if (!tmp) { bytes = 1; return hipSuccess; }
    std::copy(kin, kin + n, kout);
    std::sort(kout, kout + n);
    return hipSuccess;
  }
};
}  // namespace hipcub
