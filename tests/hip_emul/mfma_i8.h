// mfma_i8.h of tests/hip_emul -- TEST INFRASTRUCTURE ONLY: the int8 matrix instruction for the CPU stand-in of
// hip/hip_runtime.h, force-included by build_match.sh (-include) in front of colmap_amd/csrc/feature_match.hip.
//
// v_mfma_i32_16x16x64_i8: D = A (16 x 64) * B (64 x 16) + C over one wave, int8 operands, int32 accumulation (wrapping,
// no saturation). Lane maps as colmap_amd/csrc/feature_match.hip assumes them:
//   A: lane l holds row l & 15, its 16 bytes are k = 16 (l >> 4) + 0..15 (byte b of the 4 dwords in memory order);
//   B: lane l holds column l & 15, the same k;
//   C / D: register r of lane l is row 4 (l >> 4) + r, column l & 15.
// The kernel loads A and B alike, so its result does not depend on the k order inside a lane's 16 bytes; the row and
// column maps are what the GPU test's asymmetric case pins down on the hardware.
#pragma once
#include <hip/hip_runtime.h>

typedef int hip_emul_v4i32 __attribute__((ext_vector_type(4)));

inline hip_emul_v4i32 hip_emul_mfma_i32_16x16x64_i8(hip_emul_v4i32 a, hip_emul_v4i32 b, hip_emul_v4i32 c) {
  static signed char As[16][16][64], Bs[16][16][64];  // [wave of the block][row / column][k]
  const int l = hip_emul::lane_id();
  signed char (*A)[64] = As[hip_emul::wave_id()];
  signed char (*B)[64] = Bs[hip_emul::wave_id()];
  hip_emul::wave_barrier();  // the previous call's readers are done
  std::memcpy(&A[l & 15][16 * (l >> 4)], &a, 16);
  std::memcpy(&B[l & 15][16 * (l >> 4)], &b, 16);
  hip_emul::wave_barrier();
  const int j = l & 15;
  for (int r = 0; r < 4; ++r) {
    const int i = 4 * (l >> 4) + r;
    unsigned acc = (unsigned)c[r];
    for (int k = 0; k < 64; ++k) acc += (unsigned)((int)A[i][k] * (int)B[j][k]);
    c[r] = (int)acc;
  }
  return c;
}
#define __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, cbsz, abid, blgp) hip_emul_mfma_i32_16x16x64_i8((a), (b), (c))
