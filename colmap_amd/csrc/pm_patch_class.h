// pm_patch_class.h -- the classes of an NCC task of the 11 x 11 wave kernels, decided in pass A (lane per task) from
// the task's centred homography: inside (unclamped tap addressing), clamped (everything else that is evaluated), and
// answered (the three window sums are known to be exactly +0, or the cost is known to be 2.0f, before the first tap).
// Plain host / device inline C++: pm_kernels.hip includes it, tests/cpp/test_pm_patch_class.cc checks the predicates
// against a restatement of the per-tap arithmetic without a GPU.
#ifndef COLMAP_AMD_PM_PATCH_CLASS_H_
#define COLMAP_AMD_PM_PATCH_CLASS_H_

#include "pm_host_plan.h"  // PmParams

#if defined(__HIPCC__)
#define PM_CLASS_FN __host__ __device__ __forceinline__
#else
#define PM_CLASS_FN inline
#endif

namespace colmap_amd {

// Does every tap of the patch with (centred) homography Hm provably fall on texels x in [0, w - 1],
// y in [0, h - 1] of the source image? The window maps to a convex quadrilateral when the projective
// divisor is positive at its four corners, so the taps lie inside the corners' bounding box; one
// texel of margin absorbs the rounding of the per-tap evaluation. NaNs compare false.
PM_CLASS_FN bool patch_inside(const PmParams& p, const float Hm[9]) {
  // With z > 0 at a corner, 1 <= x / z <= w - 2 is z <= x <= (w - 2) z: eight divisions saved per task. The
  // flag only selects the addressing variant of the gathers (both give the same texels for a patch that is
  // inside; the one-texel margin dwarfs the rounding of the products), it never changes a result -- so the corner
  // values are taken incrementally (two products and three sums per coordinate instead of eight and eight).
  const float e = (float)(2 * p.radius);  // window extent: taps at offsets 0 .. 2 r
  const float wx = (float)(p.src_w - 2), wy = (float)(p.src_h - 2);
  float x[4], y[4], z[4];
  {
    const float a = Hm[0] * e, b = Hm[1] * e;
    x[0] = Hm[2]; x[1] = a + x[0]; x[2] = b + x[0]; x[3] = a + x[2];
  }
  {
    const float a = Hm[3] * e, b = Hm[4] * e;
    y[0] = Hm[5]; y[1] = a + y[0]; y[2] = b + y[0]; y[3] = a + y[2];
  }
  {
    const float a = Hm[6] * e, b = Hm[7] * e;
    z[0] = Hm[8]; z[1] = a + z[0]; z[2] = b + z[0]; z[3] = a + z[2];
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    ok = ok && (z[k] > 0.0f) && x[k] >= z[k] && y[k] >= z[k] && x[k] <= wx * z[k] && y[k] <= wy * z[k];
  return ok;
}

// The "outside" rule of an answered task: does every tap of the patch provably read an all-zero entry of the packed
// image's ring (ncc_front<false>: the clamp of floor(px) to [-2, w] lands on -2 or w, in x or in y) with FINITE
// bilinear fractions? Then every texel is 0, every product of the window sums is +0 and the sums are exactly
// (+0, +0, +0): pass A writes them and pass B never runs the task. A non-finite coordinate would make the fraction
// px - floor(px) NaN and the sums NaN, so finiteness is part of the claim. The predicate may refuse any patch; it must
// never accept one whose sums are not +0.
//
// Accepted: with the four window corners (x[k], y[k], z[k]) and the edge vectors a = H[.] * e, b = H[.] * e as
// patch_inside forms them,
//   (1) image no larger than kAnsMaxSize;
//   (2) |a|, |b| and the origin term of the x and y rows <= kAnsTerm (so every corner is finite, at most 3 B);
//   (3) |a|, |b| of the z row <= kAnsZEdge and kAnsZLo <= min z[k], max z[k] <= kAnsZHi;
//   (4) ONE edge that all four corners are beyond by kAnsMargin texels, tested against the largest divisor (z > 0:
//       x[k] <= max x <= -(1 + m) max z <= -(1 + m) z[k], and so on):
//       max x <= -(1 + m) max z  |  min x >= (w + m) max z  |  max y <= -(1 + m) max z  |  min y >= (h + m) max z.
// Error bound (u = 2^-24, B = kAnsTerm = 2^18, m = 8, w <= 8192; X, Y, Z = the exact affine maps of the float
// homography over the window, whose extreme values are taken at the corners):
//   * corners: the float z[k] differ from Z by at most (32 + 32 + 16 + 16) u < 2^-17, x[k] from X by at most
//     (B + B + 2 B + 3 B) u < 0.11 (the roundings of a, b and of the two sums); the product (1 + m) max z is off by
//     at most 9 * 16 u, (w + m) max z by 8200 * 16 u. So X + (1 + m) Z <= 9 * (2^-17 + 16 u) + 0.11 < 0.111 at every
//     corner, hence at every tap (affine), and likewise (w + m) Z - X <= 8200 * (2^-17 + 16 u) + 0.11 < 0.181.
//   * a tap's divisor fma(h6, dx, fma(h7, dy, h8)) differs from Z by at most 64 u + 16 u < 2^-18: it lies in
//     [1/16 - 2^-16, 16 + 2^-16]. The eight-term product `run` therefore lies in [2^-33, 2^33], its reciprocal `rinv`
//     likewise, pre * suf (seven terms) in [2^-29, 2^29] and (pre * suf) * rinv = (1 / z)(1 + d), |d| <= 18 u < 2^-19:
//     no overflow, no underflow, no NaN. Lanes beyond the window (divisor forced to 1, dx = dy = 0) get (1 + d) and
//     the finite numerators h2, h5.
//   * a tap's numerator fma(h0, dx, fma(h1, dy, h2)) differs from X by at most 2 B u + 3 B u < 0.079 and is at most
//     3 B in magnitude, so |px|, |py| <= 3 B * 16.01 < 2^24: finite, as are floor and fraction.
//   * left / above: numerator c <= -(1 + m) Z + 0.111 + 0.079 <= -9 (z - 2^-17) + 0.19 and px = (c / z)(1 + d')
//     with |d'| < 2^-18; px < -1 needs c <= -z (1 + 2^-17), i.e. 8 z >= 0.191: true for z >= 1/16 - 2^-16 with a
//     factor of 2.6 to spare. floor(px) <= -2, the clamp gives entry -2.
//   * right / below: c >= (w + m)(z - 2^-17) - 0.181 - 0.079; px >= w needs c >= w z (1 + 2^-17), i.e.
//     m z >= w z 2^-17 + (w + m) 2^-17 + 0.26: with w <= 8192 that is 7.94 z >= 0.323, true for z >= 0.041.
//     floor(px) >= w, the clamp gives entry w.
// NaNs and infinities anywhere in Hm fail a comparison of (2) or (3) and are refused: after (2) and the edge bound of
// (3) only z[k] can still be non-finite, all four alike (they share Hm[8]), and then min / max are too.
constexpr float kAnsZLo = 0.0625f, kAnsZHi = 16.0f, kAnsZEdge = 32.0f;
constexpr float kAnsTerm = 262144.0f;  // 2^18
constexpr float kAnsMargin = 8.0f;
constexpr int kAnsMaxSize = 8192;

PM_CLASS_FN bool patch_outside(const PmParams& p, const float Hm[9]) {
  const float e = (float)(2 * p.radius);
  float x[4], y[4], z[4];
  bool ok = p.src_w <= kAnsMaxSize && p.src_h <= kAnsMaxSize;
  {
    const float a = Hm[0] * e, b = Hm[1] * e;
    x[0] = Hm[2]; x[1] = a + x[0]; x[2] = b + x[0]; x[3] = a + x[2];
    ok = ok && fabsf(a) <= kAnsTerm && fabsf(b) <= kAnsTerm && fabsf(x[0]) <= kAnsTerm;
  }
  {
    const float a = Hm[3] * e, b = Hm[4] * e;
    y[0] = Hm[5]; y[1] = a + y[0]; y[2] = b + y[0]; y[3] = a + y[2];
    ok = ok && fabsf(a) <= kAnsTerm && fabsf(b) <= kAnsTerm && fabsf(y[0]) <= kAnsTerm;
  }
  {
    const float a = Hm[6] * e, b = Hm[7] * e;
    z[0] = Hm[8]; z[1] = a + z[0]; z[2] = b + z[0]; z[3] = a + z[2];
    ok = ok && fabsf(a) <= kAnsZEdge && fabsf(b) <= kAnsZEdge;
  }
  const float zmin = fminf(fminf(z[0], z[1]), fminf(z[2], z[3])), zmax = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
  const float xmin = fminf(fminf(x[0], x[1]), fminf(x[2], x[3])), xmax = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
  const float ymin = fminf(fminf(y[0], y[1]), fminf(y[2], y[3])), ymax = fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3]));
  ok = ok && zmin >= kAnsZLo && zmax <= kAnsZHi;
  const float lo = -(1.0f + kAnsMargin) * zmax;
  const float hx = ((float)p.src_w + kAnsMargin) * zmax, hy = ((float)p.src_h + kAnsMargin) * zmax;
  return ok && (xmax <= lo || xmin >= hx || ymax <= lo || ymin >= hy);
}

// The "flat reference" rule: ncc_finish returns 2.0f for this pixel before it looks at the source sums. Same
// expression, same operands (the caller passes what it will pass to ncc_finish).
PM_CLASS_FN bool ref_flat(float ref_sum, float ref_sqsum) {
  const float ref_var = ref_sqsum - ref_sum * ref_sum;
  return ref_var < 1e-5f;
}

PM_CLASS_FN bool patch_answered(const PmParams& p, const float Hm[9], float ref_sum, float ref_sqsum) {
  return ref_flat(ref_sum, ref_sqsum) || patch_outside(p, Hm);
}

}  // namespace colmap_amd

#endif  // COLMAP_AMD_PM_PATCH_CLASS_H_
