// two_view_solvers.h -- what two-view geometry estimation evaluates per sample and per match, once, for host and
// device (shared as camera_projection.h is): the sample draw, the three minimal solvers and the three residuals.
// two_view.hip runs them one lane per trial / per model; two_view_plan.h redraws samples on the host; the numpy
// checker tests/two_view_reference.py restates the draw and the residuals operation by operation.
//
// Restates (reference src/colmap):
//   estimators/solvers/fundamental_matrix.cc:47-114   FundamentalMatrixSevenPointEstimator::Estimate
//   math/polynomial.cc:143-180                        FindCubicPolynomialRoots
//   estimators/solvers/homography_matrix.cc:45-96     HomographyMatrixEstimator::Estimate, the 4-point branch
//   estimators/solvers/translation_transform.h:79-118 TranslationTransformEstimator<2>
//   geometry/essential_matrix.cc:168-182              ComputeSquaredSampsonError
//   estimators/solvers/homography_matrix.cc:98-135    HomographyMatrixEstimator::Residuals
// All three model kinds are 9 doubles: F and H row-major, T in the first two.
//
// The residuals use + - * / only and the build has -ffp-contract=off: every residual has one value, on the host, on
// gfx950 and in numpy. The solvers call sqrt, cbrt, acos and cos, whose last bit may differ between libms.
//
// The sample stream: sample (random_seed, stream_id, kind, trial) is a pure function of its four arguments, a
// splitmix64-style counter hash; indices are drawn below n and repeats rejected. The reference's RandomSampler shuffles
// with std::mt19937, whose stream through std::uniform_int_distribution is implementation-defined; it is not reproduced.
// random_seed -1 (the reference's "nondeterministic") is treated as 0: results are always reproducible.
#ifndef COLMAP_AMD_TWO_VIEW_SOLVERS_H_
#define COLMAP_AMD_TWO_VIEW_SOLVERS_H_

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TVS_HD __host__ __device__ inline
#else
#define TVS_HD inline
#endif

namespace tvs {

enum Kind { KIND_F = 0, KIND_H = 1, KIND_T = 2 };

constexpr int kMaxModels = 3;  // models of one minimal sample (the cubic of the 7-point solver)

TVS_HD int min_samples(int kind) { return kind == KIND_F ? 7 : kind == KIND_H ? 4 : 1; }
// LocalEstimator::kMinNumSamples: 8-point F, DLT H, mean T
TVS_HD int local_min_samples(int kind) { return kind == KIND_F ? 8 : kind == KIND_H ? 4 : 1; }

// ---------------------------------------------------------------------------------------------------------------------
// the sample draw
// ---------------------------------------------------------------------------------------------------------------------

TVS_HD uint64_t mix64(uint64_t z) {  // the finalizer of splitmix64
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

TVS_HD uint64_t sample_key(int32_t random_seed, uint64_t stream_id, int kind, uint64_t trial) {
  uint64_t h = mix64((uint64_t)(random_seed < 0 ? 0 : random_seed) + 0x9E3779B97F4A7C15ull);
  h = mix64(h ^ stream_id);
  h = mix64(h ^ (uint64_t)kind);
  return mix64(h ^ trial);
}

// min_samples(kind) distinct indices below n, n >= min_samples(kind) (the callers check): value c of the stream is
// mix64(key + c * golden) % n; a value that repeats an accepted index is skipped.
TVS_HD void draw_sample(int32_t random_seed, uint64_t stream_id, int kind, uint64_t trial, uint32_t n, uint32_t idx[7]) {
  const uint64_t key = sample_key(random_seed, stream_id, kind, trial);
  const int k = min_samples(kind);
  uint64_t c = 0;
  for (int j = 0; j < k; ++j) {
    for (;;) {
      const uint32_t v = (uint32_t)(mix64(key + c * 0x9E3779B97F4A7C15ull) % (uint64_t)n);
      ++c;
      bool repeat = false;
      for (int i = 0; i < 7; ++i) repeat = repeat || (i < j && idx[i] == v);
      if (!repeat) {
        idx[j] = v;
        break;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// residuals; every sum is evaluated left to right
// ---------------------------------------------------------------------------------------------------------------------

// ComputeSquaredSampsonError of (x1, y1, 1), (x2, y2, 1) under x2^T F x1 = 0
TVS_HD double sampson_error(const double F[9], double x1, double y1, double x2, double y2) {
  const double l0 = F[0] * x1 + F[1] * y1 + F[2];
  const double l1 = F[3] * x1 + F[4] * y1 + F[5];
  const double l2 = F[6] * x1 + F[7] * y1 + F[8];
  const double num = x2 * l0 + y2 * l1 + l2;
  const double d0 = x2 * F[0] + y2 * F[3] + F[6];
  const double d1 = x2 * F[1] + y2 * F[4] + F[7];
  const double denom = d0 * d0 + d1 * d1 + l0 * l0 + l1 * l1;
  if (denom == 0.0) return DBL_MAX;
  return num * num / denom;
}

// forward transfer error; a NaN (0 * inf) is an outlier of every `<=` test
TVS_HD double homography_error(const double H[9], double x1, double y1, double x2, double y2) {
  const double pd_0 = H[0] * x1 + H[1] * y1 + H[2];
  const double pd_1 = H[3] * x1 + H[4] * y1 + H[5];
  const double pd_2 = H[6] * x1 + H[7] * y1 + H[8];
  const double inv_pd_2 = 1.0 / pd_2;
  const double dd_0 = x2 - pd_0 * inv_pd_2;
  const double dd_1 = y2 - pd_1 * inv_pd_2;
  return dd_0 * dd_0 + dd_1 * dd_1;
}

TVS_HD double translation_error(const double T[9], double x1, double y1, double x2, double y2) {
  const double dx = x2 - x1 - T[0];
  const double dy = y2 - y1 - T[1];
  return dx * dx + dy * dy;
}

TVS_HD double residual(int kind, const double M[9], double x1, double y1, double x2, double y2) {
  return kind == KIND_F ? sampson_error(M, x1, y1, x2, y2)
                        : kind == KIND_H ? homography_error(M, x1, y1, x2, y2) : translation_error(M, x1, y1, x2, y2);
}

// ---------------------------------------------------------------------------------------------------------------------
// minimal solvers. `W` is the working storage of one solve: W(k) is a double&, k < kWorkDoubles. The index is a
// run-time pivot, so the device hands in LDS (lane-minor: a wave's accesses fall in distinct banks) and never a
// private array, which would live in scratch; the host hands in a plain array.
// ---------------------------------------------------------------------------------------------------------------------

constexpr int kWorkDoubles = 81;  // 7 x 9 system + two null vectors (F); 8 x 9 augmented system (H)

// FindCubicPolynomialRoots: x^3 + c2 x^2 + c1 x + c0, one Newton step on every root
TVS_HD int cubic_roots(double c2, double c1, double c0, double real[3]) {
  const double k2PiOver3 = 2.09439510239319526263557236234192;
  const double k4PiOver3 = 4.18879020478639052527114472468384;
  const double c2_over_3 = c2 / 3.0;
  const double a = c1 - c2 * c2_over_3;
  double b = (2.0 * c2 * c2 * c2 - 9.0 * c2 * c1) / 27.0 + c0;
  double c = b * b / 4.0 + a * a * a / 27.0;
  int num_roots = 0;
  if (c > 0) {
    c = sqrt(c);
    b *= -0.5;
    real[0] = cbrt(b + c) + cbrt(b - c) - c2_over_3;
    num_roots = 1;
  } else {
    c = 3.0 * b / (2.0 * a) * sqrt(-3.0 / a);
    const double d = 2.0 * sqrt(-a / 3.0);
    const double acos_over_3 = acos(c) / 3.0;
    real[0] = d * cos(acos_over_3) - c2_over_3;
    real[1] = d * cos(acos_over_3 - k2PiOver3) - c2_over_3;
    real[2] = d * cos(acos_over_3 - k4PiOver3) - c2_over_3;
    num_roots = 3;
  }
  for (int i = 0; i < num_roots; ++i) {
    const double x = real[i];
    const double x2 = x * x;
    const double x3 = x * x2;
    const double dx = -(x3 + c2 * x2 + c1 * x + c0) / (3 * x2 + 2 * c2 * x + c1);
    real[i] += dx;
  }
  return num_roots;
}

// The 7-point solver. The null space of the 7 x 9 system comes from Gauss-Jordan elimination with full pivoting: any
// basis of the null space spans the same pencil lambda f1 + (1 - lambda) f2, so Eigen's full-pivot QR is not
// imitated. A system of rank below 7 (an exactly zero pivot: repeated points) gives no model. Returns the number of
// models; models[m] is row-major and of unit Frobenius norm.
template <typename Work>
TVS_HD int solve_f7(Work& W, const double x1[7], const double y1[7], const double x2[7], const double y2[7],
                    double models[kMaxModels][9]) {
  // row i: [x2 F x1] in the unknown order of the reference, f[3 c + r] = F(r, c)
  for (int i = 0; i < 7; ++i) {
    W(9 * i + 0) = x1[i] * x2[i];
    W(9 * i + 1) = x1[i] * y2[i];
    W(9 * i + 2) = x1[i];
    W(9 * i + 3) = y1[i] * x2[i];
    W(9 * i + 4) = y1[i] * y2[i];
    W(9 * i + 5) = y1[i];
    W(9 * i + 6) = x2[i];
    W(9 * i + 7) = y2[i];
    W(9 * i + 8) = 1.0;
  }
  uint64_t perm = 0x876543210ull;  // nibble j: the unknown that column j holds
  for (int k = 0; k < 7; ++k) {
    int pr = k, pc = k;
    double best = -1.0;
    for (int r = k; r < 7; ++r)
      for (int c = k; c < 9; ++c) {
        const double v = fabs(W(9 * r + c));
        if (v > best) {  // a NaN never wins; the first of equal magnitudes does
          best = v;
          pr = r;
          pc = c;
        }
      }
    if (!(best > 0.0)) return 0;
    if (pr != k)
      for (int c = 0; c < 9; ++c) {
        const double t = W(9 * k + c);
        W(9 * k + c) = W(9 * pr + c);
        W(9 * pr + c) = t;
      }
    if (pc != k) {
      for (int r = 0; r < 7; ++r) {
        const double t = W(9 * r + k);
        W(9 * r + k) = W(9 * r + pc);
        W(9 * r + pc) = t;
      }
      const uint64_t a = (perm >> (4 * k)) & 15ull, b = (perm >> (4 * pc)) & 15ull;
      perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * pc)))) | (b << (4 * k)) | (a << (4 * pc));
    }
    const double pivot = W(9 * k + k);
    for (int r = 0; r < 7; ++r) {
      if (r == k) continue;
      const double f = W(9 * r + k) / pivot;
      for (int c = k; c < 9; ++c) W(9 * r + c) = W(9 * r + c) - f * W(9 * k + c);
    }
  }
  // null vector of free column j: 1 at its unknown, -A(i, j) / A(i, i) at the unknown of pivot column i
  for (int j = 0; j < 2; ++j) {
    for (int i = 0; i < 7; ++i) W(63 + 9 * j + (int)((perm >> (4 * i)) & 15ull)) = -W(9 * i + 7 + j) / W(9 * i + i);
    W(63 + 9 * j + (int)((perm >> (4 * (7 + j))) & 15ull)) = 1.0;
    W(63 + 9 * j + (int)((perm >> (4 * (8 - j))) & 15ull)) = 0.0;
  }
  double f1[9], f2[9];
  for (int k = 0; k < 9; ++k) {
    f2[k] = W(72 + k);
    f1[k] = W(63 + k) - f2[k];
  }
  const double t0 = f1[4] * f1[8] - f1[5] * f1[7];
  const double t1 = f1[3] * f1[8] - f1[5] * f1[6];
  const double t2 = f1[3] * f1[7] - f1[4] * f1[6];
  const double t3 = f2[4] * f2[8] - f2[5] * f2[7];
  const double t4 = f2[3] * f2[8] - f2[5] * f2[6];
  const double t5 = f2[3] * f2[7] - f2[4] * f2[6];
  double coeffs[4];
  coeffs[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
  if (fabs(coeffs[0]) < 1e-16) return 0;
  coeffs[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
              f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) - f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
              f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
              f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
  coeffs[2] = f1[0] * t3 - f1[1] * t4 + f1[2] * t5 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
              f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) - f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
              f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
              f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
  coeffs[3] = f2[0] * t3 - f2[1] * t4 + f2[2] * t5;
  double roots[3];
  const int num_roots = cubic_roots(coeffs[1] / coeffs[0], coeffs[2] / coeffs[0], coeffs[3] / coeffs[0], roots);
  for (int m = 0; m < num_roots; ++m) {
    double f[9], n2 = 0.0;
    for (int k = 0; k < 9; ++k) {
      f[k] = f1[k] * roots[m] + f2[k];
      n2 += f[k] * f[k];
    }
    const double n = sqrt(n2);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) models[m][3 * r + c] = n > 0.0 ? f[3 * c + r] / n : f[3 * c + r];
  }
  return num_roots;
}

// The 4-point solver: the 8 x 8 system of the DLT with h22 = 1, by elimination with partial pivoting; the reference's
// NaN reject (here: an exactly zero pivot, or a NaN in the solution) and its |det H| < 1e-8 reject.
template <typename Work>
TVS_HD int solve_h4(Work& W, const double x1[4], const double y1[4], const double x2[4], const double y2[4],
                    double model[9]) {
  for (int i = 0; i < 4; ++i) {
    const int a = 18 * i, b = 18 * i + 9;
    W(a + 0) = x1[i];
    W(a + 1) = y1[i];
    W(a + 2) = 1.0;
    W(a + 3) = 0.0;
    W(a + 4) = 0.0;
    W(a + 5) = 0.0;
    W(a + 6) = -x2[i] * x1[i];
    W(a + 7) = -x2[i] * y1[i];
    W(a + 8) = x2[i];  // right-hand side: -A(., 8)
    W(b + 0) = 0.0;
    W(b + 1) = 0.0;
    W(b + 2) = 0.0;
    W(b + 3) = x1[i];
    W(b + 4) = y1[i];
    W(b + 5) = 1.0;
    W(b + 6) = -y2[i] * x1[i];
    W(b + 7) = -y2[i] * y1[i];
    W(b + 8) = y2[i];
  }
  for (int k = 0; k < 8; ++k) {
    int pr = k;
    double best = -1.0;
    for (int r = k; r < 8; ++r) {
      const double v = fabs(W(9 * r + k));
      if (v > best) {
        best = v;
        pr = r;
      }
    }
    if (!(best > 0.0)) return 0;
    if (pr != k)
      for (int c = 0; c < 9; ++c) {
        const double t = W(9 * k + c);
        W(9 * k + c) = W(9 * pr + c);
        W(9 * pr + c) = t;
      }
    const double pivot = W(9 * k + k);
    for (int r = k + 1; r < 8; ++r) {
      const double f = W(9 * r + k) / pivot;
      for (int c = k; c < 9; ++c) W(9 * r + c) = W(9 * r + c) - f * W(9 * k + c);
    }
  }
  double h[9];
  h[8] = 1.0;
  bool nan = false;
  for (int k = 7; k >= 0; --k) {
    double s = W(9 * k + 8);
    for (int c = k + 1; c < 8; ++c) s = s - W(9 * k + c) * h[c];
    h[k] = s / W(9 * k + k);
    nan = nan || h[k] != h[k];
  }
  if (nan) return 0;
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) +
                     h[2] * (h[3] * h[7] - h[4] * h[6]);
  if (fabs(det) < 1e-8) return 0;
  for (int k = 0; k < 9; ++k) model[k] = h[k];
  return 1;
}

TVS_HD void solve_t1(double x1, double y1, double x2, double y2, double model[9]) {
  model[0] = x2 - x1;
  model[1] = y2 - y1;
  for (int k = 2; k < 9; ++k) model[k] = 0.0;
}

}  // namespace tvs

#endif  // COLMAP_AMD_TWO_VIEW_SOLVERS_H_
