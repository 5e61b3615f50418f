// two_view_plan.h -- everything two-view geometry estimation decides on the host: the checks on the caller's arrays and
// options, the wave-padded layout of a batch of point sets, the router of EstimateTwoViewGeometry, RANSAC's stopping
// rule, the LORANSAC walk over a whole batch of sets, the local estimators and the decisions that turn search reports
// into a TwoViewGeometry. Plain C++17: no HIP runtime -- two_view.hip implements `Backend` with launches;
// tests/cpp/test_two_view_plan.cc drives the same walk with a scripted backend without a GPU.
//
// The walk is optim/loransac.h:131-393 of the reference with InlierSupportMeasurer (optim/support_measurement.cc:36-61)
// for a minimal estimator that returns 0 to 3 models per sample and a local estimator of its own: per trial, every
// model of the sample is compared with the best support; a better one is refitted on its inlier set up to 10 times,
// stopping at the first refit that does not improve; the stopping check (:344-349) sits INSIDE the loop over a
// sample's models, so a sample without a model never stops the search; ComputeNumTrials (optim/ransac.h:179-210) is
// evaluated for the minimal estimator's sample size, with the constructor's clamp (:167-175).
// What differs is HOW the trials are evaluated, not what is decided. The search runs for all sets of a batch at once,
// in rounds: every unfinished set has its next T trials hypothesized and scored in one launch pair; the host then
// walks each set's trials in trial order. A walk that meets a model better than its best parks with a scoring request
// (the model with its mask, then each refit with its mask); the requests of all parked walks go to the device in one
// launch and the walks resume. What lies past a set's stopping trial is thrown away. A model's score depends on its
// set and on nothing else of the launch, the refits do not touch the sample stream, so a set's report is the same for
// every T and every batch composition.
//
// The local estimators take their null vectors from a one-sided (Hestenes) Jacobi SVD of the system matrix itself,
// never from an eigen-decomposition of A^T A: the homography system is in pixel units with a condition number around
// 1e6, and its square leaves nothing of the null vector in double precision.
#ifndef COLMAP_AMD_TWO_VIEW_PLAN_H_
#define COLMAP_AMD_TWO_VIEW_PLAN_H_

#include "../../include/colmap_amd/camera_models.hpp"
#include "../../include/colmap_amd_tvg.h"
#include "two_view_solvers.h"

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace two_view_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define TVG_CHECK(cond, msg)                                                         \
  do {                                                                               \
    if (!(cond)) throw ::two_view_plan::Fail(std::string("Check failed: ") + (msg)); \
  } while (0)

constexpr int kWave = 64;
constexpr int kMaxNumLocalTrials = 10;  // loransac.h:261
constexpr int kDefaultTrialRound = 64;  // trials of a set per round
constexpr int kMaxTrialRound = 4096;
constexpr uint64_t kNoLimit = std::numeric_limits<uint64_t>::max();

using Model = std::array<double, 9>;

// InlierSupportMeasurer::Support and IsLeftBetter
struct Support {
  uint64_t num_inliers = 0;
  double residual_sum = DBL_MAX;
};

inline bool is_left_better(const Support& l, const Support& r) {
  if (l.num_inliers > r.num_inliers) return true;
  return l.num_inliers == r.num_inliers && l.residual_sum < r.residual_sum;
}

// ---------------------------------------------------------------------------------------------------------------------
// checks
// ---------------------------------------------------------------------------------------------------------------------

inline void check_kind(int kind) { TVG_CHECK(kind >= 0 && kind <= 2, "kind must be TVG_KIND_F, TVG_KIND_H or TVG_KIND_T"); }

// RANSACOptions::Check (optim/ransac.h:85-95) and the range of this implementation's own field
inline void validate_ransac(const tvg_ransac_options& o) {
  TVG_CHECK(o.max_error > 0.0, "max_error must be positive");
  TVG_CHECK(o.min_inlier_ratio >= 0.0 && o.min_inlier_ratio <= 1.0, "min_inlier_ratio must lie in [0, 1]");
  TVG_CHECK(o.confidence >= 0.0 && o.confidence <= 1.0, "confidence must lie in [0, 1]");
  TVG_CHECK(o.dyn_num_trials_multiplier > 0.0, "dyn_num_trials_multiplier must be positive");
  TVG_CHECK(o.min_num_trials >= 0, "min_num_trials must not be negative");
  TVG_CHECK(o.min_num_trials <= o.max_num_trials, "min_num_trials must not exceed max_num_trials");
  TVG_CHECK(o.random_seed >= -1, "random_seed must be -1 or larger");
  TVG_CHECK(o.trials_per_round >= 0 && o.trials_per_round <= kMaxTrialRound, "trials_per_round must lie in [0, 4096]");
}

// TwoViewGeometryOptions::Check (estimators/two_view_geometry.cc:530-550)
inline void validate_options(const tvg_options& o) {
  validate_ransac(o.ransac);
  TVG_CHECK(o.min_num_inliers >= 0, "min_num_inliers must not be negative");
  TVG_CHECK(o.max_H_inlier_ratio >= 0.0 && o.max_H_inlier_ratio <= 1.0, "max_H_inlier_ratio must lie in [0, 1]");
  TVG_CHECK(o.watermark_min_inlier_ratio >= 0.0 && o.watermark_min_inlier_ratio <= 1.0,
            "watermark_min_inlier_ratio must lie in [0, 1]");
  TVG_CHECK(o.watermark_border_size >= 0.0 && o.watermark_border_size <= 1.0, "watermark_border_size must lie in [0, 1]");
  TVG_CHECK(o.watermark_detection_max_error > 0.0, "watermark_detection_max_error must be positive");
  TVG_CHECK(o.stationary_matches_max_error >= 0.0, "stationary_matches_max_error must not be negative");
}

inline void validate_offsets(int32_t num_sets, const int64_t* offsets, const void* points, const char* what) {
  TVG_CHECK(num_sets >= 0, std::string("the number of ") + what + " must not be negative");
  TVG_CHECK(offsets != nullptr, std::string("the offsets of the ") + what + " are null");
  TVG_CHECK(offsets[0] == 0, "the first offset must be 0");
  for (int32_t s = 0; s < num_sets; ++s) TVG_CHECK(offsets[s + 1] >= offsets[s], "the offsets must not decrease");
  TVG_CHECK(offsets[num_sets] < ((int64_t)1 << 31), "the matches of a batch must fit a 32-bit index");
  TVG_CHECK(offsets[num_sets] == 0 || points != nullptr, "the points are null");
}

inline void validate_camera(const tvg_camera& c, const std::string& what) {
  TVG_CHECK(colmap_amd::camera_models::num_params(c.model_id) >= 0, what + ": unknown camera model " + std::to_string(c.model_id));
  TVG_CHECK(c.width >= 0 && c.height >= 0, what + ": negative image size");
}

// ---------------------------------------------------------------------------------------------------------------------
// layout: every set's segment starts at a multiple of the wave size
// ---------------------------------------------------------------------------------------------------------------------

struct SetLayout {
  std::vector<int32_t> begin, count;  // [num_sets] first padded row and number of matches
  int64_t num_rows = 0;               // rows of the SoA arrays, padding included
};

inline SetLayout make_layout(int32_t num_sets, const int64_t* offsets) {
  SetLayout L;
  L.begin.resize((size_t)num_sets);
  L.count.resize((size_t)num_sets);
  int64_t row = 0;
  for (int32_t s = 0; s < num_sets; ++s) {
    const int64_t n = offsets[s + 1] - offsets[s];
    L.begin[(size_t)s] = (int32_t)row;
    L.count[(size_t)s] = (int32_t)n;
    row += (n + kWave - 1) / kWave * kWave;
    TVG_CHECK(row < ((int64_t)1 << 31), "the padded matches of a batch must fit a 32-bit index");
  }
  L.num_rows = row;
  return L;
}

// ---------------------------------------------------------------------------------------------------------------------
// the router: the if chain of two_view_geometry.cc:552-640 in its order
// ---------------------------------------------------------------------------------------------------------------------

namespace cm = colmap_amd::camera_models;

inline bool is_spherical(const tvg_camera& c) { return cm::is_spherical(c.model_id); }
inline bool is_perspective_pinhole(const tvg_camera& c) { return !cm::is_spherical(c.model_id) && !cm::is_fisheye(c.model_id); }
// IsCameraCalibrated (:64-66): a focal prior, or spherical and without a focal length at all
inline bool is_calibrated(const tvg_camera& c) { return is_spherical(c) || c.has_prior_focal_length != 0; }

inline int route(const tvg_camera& c1, const tvg_camera& c2, const tvg_options& o) {
  if (o.force_H_use) {
    if (!is_perspective_pinhole(c1) || !is_perspective_pinhole(c2)) return TVG_ROUTE_FORCED_H_DEGENERATE;
    return TVG_ROUTE_FORCED_H;
  }
  if (is_calibrated(c1) != is_calibrated(c2) && is_perspective_pinhole(is_calibrated(c1) ? c2 : c1))
    return TVG_ROUTE_ONE_SIDED_FOCAL;
  if (is_spherical(c1) || is_spherical(c2)) return TVG_ROUTE_SPHERICAL;
  if (c1.camera_id == c2.camera_id && !c1.has_prior_focal_length && is_perspective_pinhole(c1)) return TVG_ROUTE_SHARED_FOCAL;
  if (c1.has_prior_focal_length && c2.has_prior_focal_length) return TVG_ROUTE_CALIBRATED;
  if (!is_perspective_pinhole(c1) || !is_perspective_pinhole(c2)) return TVG_ROUTE_FISHEYE_DEGENERATE;
  return TVG_ROUTE_UNCALIBRATED;
}

inline const char* route_name(int r) {
  switch (r) {
    case TVG_ROUTE_FORCED_H_DEGENERATE: return "force_H_use with a non-pinhole camera (degenerate)";
    case TVG_ROUTE_FORCED_H: return "homography (force_H_use)";
    case TVG_ROUTE_ONE_SIDED_FOCAL: return "one-sided focal";
    case TVG_ROUTE_SPHERICAL: return "spherical";
    case TVG_ROUTE_SHARED_FOCAL: return "shared focal";
    case TVG_ROUTE_CALIBRATED: return "calibrated";
    case TVG_ROUTE_FISHEYE_DEGENERATE: return "perspective fisheye without a focal prior (degenerate)";
    case TVG_ROUTE_UNCALIBRATED: return "uncalibrated";
  }
  return "unknown";
}

inline bool route_is_built(int r) {
  return r == TVG_ROUTE_FORCED_H_DEGENERATE || r == TVG_ROUTE_FORCED_H || r == TVG_ROUTE_FISHEYE_DEGENERATE ||
         r == TVG_ROUTE_UNCALIBRATED;
}

// ---------------------------------------------------------------------------------------------------------------------
// RANSAC's trial budget
// ---------------------------------------------------------------------------------------------------------------------

// RANSAC::ComputeNumTrials (optim/ransac.h:179-210) for a minimal sample of min_samples
inline uint64_t compute_num_trials(uint64_t num_inliers, uint64_t num_samples, double confidence, double multiplier,
                                   int min_samples) {
  const double prob_failure = 1 - confidence;
  if (prob_failure <= 0) return kNoLimit;
  double prob_inlier = 1.0;
  for (int i = 0; i < min_samples; ++i)  // size_t arithmetic: num_inliers - i wraps below i, as there
    prob_inlier *= static_cast<double>(num_inliers - (uint64_t)i) / static_cast<double>(num_samples - (uint64_t)i);
  const double prob_outlier = 1 - prob_inlier;
  if (prob_outlier <= 0) return 1;
  if (prob_outlier == 1.0) return kNoLimit;
  const double v = std::ceil(std::log(prob_failure) / std::log(prob_outlier) * multiplier);
  if (!(v < 1.8446744073709552e19)) return kNoLimit;  // the cast of the reference is undefined there
  return v <= 0.0 ? 0 : static_cast<uint64_t>(v);
}

// the constructor's clamp (optim/ransac.h:167-175)
inline uint64_t clamped_max_num_trials(const tvg_ransac_options& o, double min_inlier_ratio, int min_samples) {
  const uint64_t kNumSamples = 100000;
  const uint64_t dyn = compute_num_trials(static_cast<uint64_t>(min_inlier_ratio * kNumSamples), kNumSamples, o.confidence,
                                          o.dyn_num_trials_multiplier, min_samples);
  return std::min<uint64_t>((uint64_t)o.max_num_trials, dyn);
}

// ---------------------------------------------------------------------------------------------------------------------
// one-sided (Hestenes) Jacobi SVD of an m x n matrix, n <= 9, held by columns. On return the columns of `a` are
// A V (mutually orthogonal, their norms the singular values) and `v` holds V by columns; `order` lists the columns by
// decreasing singular value.
// ---------------------------------------------------------------------------------------------------------------------

struct JacobiSvd {
  int n = 0;
  std::vector<std::vector<double>> a;  // [n][m]
  double v[9][9];                      // v[col][row]
  double sigma[9];
  int order[9];

  void compute() {
    for (int p = 0; p < n; ++p)
      for (int r = 0; r < n; ++r) v[p][r] = p == r ? 1.0 : 0.0;
    const size_t m = n ? a[0].size() : 0;
    for (int sweep = 0; sweep < 60; ++sweep) {
      bool rotated = false;
      for (int p = 0; p + 1 < n; ++p)
        for (int q = p + 1; q < n; ++q) {
          double alpha = 0.0, beta = 0.0, gamma = 0.0;
          for (size_t i = 0; i < m; ++i) {
            alpha += a[p][i] * a[p][i];
            beta += a[q][i] * a[q][i];
            gamma += a[p][i] * a[q][i];
          }
          if (!(std::fabs(gamma) > 1e-15 * std::sqrt(alpha * beta)) || gamma == 0.0) continue;
          rotated = true;
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
          for (size_t i = 0; i < m; ++i) {
            const double x = a[p][i], y = a[q][i];
            a[p][i] = c * x - s * y;
            a[q][i] = s * x + c * y;
          }
          for (int i = 0; i < n; ++i) {
            const double x = v[p][i], y = v[q][i];
            v[p][i] = c * x - s * y;
            v[q][i] = s * x + c * y;
          }
        }
      if (!rotated) break;
    }
    for (int p = 0; p < n; ++p) {
      double s2 = 0.0;
      for (size_t i = 0; i < m; ++i) s2 += a[p][i] * a[p][i];
      sigma[p] = std::sqrt(s2);
      order[p] = p;
    }
    std::stable_sort(order, order + n, [&](int l, int r) { return sigma[l] > sigma[r]; });
  }
  // Eigen's SVDBase::rank(): singular values above max(rows, cols) * epsilon relative to the largest
  int rank(size_t rows) const {
    const double thr = (double)std::max<size_t>(rows, (size_t)n) * std::numeric_limits<double>::epsilon();
    const double cut = std::max(sigma[order[0]] * thr, std::numeric_limits<double>::min());
    int r = 0;
    for (int p = 0; p < n; ++p) r += sigma[p] > cut ? 1 : 0;
    return r;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// local estimators on an inlier set; `pts` is [.][4] (x1 y1 x2 y2), `idx` the inliers in match order
// ---------------------------------------------------------------------------------------------------------------------

// CenterAndNormalizeImagePoints (geometry/normalization.cc:92-123); T = [f 0 -f cx; 0 f -f cy; 0 0 1] as (f, tx, ty)
inline void center_and_normalize(const double* pts, const std::vector<uint32_t>& idx, int side, std::vector<double>* out,
                                 double T[3]) {
  const size_t n = idx.size();
  double cx = 0.0, cy = 0.0;
  for (uint32_t i : idx) {
    cx += pts[4 * (size_t)i + 2 * side];
    cy += pts[4 * (size_t)i + 2 * side + 1];
  }
  cx /= (double)n;
  cy /= (double)n;
  double rms = 0.0;
  for (uint32_t i : idx) {
    const double dx = pts[4 * (size_t)i + 2 * side] - cx, dy = pts[4 * (size_t)i + 2 * side + 1] - cy;
    rms += dx * dx + dy * dy;
  }
  rms = std::sqrt(rms / (double)n);
  const double f = std::sqrt(2.0) / rms;
  T[0] = f;
  T[1] = -f * cx;
  T[2] = -f * cy;
  out->resize(2 * n);
  for (size_t k = 0; k < n; ++k) {
    (*out)[2 * k] = f * pts[4 * (size_t)idx[k] + 2 * side] + T[1];
    (*out)[2 * k + 1] = f * pts[4 * (size_t)idx[k] + 2 * side + 1] + T[2];
  }
}

// FundamentalMatrixEightPointEstimator::Estimate (fundamental_matrix.cc:124-176). The reference takes the null vector of
// exactly 8 points from a Householder QR of A^T and of more from a Jacobi SVD; here both come from the one SVD.
inline bool estimate_f8(const double* pts, const std::vector<uint32_t>& idx, Model* F) {
  const size_t n = idx.size();
  if (n < 8) return false;
  std::vector<double> p1, p2;
  double T1[3], T2[3];
  center_and_normalize(pts, idx, 0, &p1, T1);
  center_and_normalize(pts, idx, 1, &p2, T2);
  JacobiSvd svd;
  svd.n = 9;
  svd.a.assign(9, std::vector<double>(n));
  for (size_t k = 0; k < n; ++k) {
    const double x1 = p1[2 * k], y1 = p1[2 * k + 1], x2 = p2[2 * k], y2 = p2[2 * k + 1];
    const double row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
    for (int c = 0; c < 9; ++c) svd.a[(size_t)c][k] = row[c];
  }
  svd.compute();
  const double* q = svd.v[svd.order[8]];  // row-major 3 x 3
  // rank 2: U diag(s0, s1, 0) V^T = sum over the two largest of (Q v_k) v_k^T
  JacobiSvd p;
  p.n = 3;
  p.a.assign(3, std::vector<double>(3));
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) p.a[(size_t)c][(size_t)r] = q[3 * r + c];
  p.compute();
  double Fn[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 2; ++k) {
    const int col = p.order[k];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Fn[3 * r + c] += p.a[(size_t)col][(size_t)r] * p.v[col][c];
  }
  // normed_from_orig2^T * F * normed_from_orig1
  double G[9];  // F * T1
  for (int r = 0; r < 3; ++r) {
    G[3 * r + 0] = Fn[3 * r + 0] * T1[0];
    G[3 * r + 1] = Fn[3 * r + 1] * T1[0];
    G[3 * r + 2] = Fn[3 * r + 0] * T1[1] + Fn[3 * r + 1] * T1[2] + Fn[3 * r + 2];
  }
  for (int c = 0; c < 3; ++c) {
    (*F)[(size_t)c] = T2[0] * G[c];
    (*F)[(size_t)(3 + c)] = T2[0] * G[3 + c];
    (*F)[(size_t)(6 + c)] = T2[1] * G[c] + T2[2] * G[3 + c] + G[6 + c];
  }
  return true;
}

// HomographyMatrixEstimator::Estimate for more than 4 points (homography_matrix.cc:56-95): the DLT system in pixel
// units, the rank < 8 reject and the |det| < 1e-8 reject. 4 inliers never reach it: LORANSAC refits only a support of
// more than the minimal sample.
inline bool estimate_h_dlt(const double* pts, const std::vector<uint32_t>& idx, Model* H) {
  const size_t n = idx.size();
  if (n < 4) return false;
  JacobiSvd svd;
  svd.n = 9;
  svd.a.assign(9, std::vector<double>(2 * n, 0.0));
  for (size_t k = 0; k < n; ++k) {
    const double* p = pts + 4 * (size_t)idx[k];
    const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const double r0[9] = {x1, y1, 1.0, 0.0, 0.0, 0.0, -x2 * x1, -x2 * y1, -x2};
    const double r1[9] = {0.0, 0.0, 0.0, x1, y1, 1.0, -y2 * x1, -y2 * y1, -y2};
    for (int c = 0; c < 9; ++c) {
      svd.a[(size_t)c][2 * k] = r0[c];
      svd.a[(size_t)c][2 * k + 1] = r1[c];
    }
  }
  svd.compute();
  if (svd.rank(2 * n) < 8) return false;
  const double* h = svd.v[svd.order[8]];
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  if (std::fabs(det) < 1e-8) return false;
  for (int k = 0; k < 9; ++k) (*H)[(size_t)k] = h[k];
  return true;
}

// TranslationTransformEstimator<2>::Estimate (translation_transform.h:79-102): mean of dst minus mean of src
inline bool estimate_t_mean(const double* pts, const std::vector<uint32_t>& idx, Model* T) {
  if (idx.empty()) return false;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t i : idx)
    for (int c = 0; c < 4; ++c) s[c] += pts[4 * (size_t)i + c];
  for (int c = 0; c < 4; ++c) s[c] /= (double)idx.size();
  T->fill(0.0);
  (*T)[0] = s[2] - s[0];
  (*T)[1] = s[3] - s[1];
  return true;
}

inline bool local_estimate(int kind, const double* pts, const std::vector<uint32_t>& idx, Model* M) {
  return kind == tvs::KIND_F ? estimate_f8(pts, idx, M) : kind == tvs::KIND_H ? estimate_h_dlt(pts, idx, M) : estimate_t_mean(pts, idx, M);
}

// ---------------------------------------------------------------------------------------------------------------------
// the device, as the search sees it
// ---------------------------------------------------------------------------------------------------------------------

struct Item {  // trials [first_trial, first_trial + num_trials) of a set
  int32_t set;
  int64_t first_trial;
  int32_t num_trials;
};

struct RoundResult {  // over all trials of all items, in item order
  std::vector<int32_t> num_models;  // [trials]
  std::vector<double> models;       // [trials][3][9]
  std::vector<Support> supports;    // [trials][3]
};

struct ScoreJob {
  int32_t set;
  Model model;
};

struct Backend {
  virtual ~Backend() {}
  // a new batch of sets: points [.][4], set s = rows [offsets[s], offsets[s + 1])
  virtual void upload(const std::vector<int64_t>& offsets, const std::vector<double>& points,
                      const std::vector<uint64_t>& stream_ids) = 0;
  // hypothesize the items' trials and score every model they give
  virtual void round(int kind, double max_error, int32_t random_seed, const std::vector<Item>& items, RoundResult* out) = 0;
  // score the jobs' models; masks (nullable): one mask per job, as long as its set
  virtual void score(int kind, double max_error, const std::vector<ScoreJob>& jobs, std::vector<Support>* supports,
                     std::vector<std::vector<uint8_t>>* masks) = 0;
};

// ---------------------------------------------------------------------------------------------------------------------
// the search
// ---------------------------------------------------------------------------------------------------------------------

struct Report {
  bool success = false, has_model = false;
  uint64_t num_trials = 0;
  Support support;
  Model model{};
  std::vector<uint8_t> inlier_mask;
  uint64_t num_scored = 0, num_launches = 0;
};

struct Walk {
  enum Phase { WALKING, WAIT_SAMPLE_MASK, WAIT_REFIT };
  int32_t set = 0;
  const double* pts = nullptr;
  uint64_t n = 0;
  int kind = 0;
  uint64_t t = 0;  // the trial the walk stands at
  int j = 0;       // the model of that trial's sample
  uint64_t max_trials = 0, dyn_max = 0, min_trials = 0;
  double confidence = 0.0, multiplier = 0.0;
  bool done = false;
  Phase phase = WALKING;
  Support best, local_best;
  Model best_model{}, local_model{}, pending{};
  bool has_best = false;
  int local_trials = 0;
  std::vector<uint8_t> mask;  // of the residuals the next refit reads
  bool has_job = false;
  Report rep;

  void finish(uint64_t num_trials) {
    done = true;
    rep.num_trials = num_trials;
  }
  // loransac.h:322-341: the local optimum becomes the best, and the trial budget follows it
  void commit() {
    if (is_left_better(local_best, best)) {
      best = local_best;
      best_model = local_model;
      has_best = true;
      dyn_max = compute_num_trials(best.num_inliers, n, confidence, multiplier, tvs::min_samples(kind));
    }
  }
  // loransac.h:344-349, after every model of a sample; true: the search of this set has ended
  bool stop_check() {
    if (t >= dyn_max && t >= min_trials) {
      finish(t + 1);
      return true;
    }
    return false;
  }
  void request(const Model& m, Phase p) {
    pending = m;
    phase = p;
    has_job = true;
  }
  void end_local() {
    phase = WALKING;
    commit();
    if (!stop_check()) ++j;
  }
  void try_refit() {
    std::vector<uint32_t> idx;
    for (size_t i = 0; i < mask.size(); ++i)
      if (mask[i]) idx.push_back((uint32_t)i);
    Model m;
    if (local_estimate(kind, pts, idx, &m))
      request(m, WAIT_REFIT);
    else
      end_local();  // no local model: improved_support stays false (loransac.h:311-313)
  }
  // the answer to the pending request
  void deliver(const Support& s, std::vector<uint8_t>&& m) {
    has_job = false;
    if (phase == WAIT_SAMPLE_MASK) {
      mask = std::move(m);
      local_trials = 0;
      try_refit();
    } else {
      if (is_left_better(s, local_best)) {
        local_best = s;
        local_model = pending;
        mask = std::move(m);
        if (++local_trials < kMaxNumLocalTrials)
          try_refit();
        else
          end_local();
      } else {
        end_local();
      }
    }
  }
  // walks on through the trials [first, first + count) whose results start at `base` of R, until the set stops, the
  // round is used up or a request is pending
  void advance(const RoundResult& R, uint64_t first, uint64_t count, size_t base) {
    while (!done && !has_job) {
      if (t >= max_trials) {  // the reference's counter has been incremented once more when it leaves (loransac.h:218-223)
        finish(max_trials + 1);
        return;
      }
      if (t >= first + count) return;
      const size_t g = base + (size_t)(t - first);
      const int nm = R.num_models[g];
      while (j < nm) {
        const Support s = R.supports[tvs::kMaxModels * g + (size_t)j];
        if (is_left_better(s, best)) {
          local_best = s;
          for (int k = 0; k < 9; ++k) local_model[(size_t)k] = R.models[9 * (tvs::kMaxModels * g + (size_t)j) + (size_t)k];
          if (s.num_inliers > (uint64_t)tvs::min_samples(kind) && s.num_inliers >= (uint64_t)tvs::local_min_samples(kind)) {
            request(local_model, WAIT_SAMPLE_MASK);
            return;
          }
          commit();
        }
        if (stop_check()) return;
        ++j;
      }
      j = 0;
      ++t;
    }
  }
};

// LORANSAC of one kind over the sets of the uploaded batch. enabled (nullable): sets to search; the others get an
// empty report. ratios (nullable): min_inlier_ratio per set.
inline std::vector<Report> estimate(Backend& dev, int kind, const tvg_ransac_options& o, const std::vector<int64_t>& offsets,
                                    const std::vector<double>& points, const double* ratios, const uint8_t* enabled) {
  check_kind(kind);
  validate_ransac(o);
  const size_t S = offsets.size() - 1;
  const int T = o.trials_per_round > 0 ? o.trials_per_round : kDefaultTrialRound;
  std::vector<Walk> walks(S);
  for (size_t s = 0; s < S; ++s) {
    Walk& w = walks[s];
    w.set = (int32_t)s;
    w.pts = points.data() + 4 * (size_t)offsets[s];
    w.n = (uint64_t)(offsets[s + 1] - offsets[s]);
    w.kind = kind;
    const double ratio = ratios ? ratios[s] : o.min_inlier_ratio;
    TVG_CHECK(ratio >= 0.0 && ratio <= 1.0, "min_inlier_ratio of a set must lie in [0, 1]");
    w.max_trials = w.dyn_max = clamped_max_num_trials(o, ratio, tvs::min_samples(kind));
    w.min_trials = (uint64_t)o.min_num_trials;
    w.confidence = o.confidence;
    w.multiplier = o.dyn_num_trials_multiplier;
    if ((enabled && !enabled[s]) || w.n < (uint64_t)tvs::min_samples(kind)) w.done = true;  // loransac.h:142-144
  }
  std::vector<Item> items;
  std::vector<size_t> base;
  RoundResult R;
  std::vector<ScoreJob> jobs;
  std::vector<Walk*> owners;
  std::vector<Support> supports;
  std::vector<std::vector<uint8_t>> masks;
  for (;;) {
    items.clear();
    base.clear();
    size_t total = 0;
    for (Walk& w : walks) {
      if (w.done) continue;
      if (w.t >= w.max_trials) {
        w.finish(w.max_trials + 1);
        continue;
      }
      const uint64_t count = std::min<uint64_t>((uint64_t)T, w.max_trials - w.t);
      items.push_back({w.set, (int64_t)w.t, (int32_t)count});
      base.push_back(total);
      total += (size_t)count;
    }
    if (items.empty()) break;
    dev.round(kind, o.max_error, o.random_seed, items, &R);
    for (size_t i = 0; i < items.size(); ++i) {
      Walk& w = walks[(size_t)items[i].set];
      ++w.rep.num_launches;
      for (int32_t k = 0; k < items[i].num_trials; ++k) w.rep.num_scored += (uint64_t)R.num_models[base[i] + (size_t)k];
    }
    for (;;) {
      jobs.clear();
      owners.clear();
      for (size_t i = 0; i < items.size(); ++i) {
        Walk& w = walks[(size_t)items[i].set];
        if (!w.done && !w.has_job) w.advance(R, (uint64_t)items[i].first_trial, (uint64_t)items[i].num_trials, base[i]);
        if (!w.done && w.has_job) {
          jobs.push_back({w.set, w.pending});
          owners.push_back(&w);
        }
      }
      if (jobs.empty()) break;
      dev.score(kind, o.max_error, jobs, &supports, &masks);
      for (size_t k = 0; k < jobs.size(); ++k) {
        ++owners[k]->rep.num_scored;
        ++owners[k]->rep.num_launches;
        owners[k]->deliver(supports[k], std::move(masks[k]));
      }
    }
  }
  // the report and the winner's inlier mask (loransac.h:359-390)
  jobs.clear();
  owners.clear();
  for (Walk& w : walks) {
    w.rep.has_model = w.has_best;
    if (!w.has_best) continue;
    w.rep.support = w.best;
    w.rep.model = w.best_model;
    if (w.best.num_inliers < (uint64_t)tvs::min_samples(kind)) continue;
    w.rep.success = true;
    jobs.push_back({w.set, w.best_model});
    owners.push_back(&w);
  }
  if (!jobs.empty()) {
    dev.score(kind, o.max_error, jobs, &supports, &masks);
    for (size_t k = 0; k < jobs.size(); ++k) {
      ++owners[k]->rep.num_scored;
      ++owners[k]->rep.num_launches;
      owners[k]->rep.inlier_mask = std::move(masks[k]);
    }
  }
  std::vector<Report> out(S);
  for (size_t s = 0; s < S; ++s) out[s] = std::move(walks[s].rep);
  return out;
}

// ---------------------------------------------------------------------------------------------------------------------
// decisions: reports -> TwoViewGeometry
// ---------------------------------------------------------------------------------------------------------------------

struct Geometry {
  int config = TVG_CONFIG_UNDEFINED;
  bool has_F = false, has_H = false;
  Model F{}, H{};
  std::vector<uint8_t> inlier_mask;  // over the matches that were searched; empty: no inliers
  uint64_t num_inliers = 0;
};

// the min_inlier_ratio of the homography search (two_view_geometry.cc:283-287)
inline double homography_min_inlier_ratio(const tvg_options& o, uint64_t num_F_inliers, uint64_t num_matches) {
  return std::max(o.ransac.min_inlier_ratio, o.max_H_inlier_ratio * (double)num_F_inliers / (double)num_matches);
}

// EstimateUncalibratedTwoViewGeometry after its two searches (two_view_geometry.cc:292-320)
inline Geometry decide_uncalibrated(const Report& F, const Report& H, const tvg_options& o) {
  Geometry g;
  g.has_F = F.has_model;
  g.F = F.model;
  g.has_H = H.has_model;
  g.H = H.model;
  const uint64_t min_num_inliers = (uint64_t)o.min_num_inliers;
  if ((!F.success && !H.success) || (F.support.num_inliers < min_num_inliers && H.support.num_inliers < min_num_inliers)) {
    g.config = TVG_CONFIG_DEGENERATE;
    return g;
  }
  const double H_F_inlier_ratio = static_cast<double>(H.support.num_inliers) / (double)F.support.num_inliers;
  const std::vector<uint8_t>* best = &F.inlier_mask;
  g.num_inliers = F.support.num_inliers;
  if (H_F_inlier_ratio > o.max_H_inlier_ratio) {
    g.config = TVG_CONFIG_PLANAR_OR_PANORAMIC;
    if (H.support.num_inliers >= F.support.num_inliers) {
      g.num_inliers = H.support.num_inliers;
      best = &H.inlier_mask;
    }
  } else {
    g.config = TVG_CONFIG_UNCALIBRATED;
  }
  g.inlier_mask = *best;
  return g;
}

// EstimateCalibratedHomography after its search (two_view_geometry.cc:216-226)
inline Geometry decide_forced_homography(const Report& H, const tvg_options& o) {
  Geometry g;
  g.has_H = H.has_model;
  g.H = H.model;
  if (!H.success || H.support.num_inliers < (uint64_t)o.min_num_inliers) {
    g.config = TVG_CONFIG_DEGENERATE;
    return g;
  }
  g.config = TVG_CONFIG_PLANAR_OR_PANORAMIC;
  g.num_inliers = H.support.num_inliers;
  g.inlier_mask = H.inlier_mask;
  return g;
}

// DetectWatermarkMatches, the border test (two_view_geometry.cc:1514-1552): true when the translation search is due.
// pts: the searched matches [.][4]; mask: their inliers.
inline bool watermark_border_test(const tvg_camera& c1, const tvg_camera& c2, const double* pts, const std::vector<uint8_t>& mask,
                                  uint64_t num_inliers, const tvg_options& o) {
  if (num_inliers == 0) return false;  // the reference's ratios are NaN there and every test of them fails
  const double diagonal1 = std::sqrt((double)(c1.width * c1.width + c1.height * c1.height));
  const double diagonal2 = std::sqrt((double)(c2.width * c2.width + c2.height * c2.height));
  const double b1 = o.watermark_border_size * diagonal1, b2 = o.watermark_border_size * diagonal2;
  auto inside = [](double x, double y, double b, const tvg_camera& c) {  // AlignedBox2d::contains: closed
    return x >= b && y >= b && x <= (double)c.width - b && y <= (double)c.height - b;
  };
  uint64_t in_border = 0;
  for (size_t i = 0; i < mask.size(); ++i) {
    if (!mask[i]) continue;
    const double* p = pts + 4 * i;
    if (!inside(p[0], p[1], b1, c1) && !inside(p[2], p[3], b2, c2)) ++in_border;
  }
  const double ratio = static_cast<double>(in_border) / (double)num_inliers;
  return !(ratio < o.watermark_min_inlier_ratio);
}

// the RANSAC options of the watermark's translation search (:1556-1558)
inline tvg_ransac_options watermark_ransac_options(const tvg_options& o) {
  tvg_ransac_options r = o.ransac;
  r.max_error = o.watermark_detection_max_error;
  r.min_inlier_ratio = o.watermark_min_inlier_ratio;
  return r;
}

inline bool watermark_decision(const Report& T, uint64_t num_inliers, const tvg_options& o) {
  return static_cast<double>(T.support.num_inliers) / (double)num_inliers >= o.watermark_min_inlier_ratio;
}

// stream of iteration `it` of a pair under multiple_models; iteration 0 is the pair's own stream
inline uint64_t iteration_stream(uint64_t stream_id, int it) {
  return it == 0 ? stream_id : tvs::mix64(stream_id ^ tvs::mix64((uint64_t)it));
}

// ---------------------------------------------------------------------------------------------------------------------
// EstimateTwoViewGeometry for a batch of pairs (two_view_geometry.cc:552-640 with :339-382 and :1570-1584)
// ---------------------------------------------------------------------------------------------------------------------

struct PairResult {
  int route = 0;
  Geometry geometry;  // inlier_mask over ALL matches of the pair
};

struct VerifyStats {
  uint64_t num_scored = 0, num_launches = 0;
};

inline std::vector<PairResult> verify_pairs(Backend& dev, const tvg_options& o, int32_t num_pairs, const tvg_camera* cams1,
                                            const tvg_camera* cams2, const int64_t* match_offsets, const double* points,
                                            const uint64_t* stream_ids, VerifyStats* stats) {
  validate_options(o);
  validate_offsets(num_pairs, match_offsets, points, "pairs");
  TVG_CHECK(num_pairs == 0 || (cams1 && cams2 && stream_ids), "cameras or stream ids are null");
  const size_t P = (size_t)num_pairs;
  std::vector<PairResult> out(P);
  struct State {
    std::vector<uint32_t> remaining;  // matches still to be explained, as indices into the pair's matches
    std::vector<Geometry> found;      // under multiple_models
    bool active = false;
  };
  std::vector<State> st(P);
  for (size_t p = 0; p < P; ++p) {
    validate_camera(cams1[p], "camera 1 of pair " + std::to_string(p));
    validate_camera(cams2[p], "camera 2 of pair " + std::to_string(p));
    const size_t n = (size_t)(match_offsets[p + 1] - match_offsets[p]);
    out[p].route = route(cams1[p], cams2[p], o);
    out[p].geometry.inlier_mask.assign(n, 0);
    if (!route_is_built(out[p].route)) {
      out[p].geometry.config = TVG_CONFIG_NOT_BUILT;
      continue;
    }
    if (out[p].route == TVG_ROUTE_FORCED_H_DEGENERATE || out[p].route == TVG_ROUTE_FISHEYE_DEGENERATE) {
      out[p].geometry.config = TVG_CONFIG_DEGENERATE;
      continue;
    }
    const double* pts = points + 4 * (size_t)match_offsets[p];
    const double max2 = o.stationary_matches_max_error * o.stationary_matches_max_error;
    for (size_t i = 0; i < n; ++i) {
      if (o.filter_stationary_matches) {  // FilterStationaryMatches
        const double dx = pts[4 * i] - pts[4 * i + 2], dy = pts[4 * i + 1] - pts[4 * i + 3];
        if (dx * dx + dy * dy <= max2) continue;
      }
      st[p].remaining.push_back((uint32_t)i);
    }
    st[p].active = true;
  }

  std::vector<size_t> batch;  // pairs of this iteration's sets
  std::vector<int64_t> offsets;
  std::vector<double> pts;
  std::vector<uint64_t> streams;
  auto tally = [&](const std::vector<Report>& reports) {
    if (!stats) return;
    uint64_t launches = 0;
    for (const Report& r : reports) {
      stats->num_scored += r.num_scored;
      launches = std::max(launches, r.num_launches);
    }
    stats->num_launches += launches;  // the longest walk of a search took part in every launch of it
  };

  for (int it = 0;; ++it) {
    // this iteration's sets: the remaining matches of every active pair that has enough of them
    batch.clear();
    offsets.assign(1, 0);
    pts.clear();
    streams.clear();
    std::vector<Geometry> result(P);
    for (size_t p = 0; p < P; ++p) {
      if (!st[p].active) continue;
      if (st[p].remaining.size() < (size_t)o.min_num_inliers) {  // :190-193, :255-258
        result[p].config = TVG_CONFIG_DEGENERATE;
        continue;
      }
      const double* src = points + 4 * (size_t)match_offsets[p];
      for (uint32_t i : st[p].remaining) pts.insert(pts.end(), src + 4 * (size_t)i, src + 4 * (size_t)i + 4);
      offsets.push_back((int64_t)(pts.size() / 4));
      streams.push_back(iteration_stream(stream_ids[p], it));
      batch.push_back(p);
    }
    const size_t S = batch.size();
    if (S > 0) {
      dev.upload(offsets, pts, streams);
      std::vector<uint8_t> is_uncal(S);
      bool any_uncal = false;
      for (size_t s = 0; s < S; ++s) any_uncal |= (is_uncal[s] = out[batch[s]].route == TVG_ROUTE_UNCALIBRATED) != 0;
      std::vector<Report> F(S);
      if (any_uncal) {
        F = estimate(dev, tvs::KIND_F, o.ransac, offsets, pts, nullptr, is_uncal.data());
        tally(F);
      }
      std::vector<double> ratios(S);
      for (size_t s = 0; s < S; ++s)
        ratios[s] = is_uncal[s] ? homography_min_inlier_ratio(o, F[s].support.num_inliers, (uint64_t)(offsets[s + 1] - offsets[s]))
                                : o.ransac.min_inlier_ratio;
      std::vector<Report> H = estimate(dev, tvs::KIND_H, o.ransac, offsets, pts, ratios.data(), nullptr);
      tally(H);
      for (size_t s = 0; s < S; ++s)
        result[batch[s]] = is_uncal[s] ? decide_uncalibrated(F[s], H[s], o) : decide_forced_homography(H[s], o);

      // the watermark test: a translation search on the inlier points of the pairs that pass the border test
      if (o.detect_watermark) {
        std::vector<size_t> wm;
        std::vector<int64_t> w_offsets(1, 0);
        std::vector<double> w_pts;
        std::vector<uint64_t> w_streams;
        for (size_t s = 0; s < S; ++s) {
          const size_t p = batch[s];
          const Geometry& g = result[p];
          if (g.config == TVG_CONFIG_DEGENERATE) continue;
          const double* sp = pts.data() + 4 * (size_t)offsets[s];
          if (!watermark_border_test(cams1[p], cams2[p], sp, g.inlier_mask, g.num_inliers, o)) continue;
          for (size_t i = 0; i < g.inlier_mask.size(); ++i)
            if (g.inlier_mask[i]) w_pts.insert(w_pts.end(), sp + 4 * i, sp + 4 * i + 4);
          w_offsets.push_back((int64_t)(w_pts.size() / 4));
          w_streams.push_back(streams[s]);
          wm.push_back(p);
        }
        if (!wm.empty()) {
          dev.upload(w_offsets, w_pts, w_streams);
          const std::vector<Report> T = estimate(dev, tvs::KIND_T, watermark_ransac_options(o), w_offsets, w_pts, nullptr, nullptr);
          tally(T);
          for (size_t k = 0; k < wm.size(); ++k)
            if (watermark_decision(T[k], result[wm[k]].num_inliers, o)) result[wm[k]].config = TVG_CONFIG_WATERMARK;
        }
      }
    }

    // what the iteration means for every active pair
    bool again = false;
    for (size_t p = 0; p < P; ++p) {
      if (!st[p].active) continue;
      Geometry& g = result[p];
      // the mask over the pair's matches
      std::vector<uint8_t> full(out[p].geometry.inlier_mask.size(), 0);
      std::vector<uint32_t> rest;
      for (size_t k = 0; k < st[p].remaining.size(); ++k) {
        if (!g.inlier_mask.empty() && g.inlier_mask[k])
          full[st[p].remaining[k]] = 1;
        else
          rest.push_back(st[p].remaining[k]);
      }
      g.inlier_mask = std::move(full);
      if (!o.multiple_models) {
        out[p].geometry = std::move(g);
        st[p].active = false;
        continue;
      }
      // EstimateMultipleTwoViewGeometries (:349-381)
      if (g.config != TVG_CONFIG_DEGENERATE) {
        st[p].remaining = std::move(rest);
        if (!(o.multiple_ignore_watermark && g.config == TVG_CONFIG_WATERMARK)) st[p].found.push_back(std::move(g));
        again = true;
        continue;
      }
      st[p].active = false;
      std::vector<Geometry>& found = st[p].found;
      if (found.empty()) {
        out[p].geometry.config = TVG_CONFIG_DEGENERATE;
      } else if (found.size() == 1) {
        out[p].geometry = std::move(found[0]);
      } else {
        Geometry& m = out[p].geometry;
        m.config = TVG_CONFIG_MULTIPLE;  // only the inlier matches are set (two_view_geometry.h:115-116)
        for (const Geometry& f : found) {
          m.num_inliers += f.num_inliers;
          for (size_t i = 0; i < m.inlier_mask.size(); ++i) m.inlier_mask[i] |= f.inlier_mask[i];
        }
      }
    }
    if (!again) break;
  }
  return out;
}

}  // namespace two_view_plan

#endif  // COLMAP_AMD_TWO_VIEW_PLAN_H_
