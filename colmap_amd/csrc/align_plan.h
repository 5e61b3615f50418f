// align_plan.h -- everything model alignment decides on the host: the checks on the caller's arrays, the layout the
// reprojection scorer reads (records sorted by image, every image's segment padded to whole waves), Sim3 <-> 3x4 maps,
// the deterministic sample stream, RANSAC's stopping rule and the LORANSAC search loop itself. Plain C++17: no HIP
// runtime -- model_align.hip builds the plan, uploads it and hands the loop a scorer that launches;
// tests/cpp/test_align_plan.cc drives the same loop with a scripted scorer without a GPU.
//
// The loop is optim/loransac.h:131-393 of the reference with InlierSupportMeasurer (optim/support_measurement.cc:36-61):
// one hypothesis per trial from a minimal sample of 3, support = (inlier count, then residual sum), up to 10 local refits
// on the inlier set of the last residuals that stop at the first refit that does not improve, ComputeNumTrials
// (optim/ransac.h:179-210) with the constructor's clamp (:167-175), and the inlier mask recomputed for the winner.
// What differs is HOW the trials are scored, not what is decided: the loop draws the next B samples, estimates their
// models on the host (Horn's closed form, AlignToPositions) and has them scored in ONE call; then it walks the results
// in trial order under exactly the sequential rules and throws away what lies past the stopping trial. The scores of a
// hypothesis do not depend on its batch (model_align.hip), the refits do not touch the sample stream, so the report is
// the same for every B.
//
// Samples come from the 64-bit LCG of colmap_amd/estimators.py (_lcg) with rejection of repeats. The reference's
// RandomSampler shuffles with std::mt19937 through std::uniform_int_distribution, whose stream is implementation-defined;
// it is not reproduced.
#ifndef COLMAP_AMD_ALIGN_PLAN_H_
#define COLMAP_AMD_ALIGN_PLAN_H_

#include "../../include/colmap_amd/bundle_adjustment.hpp"  // AlignToPositions (Horn), QuatToRot, RotToQuat
#include "../../include/colmap_amd/camera_models.hpp"
#include "../../include/colmap_amd_align.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace align_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define ALIGN_CHECK(cond, msg)                                                    \
  do {                                                                            \
    if (!(cond)) throw ::align_plan::Fail(std::string("Check failed: ") + (msg)); \
  } while (0)

constexpr int kWave = 64;
constexpr int kMinNumSamples = 3;       // ReconstructionAlignmentEstimator / SimilarityTransformEstimator<3>
constexpr int kMaxNumLocalTrials = 10;  // loransac.h:261
constexpr int kDefaultBatch = 16;       // one hypothesis tile; chosen by the measurement of DESIGN 2.4d

// ---------------------------------------------------------------------------------------------------------------------
// Sim3: 8 doubles in the order of Sim3d::ToFile (geometry/sim3.cc:39-48): scale, qw qx qy qz, tx ty tz
// ---------------------------------------------------------------------------------------------------------------------

inline void sim3_rotation(const double sim[8], double R[9]) {
  const double n = std::sqrt(sim[1] * sim[1] + sim[2] * sim[2] + sim[3] * sim[3] + sim[4] * sim[4]);
  const double q[4] = {sim[2] / n, sim[3] / n, sim[4] / n, sim[1] / n};  // xyzw
  colmap_amd::QuatToRot(q, R);
}

// b_from_a as the 3x4 map [sR | t], row-major: the operator* of geometry/sim3.h:120-123 applies s * (R x) + t; the
// scorer applies the rows of this matrix.
inline void sim3_matrix(const double sim[8], double M[12]) {
  double R[9];
  sim3_rotation(sim, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M[4 * r + c] = sim[0] * R[3 * r + c];
    M[4 * r + 3] = sim[5 + r];
  }
}

// Inverse(Sim3d) (geometry/sim3.h:98-105): scale 1 / s, rotation R^T, translation (R^T t) / -s
inline void sim3_inverse(const double sim[8], double inv[8]) {
  double R[9];
  sim3_rotation(sim, R);
  const double n = std::sqrt(sim[1] * sim[1] + sim[2] * sim[2] + sim[3] * sim[3] + sim[4] * sim[4]);
  inv[0] = 1.0 / sim[0];
  inv[1] = sim[1] / n;
  inv[2] = -sim[2] / n;
  inv[3] = -sim[3] / n;
  inv[4] = -sim[4] / n;
  for (int r = 0; r < 3; ++r)
    inv[5 + r] = (R[r] * sim[5] + R[3 + r] * sim[6] + R[6 + r] * sim[7]) / -sim[0];
}

inline void sim3_from_srt(double scale, const double R[9], const double t[3], double sim[8]) {
  double q[4];
  colmap_amd::RotToQuat(R, q);  // xyzw
  sim[0] = scale;
  sim[1] = q[3];
  sim[2] = q[0];
  sim[3] = q[1];
  sim[4] = q[2];
  sim[5] = t[0];
  sim[6] = t[1];
  sim[7] = t[2];
}

inline void check_sim3(const double sim[8], const std::string& what) {
  bool finite = true;
  for (int k = 0; k < 8; ++k) finite = finite && std::isfinite(sim[k]);
  ALIGN_CHECK(finite, what + " is not finite");
  ALIGN_CHECK(sim[0] != 0.0, what + " has scale 0");
  ALIGN_CHECK(sim[1] * sim[1] + sim[2] * sim[2] + sim[3] * sim[3] + sim[4] * sim[4] > 0.0, what + " has a zero quaternion");
}

// Image::ProjectionCenter: -R^T t of cam_from_world (qx qy qz qw tx ty tz)
inline std::array<double, 3> projection_center(const double pose[7]) {
  double R[9];
  colmap_amd::QuatToRot(pose, R);
  return {-(R[0] * pose[4] + R[3] * pose[5] + R[6] * pose[6]), -(R[1] * pose[4] + R[4] * pose[5] + R[7] * pose[6]),
          -(R[2] * pose[4] + R[5] * pose[5] + R[8] * pose[6])};
}

// ---------------------------------------------------------------------------------------------------------------------
// checks; every check happens before anything is read through the array it guards
// ---------------------------------------------------------------------------------------------------------------------

inline void validate_camera(const align_camera& c, const std::string& what) {
  const int n = colmap_amd::camera_models::num_params(c.model_id);
  ALIGN_CHECK(n > 0, what + ": unknown camera model id " + std::to_string(c.model_id));
  ALIGN_CHECK(c.num_params == n, what + ": model " + std::to_string(c.model_id) + " takes " + std::to_string(n) +
                                     " parameters, got " + std::to_string(c.num_params));
  ALIGN_CHECK(c.width > 0 && c.height > 0, what + ": width and height must be positive");
}

inline void validate(const align_reproj_pair& p) {
  ALIGN_CHECK(p.num_images >= 0 && p.num_records >= 0, "counts must not be negative");
  ALIGN_CHECK(p.num_records < std::numeric_limits<int32_t>::max() - 64 * (int64_t)p.num_images - 64,
              "the padded records must fit a 32-bit index");
  ALIGN_CHECK(p.num_images == 0 || (p.src_cameras && p.tgt_cameras && p.src_poses && p.tgt_poses && p.src_num_points2D &&
                                    p.tgt_num_points2D),
              "image arrays are null (each has num_images entries)");
  ALIGN_CHECK(p.num_records == 0 || (p.rec_image && p.rec_src_xyz && p.rec_tgt_xyz && p.rec_src_xy && p.rec_tgt_xy),
              "record arrays are null (each has num_records entries)");
  for (int32_t i = 0; i < p.num_images; ++i) {
    // THROW_CHECK_EQ(src_image.NumPoints2D(), tgt_image.NumPoints2D()), alignment.cc:120
    ALIGN_CHECK(p.src_num_points2D[i] == p.tgt_num_points2D[i],
                "image " + std::to_string(i) + ": NumPoints2D differs between the models (" +
                    std::to_string(p.src_num_points2D[i]) + " and " + std::to_string(p.tgt_num_points2D[i]) + ")");
    validate_camera(p.src_cameras[i], "image " + std::to_string(i) + ", src camera");
    validate_camera(p.tgt_cameras[i], "image " + std::to_string(i) + ", tgt camera");
  }
  for (int64_t r = 0; r < p.num_records; ++r)
    ALIGN_CHECK(p.rec_image[r] >= 0 && p.rec_image[r] < p.num_images,
                "record " + std::to_string(r) + ": image slot " + std::to_string(p.rec_image[r]) + " out of range");
}

inline void validate_positions(const double* src, const double* tgt, int64_t n) {
  ALIGN_CHECK(n >= 0, "the number of points must not be negative");
  ALIGN_CHECK(n < std::numeric_limits<int32_t>::max() - 4096, "the number of points must fit a 32-bit index");
  ALIGN_CHECK(n == 0 || (src && tgt), "point arrays are null (each has 3 * num_points entries)");
}

inline void validate_options(const align_options& o, bool reprojection) {
  ALIGN_CHECK(o.max_error >= 0.0, "max_error must not be negative");  // THROW_CHECK_GE(max_reproj_error, 0)
  if (reprojection)
    ALIGN_CHECK(o.min_inlier_observations >= 0.0 && o.min_inlier_observations <= 1.0,
                "min_inlier_observations must lie in [0, 1]");
  else
    ALIGN_CHECK(o.max_error > 0.0, "max_error must be positive");  // RANSACOptions::Check
  ALIGN_CHECK(o.min_inlier_ratio >= 0.0 && o.min_inlier_ratio <= 1.0, "min_inlier_ratio must lie in [0, 1]");
  ALIGN_CHECK(o.confidence >= 0.0 && o.confidence <= 1.0, "confidence must lie in [0, 1]");
  ALIGN_CHECK(o.min_num_trials >= 0 && o.min_num_trials <= o.max_num_trials, "min_num_trials must lie in [0, max_num_trials]");
  ALIGN_CHECK(o.random_seed >= 0, "random_seed must not be negative (the sample stream is deterministic)");
  ALIGN_CHECK(o.batch_size >= 0 && o.batch_size <= ALIGN_MAX_BATCH, "batch_size must lie in [0, ALIGN_MAX_BATCH] (0 = default)");
}

// ---------------------------------------------------------------------------------------------------------------------
// layout of the reprojection scorer
// ---------------------------------------------------------------------------------------------------------------------

// Records sorted by image slot (stable: within an image they keep the caller's order) and every image's segment padded
// to whole waves of 64, so that a wave holds records of ONE image: its poses and cameras are wave-uniform and it takes
// one branch of each camera-model switch. Row r of the padded arrays holds record order[r], or nothing (order[r] = -1,
// beyond wave_count of its wave). Structure of arrays: component c of row r is at [c * num_rows + r].
struct ReprojLayout {
  int64_t num_rows = 0;                  // 64 * number of waves
  std::vector<int32_t> order;            // [num_rows] caller's record index, -1 for padding
  std::vector<int32_t> wave_image;       // [num_waves] image slot of the wave
  std::vector<int32_t> wave_count;       // [num_waves] valid lanes of the wave, 1..64
  std::vector<int32_t> image_wave_begin; // [num_images + 1] waves of image i: image_wave_begin[i] .. [i + 1] - 1
  std::vector<uint32_t> common;          // [num_images] records of the image: num_common_points of alignment.cc:123
};

// of a validated pair
inline ReprojLayout make_layout(const align_reproj_pair& p) {
  ReprojLayout L;
  const size_t I = (size_t)p.num_images;
  L.common.assign(I, 0u);
  for (int64_t r = 0; r < p.num_records; ++r) ++L.common[(size_t)p.rec_image[r]];
  L.image_wave_begin.assign(I + 1, 0);
  for (size_t i = 0; i < I; ++i) L.image_wave_begin[i + 1] = L.image_wave_begin[i] + (int32_t)((L.common[i] + kWave - 1) / kWave);
  const size_t W = (size_t)L.image_wave_begin[I];
  L.num_rows = (int64_t)W * kWave;
  L.order.assign((size_t)L.num_rows, -1);
  L.wave_image.resize(W);
  L.wave_count.resize(W);
  std::vector<int64_t> next(I);
  for (size_t i = 0; i < I; ++i) {
    next[i] = (int64_t)L.image_wave_begin[i] * kWave;
    for (int32_t w = L.image_wave_begin[i]; w < L.image_wave_begin[i + 1]; ++w) {
      L.wave_image[(size_t)w] = (int32_t)i;
      const int64_t left = (int64_t)L.common[i] - (int64_t)(w - L.image_wave_begin[i]) * kWave;
      L.wave_count[(size_t)w] = (int32_t)std::min<int64_t>(left, kWave);
    }
  }
  for (int64_t r = 0; r < p.num_records; ++r) L.order[(size_t)next[(size_t)p.rec_image[r]]++] = (int32_t)r;
  return L;
}

// The residual of ReconstructionAlignmentEstimator::Residuals (alignment.cc:166-173) from the integer counts.
inline double reproj_residual(uint32_t inliers, uint32_t common) {
  if (common == 0) return 1.0;
  const double negative_inlier_ratio = 1.0 - (double)inliers / (double)common;
  return negative_inlier_ratio * negative_inlier_ratio;
}

// ---------------------------------------------------------------------------------------------------------------------
// the search
// ---------------------------------------------------------------------------------------------------------------------

constexpr uint64_t kNoLimit = std::numeric_limits<uint64_t>::max();  // the reference's size_t max

// RANSAC::ComputeNumTrials (optim/ransac.h:179-210) for kMinNumSamples = 3. num_inliers - i is unsigned in the reference
// and wraps below 3 inliers; a factor 0 is always among the three then, so the product is 0 either way.
inline uint64_t ComputeNumTrials(uint64_t num_inliers, uint64_t num_samples, double confidence, double num_trials_multiplier) {
  const double prob_failure = 1 - confidence;
  if (prob_failure <= 0) return kNoLimit;
  double prob_inlier = 1.0;
  for (int i = 0; i < kMinNumSamples; ++i)
    prob_inlier *= static_cast<double>(num_inliers - (uint64_t)i) / static_cast<double>(num_samples - (uint64_t)i);
  const double prob_outlier = 1 - prob_inlier;
  if (prob_outlier <= 0) return 1;
  if (prob_outlier == 1.0) return kNoLimit;
  const double trials = std::ceil(std::log(prob_failure) / std::log(prob_outlier) * num_trials_multiplier);
  if (!(trials < 18446744073709551615.0)) return kNoLimit;
  return trials > 0.0 ? static_cast<uint64_t>(trials) : 0;
}

// the clamp of the RANSAC constructor (optim/ransac.h:167-175)
inline uint64_t clamped_max_num_trials(const align_options& o) {
  const uint64_t kNumSamples = 100000;
  const uint64_t dyn = ComputeNumTrials(static_cast<uint64_t>(o.min_inlier_ratio * kNumSamples), kNumSamples, o.confidence,
                                        o.dyn_num_trials_multiplier);
  return std::min<uint64_t>((uint64_t)o.max_num_trials, dyn);
}

struct SampleStream {
  uint64_t state;
  explicit SampleStream(int32_t seed) : state(lcg(0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)seed)) {}
  static uint64_t lcg(uint64_t s) { return s * 6364136223846793005ull + 1442695040888963407ull; }
  // three different indices below n (n >= 3)
  void draw(size_t n, size_t idx[kMinNumSamples]) {
    for (int k = 0; k < kMinNumSamples;) {
      state = lcg(state);
      const size_t c = (size_t)((state >> 33) % n);
      bool dup = false;
      for (int j = 0; j < k; ++j) dup = dup || idx[j] == c;
      if (!dup) idx[k++] = c;
    }
  }
};

struct Support {  // InlierSupportMeasurer::Support
  uint64_t num_inliers = 0;
  double residual_sum = std::numeric_limits<double>::max();
};

inline bool IsLeftBetter(const Support& left, const Support& right) {
  if (left.num_inliers > right.num_inliers) return true;
  return left.num_inliers == right.num_inliers && left.residual_sum < right.residual_sum;
}

struct Report {
  bool success = false;
  uint64_t num_trials = 0;
  Support support;
  std::array<double, 8> model{{1, 1, 0, 0, 0, 0, 0, 0}};
  std::vector<uint8_t> inlier_mask;
  uint64_t num_scored = 0;   // hypotheses handed to the scorer (those past the stopping trial included)
  uint64_t num_launches = 0;
};

// Horn's closed form on the given samples of two point sets; false where it has no answer (collinear, coincident).
inline bool estimate_sim3(const double* src, const double* tgt, const size_t* idx, size_t n, double sim[8]) {
  std::vector<std::array<double, 3>> a(n), b(n);
  for (size_t k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c) {
      a[k][c] = src[3 * idx[k] + c];
      b[k][c] = tgt[3 * idx[k] + c];
    }
  double scale, R[9], t[3];
  if (!colmap_amd::AlignToPositions(a, b, &scale, R, t)) return false;
  if (!(std::isfinite(scale) && scale > 0.0)) return false;
  sim3_from_srt(scale, R, t, sim);
  for (int k = 0; k < 8; ++k)
    if (!std::isfinite(sim[k])) return false;
  return true;
}

// Problem:
//   size_t num_samples() const;
//   bool estimate(const size_t* idx, size_t n, double sim[8]);      the model of the samples idx[0..n-1]
//   void score(const double* sims, int B, Support* supports);       Evaluate(residuals, max_residual) of B models, one call
//   void inliers(const double sim[8], std::vector<uint8_t>* mask, Support* s);   one model: residual <= max_residual
//                                                                   of every sample too
// The problem owns max_residual. score and inliers agree on a model's support whatever the batch it is scored in.
template <typename Problem>
Report loransac(Problem& problem, const align_options& opt) {
  Report report;
  const size_t num_samples = problem.num_samples();
  if (num_samples < (size_t)kMinNumSamples) return report;
  const uint64_t min_num_trials = (uint64_t)opt.min_num_trials;
  const uint64_t max_num_trials = clamped_max_num_trials(opt);
  const uint64_t batch = (uint64_t)(opt.batch_size > 0 ? opt.batch_size : kDefaultBatch);

  Support best_support;
  best_support.num_inliers = 0;
  bool have_best = false;
  std::array<double, 8> best_model{};
  SampleStream stream(opt.random_seed);
  uint64_t trial_counter = 0, dyn_max_num_trials = max_num_trials;
  bool abort = false;

  std::vector<double> sims;
  std::vector<uint8_t> mask, local_mask;
  std::vector<int> slot;  // of a trial of the batch: its row in sims, -1 where the sample has no model
  std::vector<Support> supports;
  std::vector<size_t> inlier_idx;

  while (!abort) {
    if (trial_counter >= max_num_trials) {  // the fetch_add that finds the limit still counts (loransac.h:216-221, 358)
      ++trial_counter;
      break;
    }
    // No trial at or past max(dyn_max_num_trials, min_num_trials) with a model survives its own stopping check; samples
    // without a model do not check, so the walk below decides, and this bound only saves work.
    uint64_t want = std::min<uint64_t>(batch, max_num_trials - trial_counter);
    const uint64_t stop_at = std::max(dyn_max_num_trials, min_num_trials);
    if (stop_at != kNoLimit && stop_at + 1 > trial_counter) want = std::min<uint64_t>(want, stop_at + 1 - trial_counter);
    if (stop_at <= trial_counter) want = 1;
    sims.clear();
    slot.assign((size_t)want, -1);
    for (uint64_t k = 0; k < want; ++k) {
      size_t idx[kMinNumSamples];
      stream.draw(num_samples, idx);
      double sim[8];
      if (problem.estimate(idx, kMinNumSamples, sim)) {
        slot[(size_t)k] = (int)(sims.size() / 8);
        sims.insert(sims.end(), sim, sim + 8);
      }
    }
    supports.assign(sims.size() / 8, Support());
    if (!sims.empty()) {
      problem.score(sims.data(), (int)(sims.size() / 8), supports.data());
      report.num_scored += sims.size() / 8;
      ++report.num_launches;
    }
    for (uint64_t k = 0; k < want; ++k) {
      const uint64_t curr_trial = trial_counter++;
      if (slot[(size_t)k] < 0) continue;  // no model: no stopping check either (it sits in the loop over the models)
      const double* sample_model = sims.data() + 8 * (size_t)slot[(size_t)k];
      const Support support = supports[(size_t)slot[(size_t)k]];
      if (IsLeftBetter(support, best_support)) {
        Support local_best_support = support;
        std::array<double, 8> local_best_model;
        std::copy(sample_model, sample_model + 8, local_best_model.begin());
        if (support.num_inliers > (uint64_t)kMinNumSamples) {
          Support again;
          problem.inliers(sample_model, &mask, &again);
          ++report.num_scored;
          ++report.num_launches;
          for (int local_num_trials = 0; local_num_trials < kMaxNumLocalTrials; ++local_num_trials) {
            inlier_idx.clear();
            for (size_t i = 0; i < mask.size(); ++i)
              if (mask[i]) inlier_idx.push_back(i);
            double local_model[8];
            bool improved_support = false;
            if (problem.estimate(inlier_idx.data(), inlier_idx.size(), local_model)) {
              Support local_support;
              problem.inliers(local_model, &local_mask, &local_support);
              ++report.num_scored;
              ++report.num_launches;
              if (IsLeftBetter(local_support, local_best_support)) {
                local_best_support = local_support;
                std::copy(local_model, local_model + 8, local_best_model.begin());
                improved_support = true;
                mask.swap(local_mask);
              }
            }
            if (!improved_support) break;
          }
        }
        if (IsLeftBetter(local_best_support, best_support)) {
          best_support = local_best_support;
          best_model = local_best_model;
          have_best = true;
          dyn_max_num_trials = ComputeNumTrials(best_support.num_inliers, num_samples, opt.confidence, opt.dyn_num_trials_multiplier);
        }
      }
      if (curr_trial >= dyn_max_num_trials && curr_trial >= min_num_trials) {
        abort = true;
        break;
      }
    }
  }

  report.num_trials = trial_counter;
  if (!have_best) return report;
  report.support = best_support;
  report.model = best_model;
  if (report.support.num_inliers < (uint64_t)kMinNumSamples) return report;
  report.success = true;
  Support final_support;
  problem.inliers(report.model.data(), &report.inlier_mask, &final_support);
  ++report.num_scored;
  ++report.num_launches;
  return report;
}

}  // namespace align_plan
#endif  // COLMAP_AMD_ALIGN_PLAN_H_
