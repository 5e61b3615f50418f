// obs_plan.h -- everything observation filtering decides on the host: the checks on the caller's model, the order in
// which the per-observation pass visits the observations, the lane-group class of every point, and the reduction of the
// per-point counts. Plain C++17: no HIP runtime -- obs_filter.hip builds the plan, uploads it and launches with it;
// tests/cpp/test_obs_plan.cc checks it against brute-force code without a GPU.
#ifndef COLMAP_AMD_OBS_PLAN_H_
#define COLMAP_AMD_OBS_PLAN_H_

#include "../../include/colmap_amd/camera_models.hpp"
#include "../../include/colmap_amd_obs.h"

#include <algorithm>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace obs_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define OBS_CHECK(cond, msg)                                                    \
  do {                                                                          \
    if (!(cond)) throw ::obs_plan::Fail(std::string("Check failed: ") + (msg)); \
  } while (0)

using colmap_amd::camera_models::kNumModels;

// Lane groups of the per-point pass: a point whose track has up to kSerialMax observations is one lane's work (at most
// 120 pairs, and the pair loop stops at the first good one); up to kRowMax it gets a row of 16 lanes; a longer track
// gets the whole wave.
constexpr int kNumClasses = 3;
constexpr int kClassWidth[kNumClasses] = {1, 16, 64};
constexpr int64_t kSerialMax = 16, kRowMax = 64;
inline int length_class(int64_t track_length) { return track_length <= kSerialMax ? 0 : track_length <= kRowMax ? 1 : 2; }

// Every check happens before anything is read THROUGH the array it guards: the counts and pointers first, then the
// offsets (which index the observation arrays), then the indices the observations and images hold (which index the
// image and camera arrays), then the cameras.
inline void validate(const obs_model& m) {
  OBS_CHECK(m.num_cameras >= 0 && m.num_images >= 0 && m.num_points >= 0 && m.num_observations >= 0,
            "model counts must not be negative");
  // observations and points are addressed with 32-bit indices on the device
  OBS_CHECK(m.num_points < std::numeric_limits<int32_t>::max(), "num_points must fit a 32-bit index");
  OBS_CHECK(m.num_observations < std::numeric_limits<int32_t>::max(), "num_observations must fit a 32-bit index");
  OBS_CHECK(m.obs_offsets != nullptr, "obs_offsets is null (it has num_points + 1 entries)");
  OBS_CHECK(m.num_cameras == 0 || m.cameras, "cameras is null");
  OBS_CHECK(m.num_images == 0 || (m.image_poses && m.image_camera), "image arrays are null");
  OBS_CHECK(m.num_points == 0 || m.points, "points is null");
  OBS_CHECK(m.num_observations == 0 || (m.obs_image && m.obs_xy), "observation arrays are null");
  OBS_CHECK(m.obs_offsets[0] == 0, "obs_offsets must start at 0");
  for (int64_t p = 0; p < m.num_points; ++p)
    OBS_CHECK(m.obs_offsets[p + 1] >= m.obs_offsets[p], "obs_offsets decreases at point " + std::to_string(p));
  OBS_CHECK(m.obs_offsets[m.num_points] == m.num_observations, "obs_offsets must end at num_observations");
  for (int64_t o = 0; o < m.num_observations; ++o)
    OBS_CHECK(m.obs_image[o] >= 0 && m.obs_image[o] < m.num_images,
              "observation " + std::to_string(o) + ": image index " + std::to_string(m.obs_image[o]) + " out of range");
  for (int32_t i = 0; i < m.num_images; ++i)
    OBS_CHECK(m.image_camera[i] >= 0 && m.image_camera[i] < m.num_cameras,
              "image " + std::to_string(i) + ": camera index " + std::to_string(m.image_camera[i]) + " out of range");
  for (int32_t c = 0; c < m.num_cameras; ++c) {
    const int n = colmap_amd::camera_models::num_params(m.cameras[c].model_id);
    OBS_CHECK(n > 0, "camera " + std::to_string(c) + ": unknown camera model id " + std::to_string(m.cameras[c].model_id));
    OBS_CHECK(m.cameras[c].num_params == n, "camera " + std::to_string(c) + ": model " + std::to_string(m.cameras[c].model_id) +
                                                " takes " + std::to_string(n) + " parameters, got " +
                                                std::to_string(m.cameras[c].num_params));
    OBS_CHECK(m.cameras[c].width > 0 && m.cameras[c].height > 0,
              "camera " + std::to_string(c) + ": width and height must be positive");
  }
}

struct Plan {
  std::vector<int32_t> obs_point;                  // [num_observations] the point of an observation
  std::vector<int32_t> eval_order;                 // [num_observations] the per-observation pass: lane t takes
                                                   // observation eval_order[t]; sorted by camera model id (stable), so
                                                   // that a wave takes one branch of the model switch
  std::vector<int32_t> class_points[kNumClasses];  // the points of each lane-group class, ascending
};

// of a validated model
inline Plan make_plan(const obs_model& m, bool want_eval_order) {
  Plan plan;
  plan.obs_point.resize((size_t)m.num_observations);
  for (int64_t p = 0; p < m.num_points; ++p) {
    for (int64_t o = m.obs_offsets[p]; o < m.obs_offsets[p + 1]; ++o) plan.obs_point[(size_t)o] = (int32_t)p;
    plan.class_points[length_class(m.obs_offsets[p + 1] - m.obs_offsets[p])].push_back((int32_t)p);
  }
  if (want_eval_order) {  // counting sort by model id
    int64_t start[kNumModels + 1] = {0};
    for (int64_t o = 0; o < m.num_observations; ++o) ++start[m.cameras[m.image_camera[m.obs_image[o]]].model_id + 1];
    for (int k = 0; k < kNumModels; ++k) start[k + 1] += start[k];
    plan.eval_order.resize((size_t)m.num_observations);
    for (int64_t o = 0; o < m.num_observations; ++o)
      plan.eval_order[(size_t)start[m.cameras[m.image_camera[m.obs_image[o]]].model_id]++] = (int32_t)o;
  }
  return plan;
}

// The filtered-observation count of a call: the per-point counts added in point order, in integers -- the same input
// gives the same number on every run.
inline int64_t sum_counts(const uint32_t* point_count, int64_t num_points) {
  int64_t sum = 0;
  for (int64_t p = 0; p < num_points; ++p) sum += (int64_t)point_count[p];
  return sum;
}

}  // namespace obs_plan
#endif  // COLMAP_AMD_OBS_PLAN_H_
