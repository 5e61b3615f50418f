// model_plan.h -- everything the model statistics decide on the host: the checks on the caller's model, the
// observations bucketed by image for the depth pass, the lane-group class of every point for the pair passes, the
// number of track pairs, the selection class of every segment, the device memory a call needs and the limits beyond
// which a model is refused. Plain C++17: no HIP runtime -- model_stats.hip builds the plan, uploads it and launches
// with it; tests/cpp/test_model_plan.cc checks it against brute-force code without a GPU.
//
// Limits (a model beyond one is refused with a "Check failed: ..." message that names it; nothing overflows):
//   kMaxImages        8192    the pair table is dense: num_images (num_images - 1) / 2 cells, addressed with a 32-bit
//                             index (33.5 M cells, 20 bytes each), and a row of it is ranked in the LDS of one workgroup
//   num_points, num_observations < 2^31   addressed with 32-bit indices on the device
//   kMaxTrackPairs    2^40    sum over the points of L (L - 1) / 2, accumulated in 64 bits
//   kMaxCellPairs     2^31-1  a cell of the pair table is an int32: the sum over the points of floor(L/2) ceil(L/2), the
//                             most pairs one track can give to ONE image pair, must fit
//   device memory             device_bytes_* against what the device reports free, before anything is launched
#ifndef COLMAP_AMD_MODEL_PLAN_H_
#define COLMAP_AMD_MODEL_PLAN_H_

#include "../../include/colmap_amd_model.h"

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace model_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define MODEL_CHECK(cond, msg)                                                    \
  do {                                                                            \
    if (!(cond)) throw ::model_plan::Fail(std::string("Check failed: ") + (msg)); \
  } while (0)

constexpr int32_t kMaxImages = 8192;
constexpr int64_t kMaxTrackPairs = (int64_t)1 << 40;
constexpr int64_t kMaxCellPairs = std::numeric_limits<int32_t>::max();

// Lane groups of the pair passes, as in obs_plan.h: a track of up to kSerialMax observations is one lane's work, up to
// kRowMax it gets a row of 16 lanes, a longer one the whole wave.
constexpr int kNumClasses = 3;
constexpr int kClassWidth[kNumClasses] = {1, 16, 64};
constexpr int64_t kSerialMax = 16, kRowMax = 64;
inline int length_class(int64_t track_length) { return track_length <= kSerialMax ? 0 : track_length <= kRowMax ? 1 : 2; }

// Order-statistic selection: a segment of up to kSelectWaveMax values is ranked in registers by one wave (one value
// per lane), a longer one gets a workgroup and a radix select.
constexpr int64_t kSelectWaveMax = 64;
inline int select_class(int64_t segment_length) { return segment_length <= kSelectWaveMax ? 0 : 1; }

inline int64_t num_cells(int64_t num_images) { return num_images * (num_images - 1) / 2; }
// the cell of the image pair a < b in the upper-triangular table, row-major
inline int64_t cell_index(int64_t a, int64_t b, int64_t num_images) { return a * (2 * num_images - a - 1) / 2 + (b - a - 1); }

// Every check happens before anything is read THROUGH the array it guards: the counts and pointers first, then the
// offsets (which index track_image), then the image indices (which index R and T on the device).
inline void validate(const model_flat& m) {
  MODEL_CHECK(m.num_images >= 0 && m.num_points >= 0 && m.num_observations >= 0, "model counts must not be negative");
  MODEL_CHECK(m.num_images <= kMaxImages, "num_images " + std::to_string(m.num_images) + " exceeds the limit of the dense pair table, " +
                                              std::to_string(kMaxImages) + " images");
  MODEL_CHECK(m.num_points < std::numeric_limits<int32_t>::max(), "num_points must fit a 32-bit index");
  MODEL_CHECK(m.num_observations < std::numeric_limits<int32_t>::max(), "num_observations must fit a 32-bit index");
  MODEL_CHECK(m.track_offsets != nullptr, "track_offsets is null (it has num_points + 1 entries)");
  MODEL_CHECK(m.num_images == 0 || (m.R && m.T), "image arrays are null");
  MODEL_CHECK(m.num_points == 0 || m.points, "points is null");
  MODEL_CHECK(m.num_observations == 0 || m.track_image, "track_image is null");
  MODEL_CHECK(m.track_offsets[0] == 0, "track_offsets must start at 0");
  for (int64_t p = 0; p < m.num_points; ++p)
    MODEL_CHECK(m.track_offsets[p + 1] >= m.track_offsets[p], "track_offsets decreases at point " + std::to_string(p));
  MODEL_CHECK(m.track_offsets[m.num_points] == m.num_observations, "track_offsets must end at num_observations");
  for (int64_t o = 0; o < m.num_observations; ++o)
    MODEL_CHECK(m.track_image[o] >= 0 && m.track_image[o] < m.num_images,
                "observation " + std::to_string(o) + ": image index " + std::to_string(m.track_image[o]) + " out of range");
}

inline void validate_percentile(double p) {
  MODEL_CHECK(p >= 0.0 && p <= 100.0, "percentile must lie in [0, 100]");  // Percentile, math/math.h:207-208 (a NaN fails)
}

// ---- depth pass --------------------------------------------------------------------------------------------------------

struct DepthPlan {
  std::vector<int64_t> image_offsets;  // [num_images + 1] the segment of image i in by-image order
  std::vector<int32_t> obs_order;      // [num_observations] lane t takes observation obs_order[t]: bucketed by image
                                       // (counting sort, stable: observation order within an image)
  std::vector<int32_t> obs_point;      // [num_observations] the point of an observation
  std::vector<int32_t> select_ids[2];  // the images of each selection class, ascending
};

// of a validated model
inline DepthPlan make_depth_plan(const model_flat& m) {
  DepthPlan plan;
  const size_t I = (size_t)m.num_images, O = (size_t)m.num_observations;
  plan.image_offsets.assign(I + 1, 0);
  for (size_t o = 0; o < O; ++o) ++plan.image_offsets[(size_t)m.track_image[o] + 1];
  for (size_t i = 0; i < I; ++i) plan.image_offsets[i + 1] += plan.image_offsets[i];
  plan.obs_order.resize(O);
  plan.obs_point.resize(O);
  std::vector<int64_t> cursor(plan.image_offsets.begin(), plan.image_offsets.end() - 1);
  for (int64_t p = 0; p < m.num_points; ++p)
    for (int64_t o = m.track_offsets[p]; o < m.track_offsets[p + 1]; ++o) {
      plan.obs_point[(size_t)o] = (int32_t)p;
      plan.obs_order[(size_t)cursor[(size_t)m.track_image[o]]++] = (int32_t)o;
    }
  for (size_t i = 0; i < I; ++i)
    plan.select_ids[select_class(plan.image_offsets[i + 1] - plan.image_offsets[i])].push_back((int32_t)i);
  return plan;
}

inline int64_t device_bytes_depth(const model_flat& m) {
  const int64_t I = m.num_images, P = m.num_points, O = m.num_observations;
  // R, T, ranges; points; track_image, obs_order, obs_point, depth bits; image_offsets, select ids
  return I * (9 + 3 + 2) * 4 + P * 3 * 4 + O * 4 * 4 + (I + 1) * 8 + I * 4;
}

// ---- pair passes -------------------------------------------------------------------------------------------------------

struct PairPlan {
  std::vector<int32_t> class_points[kNumClasses];  // the points of each lane-group class, ascending; tracks shorter
                                                   // than 2 have no pair and are in no class
  int64_t total_pairs = 0;                         // sum of L (L - 1) / 2: pairs of track positions, equal images included
  int64_t num_cells = 0;
};

// of a validated model
inline PairPlan make_pair_plan(const model_flat& m) {
  PairPlan plan;
  plan.num_cells = num_cells(m.num_images);
  int64_t cell_bound = 0;
  for (int64_t p = 0; p < m.num_points; ++p) {
    const int64_t L = m.track_offsets[p + 1] - m.track_offsets[p];  // < 2^31: every term below is < 2^61
    if (L < 2) continue;
    plan.class_points[length_class(L)].push_back((int32_t)p);
    plan.total_pairs += L * (L - 1) / 2;
    MODEL_CHECK(plan.total_pairs <= kMaxTrackPairs, "the tracks hold more than 2^40 pairs of observations");
    cell_bound += (L / 2) * ((L + 1) / 2);
    MODEL_CHECK(cell_bound <= kMaxCellPairs, "one image pair could share more than 2^31 - 1 track pairs (the pair table counts in int32)");
  }
  return plan;
}

// before the count pass: the tables and the model; `pairs` more floats once the counts are known
inline int64_t device_bytes_pairs(const model_flat& m, const PairPlan& plan, int64_t pairs) {
  const int64_t I = m.num_images, P = m.num_points, O = m.num_observations;
  // R, T, centres (double); points; offsets + track_image + class lists; per cell: count, cursor, percentile angle
  // (int32 / float) and offset (int64), segment id; the angles
  return I * (12 * 4 + 3 * 8) + P * 3 * 4 + (P + 1) * 8 + O * 4 + P * 4 + plan.num_cells * (4 + 4 + 4 + 8 + 4) + 8 * 4096 +
         pairs * 4;
}

inline void check_device_memory(int64_t need, int64_t free_bytes) {
  MODEL_CHECK(need <= free_bytes, "the call needs " + std::to_string(need) + " bytes of device memory, the device has " +
                                      std::to_string(free_bytes) + " free");
}

// The non-empty cells by selection class (ascending), and the number of pairs they hold, from the count table.
struct CellSegments {
  std::vector<int32_t> select_ids[2];
  int64_t pairs = 0;
};

inline CellSegments make_cell_segments(const int32_t* counts, int64_t num_cells) {
  CellSegments s;
  for (int64_t c = 0; c < num_cells; ++c) {
    if (counts[c] <= 0) continue;
    s.select_ids[select_class(counts[c])].push_back((int32_t)c);
    s.pairs += counts[c];
  }
  return s;
}

// The pair table as the CSR of model_pairs: row i lists the images j != i with a non-empty cell, ascending.
inline void make_rows(const int32_t* counts, const float* angles, int32_t num_images, std::vector<int64_t>* row_offsets,
                      std::vector<int32_t>* other, std::vector<int32_t>* count, std::vector<float>* angle) {
  const int64_t I = num_images;
  row_offsets->assign((size_t)I + 1, 0);
  other->clear();
  count->clear();
  angle->clear();
  for (int64_t i = 0; i < I; ++i) {
    for (int64_t j = 0; j < I; ++j) {
      if (j == i) continue;
      const int64_t c = j < i ? cell_index(j, i, I) : cell_index(i, j, I);
      if (counts[c] <= 0) continue;
      other->push_back((int32_t)j);
      count->push_back(counts[c]);
      angle->push_back(angles[c]);
    }
    (*row_offsets)[(size_t)i + 1] = (int64_t)other->size();
  }
}

}  // namespace model_plan
#endif  // COLMAP_AMD_MODEL_PLAN_H_
