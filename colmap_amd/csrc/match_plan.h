// match_plan.h -- everything descriptor matching decides on the host: the checks on the caller's arguments, the device
// image of a descriptor set, the tile table one launch walks, and the finish that turns the device's (idx, best, second)
// triples into FeatureMatches. Plain C++17: no HIP runtime -- feature_match.hip uploads what is built here;
// tests/cpp/test_match_plan.cc runs it without a GPU.
//
// The arithmetic is the reference's (feature/sift.cc:772-864, 967-1004): dot(i, j) = sum_k A[i][k] * B[j][k] over uint8
// is at most 128 * 255^2 = 8 323 200 < 2^24, so its float image is exact and the device may keep integers. Per row,
// best = the largest dot, idx = the SMALLEST column that attains it, second = the largest dot once one instance of best
// is removed; all start at 0, 0, -1 and only a dot > 0 counts. These definitions do not depend on the scan order, so two
// partial results merge as best = max, second = max(min(b1, b2), s1, s2), smaller index on equal best.
// The decision is the reference's float code, with the C library's acosf:
//   d1 = acosf(min(best / 262144, 1)), d2 likewise from second; reject d1 > max_distance; reject d1 >= max_ratio * d2.
#ifndef COLMAP_AMD_MATCH_PLAN_H_
#define COLMAP_AMD_MATCH_PLAN_H_

#include "../../include/colmap_amd_match.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace match_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define MATCH_CHECK(cond, msg)                                                    \
  do {                                                                            \
    if (!(cond)) throw ::match_plan::Fail(std::string("Check failed: ") + (msg)); \
  } while (0)

constexpr int kDim = MATCH_DESCRIPTOR_DIM;
constexpr int kWaveRows = 64;               // query rows of one wave: 4 MFMA tiles of 16
constexpr int kTileRows = 4 * kWaveRows;    // query rows of one workgroup (4 waves)
constexpr int kChunkRows = 64;              // rows of the other set one LDS chunk holds; sets are padded to this
constexpr int kRowBias = 128 * 128 * 128;   // 2 097 152: sum_k 128 * 128
// corr of a padding row. A real row's biased value acc + corr = dot - 128 * sum(query) is above -2^22; this is below
// all of them and (kAbsent << 8) is exactly INT32_MIN, so the packed key of the kernel cannot overflow.
constexpr int32_t kAbsent = -(1 << 23);
constexpr size_t kDefaultCacheBytes = (size_t)4 << 30;

inline int padded_rows(int rows) { return (rows + kChunkRows - 1) / kChunkRows * kChunkRows; }
inline size_t device_bytes(int rows) { return (size_t)padded_rows(rows) * (kDim + sizeof(int32_t)); }

// ---------------------------------------------------------------------------------------------------------------------
// checks
// ---------------------------------------------------------------------------------------------------------------------

inline int effective_max_num_matches(int max_num_matches) {
  MATCH_CHECK(max_num_matches >= 0, "max_num_matches must not be negative");
  return max_num_matches == 0 ? (int)MATCH_DEFAULT_MAX_NUM_MATCHES : max_num_matches;
}

// room for one pair of full sets at the least: a batch of one must always fit
inline size_t effective_cache_bytes(size_t cache_bytes, int max_num_matches) {
  const size_t floor = 2 * device_bytes(max_num_matches);
  return std::max(cache_bytes == 0 ? kDefaultCacheBytes : cache_bytes, floor);
}

// the rows of a set that take part (sift.cc:1404-1418 warns and truncates); *truncated tells the caller to warn
inline int check_descriptors(int rows, int cols, const uint8_t* data, int max_num_matches, bool* truncated) {
  MATCH_CHECK(rows >= 0, "descriptor rows must not be negative");
  MATCH_CHECK(cols == kDim, "descriptors must have 128 columns (SIFT), got " + std::to_string(cols));
  MATCH_CHECK(rows == 0 || data != nullptr, "descriptor data is null");
  *truncated = rows > max_num_matches;
  return *truncated ? max_num_matches : rows;
}

inline void check_options(const match_options* o) {
  MATCH_CHECK(o != nullptr, "options is null");
  MATCH_CHECK(o->max_ratio > 0.0f, "max_ratio must be positive");      // SiftMatchingOptions::Check
  MATCH_CHECK(o->max_distance > 0.0f, "max_distance must be positive");
  MATCH_CHECK(o->min_num_inliers >= 0, "min_num_inliers must not be negative");
}

// ---------------------------------------------------------------------------------------------------------------------
// device image of a set: rows padded to kChunkRows; desc = byte ^ 0x80 (the value x - 128 as int8, the matrix
// instruction is signed), padding rows 0; corr[row] = 128 * sum(row) - 2 097 152, padding rows kAbsent. With both
// operands biased, sum_k (a - 128)(b - 128) + corr_a + 128 * sum(b) is the unsigned dot exactly, in int32.
// ---------------------------------------------------------------------------------------------------------------------

inline void build_device_image(const uint8_t* data, int rows, std::vector<int8_t>* desc, std::vector<int32_t>* corr) {
  const int padded = padded_rows(rows);
  desc->assign((size_t)padded * kDim, 0);
  corr->assign(padded, kAbsent);
  for (int r = 0; r < rows; ++r) {
    int32_t sum = 0;
    for (int k = 0; k < kDim; ++k) {
      const uint8_t v = data[(size_t)r * kDim + k];
      sum += v;
      (*desc)[(size_t)r * kDim + k] = (int8_t)(v ^ 0x80);
    }
    (*corr)[r] = 128 * sum - kRowBias;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// tile table: one workgroup per kTileRows query rows of one direction of one pair
// ---------------------------------------------------------------------------------------------------------------------

struct Tile {
  int32_t query_set;    // index into the launch's set table
  int32_t stream_set;
  int32_t query_row0;
  int32_t reserved;
  int64_t out_row0;     // row of the launch's output where the direction's results start
};

struct PairSlots {
  int32_t set1, set2;   // indices into the set table
};

struct Launch {
  std::vector<Tile> tiles;
  std::vector<int64_t> out_row0;  // [2 * pair + direction]
  int64_t out_rows = 0;
};

inline Launch build_launch(const std::vector<int32_t>& set_rows, const PairSlots* pairs, int n) {
  MATCH_CHECK(n >= 0, "number of pairs must not be negative");
  MATCH_CHECK(n == 0 || pairs != nullptr, "pairs is null");
  Launch L;
  L.out_row0.resize(2 * (size_t)n);
  const int num_sets = (int)set_rows.size();
  for (int p = 0; p < n; ++p) {
    const int32_t s[2] = {pairs[p].set1, pairs[p].set2};
    for (int d = 0; d < 2; ++d)
      MATCH_CHECK(s[d] >= 0 && s[d] < num_sets, "pair " + std::to_string(p) + " names an unknown descriptor slot");
    for (int d = 0; d < 2; ++d) {
      const int rows = set_rows[s[d]];
      L.out_row0[2 * (size_t)p + d] = L.out_rows;
      for (int r0 = 0; r0 < rows; r0 += kTileRows) L.tiles.push_back(Tile{s[d], s[1 - d], r0, 0, L.out_rows});
      L.out_rows += rows;
    }
  }
  return L;
}

// ---------------------------------------------------------------------------------------------------------------------
// finish
// ---------------------------------------------------------------------------------------------------------------------

// FindBestMatchesOneWayBruteForce's decision for one row (sift.cc:798-822): the matched column or -1
inline int32_t decide(const int32_t sel[3], float max_ratio, float max_distance) {
  constexpr float kInvSqDescriptorNorm = (float)(1.0 / (512.0 * 512.0));
  if (sel[0] < 0) return -1;
  const float d1 = acosf(std::min(kInvSqDescriptorNorm * (float)sel[1], 1.0f));
  if (d1 > max_distance) return -1;
  const float d2 = acosf(std::min(kInvSqDescriptorNorm * (float)sel[2], 1.0f));
  if (d1 >= max_ratio * d2) return -1;
  return sel[0];
}

// FindBestMatchesBruteForce (sift.cc:828-864) on the two directions' triples, then the controller's min_num_inliers
// cut (feature_matching_utils.cc:502-505). matches: pairs (idx1, idx2), ascending idx1.
inline void finish(const int32_t* sel12, int64_t n1, const int32_t* sel21, int64_t n2, const match_options& o,
                   std::vector<uint32_t>* matches) {
  matches->clear();
  MATCH_CHECK(n1 == 0 || sel12 != nullptr, "selection of direction 0 is null");
  MATCH_CHECK(n2 == 0 || sel21 != nullptr, "selection of direction 1 is null");
  std::vector<int32_t> m21;
  if (o.cross_check) {
    m21.resize(n2);
    for (int64_t j = 0; j < n2; ++j) m21[j] = decide(sel21 + 3 * j, o.max_ratio, o.max_distance);
  }
  for (int64_t i = 0; i < n1; ++i) {
    const int32_t j = decide(sel12 + 3 * i, o.max_ratio, o.max_distance);
    if (j < 0) continue;
    MATCH_CHECK(j < n2, "selection names a column beyond the other set");
    if (o.cross_check && m21[j] != (int32_t)i) continue;
    matches->push_back((uint32_t)i);
    matches->push_back((uint32_t)j);
  }
  if ((int64_t)(matches->size() / 2) < o.min_num_inliers) matches->clear();
}

inline void options_init(match_options* o) {
  o->max_ratio = 0.8f;
  o->max_distance = 0.7f;
  o->cross_check = 1;
  o->min_num_inliers = 15;
}

}  // namespace match_plan

#endif  // COLMAP_AMD_MATCH_PLAN_H_
