// feature_matching.hpp -- C++ host side of SIFT descriptor matching (reference feature/types.h: FeatureMatch,
// FeatureMatches; feature/sift.h: SiftMatchingOptions; feature/matcher.h: FeatureMatcher) over the C ABI of
// colmap_amd_match.h. Header-only, standard library only.
//
//   colmap_amd::FeatureMatcher matcher(colmap_amd::SiftMatchingOptions(), /*gpu_index=*/0);
//   matcher.SetDescriptors(1, rows1, data1);       // uint8 [rows][128], kept on the device under the image id
//   matcher.SetDescriptors(2, rows2, data2);
//   colmap_amd::FeatureMatches matches;
//   matcher.Match(1, 2, &matches);
//   auto all = matcher.Match({{1, 2}, {1, 3}, {2, 3}});   // one launch
//
// Errors are std::runtime_error carrying match_last_error(). There is no CPU path.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../colmap_amd_match.h"

namespace colmap_amd {

typedef uint32_t image_t;
typedef uint32_t point2D_t;

// feature/types.h
struct FeatureMatch {
  point2D_t point2D_idx1 = 0xffffffffu;
  point2D_t point2D_idx2 = 0xffffffffu;
  FeatureMatch() = default;
  FeatureMatch(point2D_t idx1, point2D_t idx2) : point2D_idx1(idx1), point2D_idx2(idx2) {}
  bool operator==(const FeatureMatch& o) const { return point2D_idx1 == o.point2D_idx1 && point2D_idx2 == o.point2D_idx2; }
};
typedef std::vector<FeatureMatch> FeatureMatches;

// feature/sift.h SiftMatchingOptions, with the two fields of FeatureMatchingOptions and TwoViewGeometryOptions that the
// brute-force GPU matcher and its controller read
struct SiftMatchingOptions {
  double max_ratio = 0.8;
  double max_distance = 0.7;
  bool cross_check = true;
  int max_num_matches = 32768;
  int min_num_inliers = 15;

  bool Check() const { return max_ratio > 0 && max_distance > 0 && max_num_matches > 0 && min_num_inliers >= 0; }
};

class FeatureMatcher {
 public:
  explicit FeatureMatcher(const SiftMatchingOptions& options = SiftMatchingOptions(), int gpu_index = 0,
                          size_t cache_bytes = 0)
      : options_(options) {
    if (!options.Check()) throw std::runtime_error("SiftMatchingOptions::Check failed");
    Check(match_create(gpu_index, options.max_num_matches, cache_bytes, &handle_));
  }
  FeatureMatcher(const FeatureMatcher&) = delete;
  FeatureMatcher& operator=(const FeatureMatcher&) = delete;
  ~FeatureMatcher() { match_destroy(handle_); }

  // descriptors: [rows][128] uint8, row-major (FeatureDescriptors)
  void SetDescriptors(image_t image_id, int rows, const uint8_t* descriptors) {
    Check(match_set_descriptors(handle_, image_id, rows, MATCH_DESCRIPTOR_DIM, descriptors));
  }
  bool HasDescriptors(image_t image_id) { return match_has_descriptors(handle_, image_id) != 0; }

  // FeatureMatcher::Match for two resident images
  void Match(image_t image_id1, image_t image_id2, FeatureMatches* matches) {
    *matches = std::move(Match({{image_id1, image_id2}})[0]);
  }

  // all pairs in one launch; result k belongs to pairs[k]
  std::vector<FeatureMatches> Match(const std::vector<std::pair<image_t, image_t>>& pairs) {
    std::vector<match_pair> list;
    list.reserve(pairs.size());
    for (const auto& p : pairs) list.push_back(match_pair{p.first, p.second});
    match_options o;
    match_options_init(&o);
    o.max_ratio = (float)options_.max_ratio;
    o.max_distance = (float)options_.max_distance;
    o.cross_check = options_.cross_check ? 1 : 0;
    o.min_num_inliers = options_.min_num_inliers;
    Check(match_pairs(handle_, list.data(), (int32_t)list.size(), &o));
    std::vector<FeatureMatches> out(pairs.size());
    std::vector<uint32_t> flat;
    for (size_t k = 0; k < pairs.size(); ++k) {
      int64_t count = 0;
      Check(match_num_matches(handle_, (int32_t)k, &count));
      flat.resize(2 * (size_t)count);
      Check(match_copy_matches(handle_, (int32_t)k, flat.data(), count));
      out[k].reserve(count);
      for (int64_t m = 0; m < count; ++m) out[k].emplace_back(flat[2 * m], flat[2 * m + 1]);
    }
    return out;
  }

 private:
  static void Check(int rc) {
    if (rc != 0) throw std::runtime_error(match_last_error());
  }
  SiftMatchingOptions options_;
  match_handle* handle_ = nullptr;
};

}  // namespace colmap_amd
