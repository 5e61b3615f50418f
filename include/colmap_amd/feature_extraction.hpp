// feature_extraction.hpp -- C++ host side of SIFT feature extraction (reference feature/sift.h: SiftExtractionOptions,
// CreateSiftFeatureExtractor; feature/types.h: FeatureKeypoint, FeatureDescriptors; feature/extractor.h:
// FeatureExtractor::Extract) over the C ABI of colmap_amd_sift.h. Header-only, standard library only.
//
//   auto extractor = colmap_amd::CreateSiftFeatureExtractor(colmap_amd::SiftExtractionOptions(), /*gpu_index=*/0);
//   colmap_amd::FeatureKeypoints keypoints;
//   colmap_amd::FeatureDescriptors descriptors;
//   extractor->Extract(colmap_amd::GreyBitmap{width, height, pixels}, &keypoints, &descriptors);
//
// The arithmetic is the reference's VLFeat route (SiftCPUFeatureExtractor::Extract, feature/sift.cc:138-341). Errors are
// std::runtime_error carrying sift_last_error(). There is no CPU path.
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../colmap_amd_sift.h"

namespace colmap_amd {

// feature/sift.h:41-101, the members of the built route
struct SiftExtractionOptions {
  enum class Normalization { L1_ROOT = SIFT_NORMALIZATION_L1_ROOT, L2 = SIFT_NORMALIZATION_L2 };
  int max_num_features = 8192;
  int first_octave = -1;
  int num_octaves = 4;
  int octave_resolution = 3;
  double peak_threshold = 0.02 / 3.0;
  double edge_threshold = 10.0;
  int max_num_orientations = 2;
  bool upright = false;
  Normalization normalization = Normalization::L1_ROOT;

  sift_options c() const {
    sift_options o;
    sift_options_init(&o);
    o.max_num_features = max_num_features;
    o.first_octave = first_octave;
    o.num_octaves = num_octaves;
    o.octave_resolution = octave_resolution;
    o.peak_threshold = peak_threshold;
    o.edge_threshold = edge_threshold;
    o.max_num_orientations = max_num_orientations;
    o.upright = upright ? 1 : 0;
    o.normalization = (int32_t)normalization;
    return o;
  }
  // SiftExtractionOptions::Check (sift.cc:72-84) and the limits of the kernels
  bool Check(std::string* why = nullptr) const {
    const sift_options o = c();
    const std::string bad = sift_options_check(&o);
    if (why) *why = bad;
    return bad.empty();
  }
};

// feature/types.h FeatureKeypoint (feature/types.cc:38-155)
struct FeatureKeypoint {
  float x = 0, y = 0, a11 = 1, a12 = 0, a21 = 0, a22 = 1;
  FeatureKeypoint() = default;
  FeatureKeypoint(float x_, float y_) : x(x_), y(y_) {}
  FeatureKeypoint(float x_, float y_, float scale, float orientation) : x(x_), y(y_) {
    if (!(scale >= 0.0f)) throw std::runtime_error("FeatureKeypoint: scale must not be negative");
    const float scale_cos_orientation = scale * std::cos(orientation);
    const float scale_sin_orientation = scale * std::sin(orientation);
    a11 = scale_cos_orientation;
    a12 = -scale_sin_orientation;
    a21 = scale_sin_orientation;
    a22 = scale_cos_orientation;
  }
  FeatureKeypoint(float x_, float y_, float a11_, float a12_, float a21_, float a22_)
      : x(x_), y(y_), a11(a11_), a12(a12_), a21(a21_), a22(a22_) {}
  void Rescale(float scale) { Rescale(scale, scale); }
  void Rescale(float scale_x, float scale_y) {
    if (!(scale_x > 0 && scale_y > 0)) throw std::runtime_error("FeatureKeypoint::Rescale: scales must be positive");
    x *= scale_x;
    y *= scale_y;
    a11 *= scale_x;
    a12 *= scale_y;
    a21 *= scale_x;
    a22 *= scale_y;
  }
  float ComputeScaleX() const { return std::sqrt(a11 * a11 + a21 * a21); }
  float ComputeScaleY() const { return std::sqrt(a12 * a12 + a22 * a22); }
  float ComputeScale() const { return (ComputeScaleX() + ComputeScaleY()) / 2.0f; }
  float ComputeOrientation() const { return std::atan2(a21, a11); }
};
typedef std::vector<FeatureKeypoint> FeatureKeypoints;

// feature/types.h FeatureDescriptors: rows x 128 bytes, row-major
struct FeatureDescriptors {
  int rows = 0;
  std::vector<uint8_t> data;
  const uint8_t* row(int r) const { return data.data() + (size_t)r * SIFT_DESCRIPTOR_DIM; }
};

// What Extract reads of a Bitmap: 8-bit grey pixels, row-major
struct GreyBitmap {
  int width = 0, height = 0;
  const uint8_t* data = nullptr;
};

// feature/extractor.h FeatureExtractor with the SIFT extractor behind it
class FeatureExtractor {
 public:
  FeatureExtractor(const SiftExtractionOptions& options, int gpu_index) : options_(options) {
    std::string why;
    if (!options.Check(&why)) throw std::runtime_error("SiftExtractionOptions::Check failed: " + why);
    Check(sift_create(gpu_index, &handle_));
  }
  FeatureExtractor(const FeatureExtractor&) = delete;
  FeatureExtractor& operator=(const FeatureExtractor&) = delete;
  ~FeatureExtractor() { sift_destroy(handle_); }

  // FeatureExtractor::Extract (sift.cc:158-336); descriptors may be null
  bool Extract(const GreyBitmap& bitmap, FeatureKeypoints* keypoints, FeatureDescriptors* descriptors) {
    if (!keypoints) throw std::runtime_error("Extract: keypoints must not be null");
    const sift_options o = options_.c();
    Check(sift_extract(handle_, bitmap.data, bitmap.width, bitmap.height, &o));
    const int64_t n = sift_num_features(handle_);
    std::vector<float> flat(4 * (size_t)n);
    Check(sift_copy_keypoints(handle_, flat.data(), n));
    keypoints->clear();
    keypoints->reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) keypoints->emplace_back(flat[4 * i], flat[4 * i + 1], flat[4 * i + 2], flat[4 * i + 3]);
    if (descriptors) {
      descriptors->rows = (int)n;
      descriptors->data.resize((size_t)n * SIFT_DESCRIPTOR_DIM);
      Check(sift_copy_descriptors(handle_, descriptors->data.data(), n));
    }
    return true;
  }

 private:
  static void Check(int rc) {
    if (rc != 0) throw std::runtime_error(sift_last_error());
  }
  SiftExtractionOptions options_;
  sift_handle* handle_ = nullptr;
};

// CreateSiftFeatureExtractor (feature/sift.cc): the GPU extractor
inline std::unique_ptr<FeatureExtractor> CreateSiftFeatureExtractor(const SiftExtractionOptions& options = SiftExtractionOptions(),
                                                                    int gpu_index = 0) {
  return std::make_unique<FeatureExtractor>(options, gpu_index);
}

}  // namespace colmap_amd
