// colmap_amd/model.hpp -- colmap_amd::mvs::Model: the statistics of mvs::Model (reference src/colmap/mvs/model.{h,cc})
// on the MI355X, header-only over the C ABI of include/colmap_amd_model.h. The caller fills `images` and `points`
// (reading sparse-model files is not part of this header); every statistic is computed on the GPU, there is no CPU
// path. The return types are the reference's.
//
//   Model model;
//   model.AddImage("a.png", Image(path, width, height, K, R, T));  ...
//   model.points.push_back({x, y, z, {0, 1, 4}});                   ...
//   auto ranges = model.ComputeDepthRanges();                  // -> PatchMatchOptions::depth_min / depth_max of image i
//   auto overlapping = model.GetMaxOverlappingImages(50, 0.0); // -> StereoFusion::Run(inputs, overlapping)
#ifndef COLMAP_AMD_MODEL_HPP_
#define COLMAP_AMD_MODEL_HPP_

#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../colmap_amd_model.h"
#include "mvs.hpp"

namespace colmap_amd {
namespace mvs {

class Model {
 public:
  struct Point {  // mvs/model.h:50-55
    float x = 0, y = 0, z = 0;
    std::vector<int> track;
  };

  std::vector<Image> images;
  std::vector<Point> points;
  int gpu_index = 0;

  // appends an image under a name, the way the reference's readers fill images / image_names_ / image_name_to_idx_
  int AddImage(const std::string& name, const Image& image) {
    const int idx = (int)images.size();
    images.push_back(image);
    image_names_.push_back(name);
    image_name_to_idx_.emplace(name, idx);
    return idx;
  }

  int GetImageIdx(const std::string& name) const {  // model.cc:108-112
    const auto it = image_name_to_idx_.find(name);
    if (it == image_name_to_idx_.end()) throw std::invalid_argument("Image with name `" + name + "` does not exist");
    return it->second;
  }

  const std::string& GetImageName(int image_idx) const {  // model.cc:114-118
    if (image_idx < 0) throw std::invalid_argument("Check failed: image_idx >= 0");
    if ((size_t)image_idx >= image_names_.size()) throw std::invalid_argument("Check failed: image_idx < image_names_.size()");
    return image_names_[(size_t)image_idx];
  }

  // model.cc:120-171; equal shared counts in ascending image index
  std::vector<std::vector<int>> GetMaxOverlappingImages(size_t num_images, double min_triangulation_angle) const {
    const Flat f(*this);
    const size_t I = images.size();
    const size_t per_row = I == 0 ? 0 : (num_images < I - 1 ? num_images : I - 1);
    std::vector<int64_t> ptr(I + 1, 0);
    std::vector<int32_t> idx(per_row * I + 1);
    size_t total = 0;
    const int64_t wanted = num_images > (size_t)INT32_MAX ? (int64_t)INT32_MAX : (int64_t)num_images;
    Check(model_get_max_overlapping_images(&f.model, wanted, min_triangulation_angle, ptr.data(), idx.data(), &total, gpu_index));
    std::vector<std::vector<int>> overlapping(I);
    for (size_t i = 0; i < I; ++i) overlapping[i].assign(idx.begin() + ptr[i], idx.begin() + ptr[i + 1]);
    return overlapping;
  }

  std::vector<std::pair<float, float>> ComputeDepthRanges() const {  // model.cc:178-218
    const Flat f(*this);
    std::vector<float> ranges(2 * images.size() + 1);
    Check(model_compute_depth_ranges(&f.model, ranges.data(), gpu_index));
    std::vector<std::pair<float, float>> out(images.size());
    for (size_t i = 0; i < images.size(); ++i) out[i] = {ranges[2 * i], ranges[2 * i + 1]};
    return out;
  }

  std::vector<std::map<int, int>> ComputeSharedPoints() const {  // model.cc:220-235
    const Pairs p(*this, 75.0);
    std::vector<std::map<int, int>> out(images.size());
    for (size_t i = 0; i < images.size(); ++i)
      for (int64_t e = p.row_offsets[i]; e < p.row_offsets[i + 1]; ++e) out[i].emplace_hint(out[i].end(), p.other[e], p.count[e]);
    return out;
  }

  std::vector<std::map<int, float>> ComputeTriangulationAngles(float percentile = 50) const {  // model.cc:237-277
    const Pairs p(*this, (double)percentile);
    std::vector<std::map<int, float>> out(images.size());
    for (size_t i = 0; i < images.size(); ++i)
      for (int64_t e = p.row_offsets[i]; e < p.row_offsets[i + 1]; ++e) out[i].emplace_hint(out[i].end(), p.other[e], p.angle[e]);
    return out;
  }

  // the flat arrays of model_flat, owned
  struct Flat {
    std::vector<float> R, T, xyz;
    std::vector<int64_t> offsets;
    std::vector<int32_t> track_image;
    model_flat model{};
    explicit Flat(const Model& m) {
      for (const Image& im : m.images) {
        R.insert(R.end(), im.GetR(), im.GetR() + 9);
        T.insert(T.end(), im.GetT(), im.GetT() + 3);
      }
      offsets.push_back(0);
      for (const Point& p : m.points) {
        xyz.insert(xyz.end(), {p.x, p.y, p.z});
        track_image.insert(track_image.end(), p.track.begin(), p.track.end());
        offsets.push_back((int64_t)track_image.size());
      }
      model.num_images = (int32_t)m.images.size();
      model.num_points = (int64_t)m.points.size();
      model.num_observations = (int64_t)track_image.size();
      model.R = R.data();
      model.T = T.data();
      model.points = xyz.data();
      model.track_offsets = offsets.data();
      model.track_image = track_image.data();
    }
  };

 private:
  static void Check(int rc) {
    if (rc != 0) throw std::runtime_error(model_last_error());
  }

  struct Pairs {
    std::vector<int64_t> row_offsets;
    std::vector<int32_t> other, count;
    std::vector<float> angle;
    Pairs(const Model& m, double percentile) {
      const Flat f(m);
      model_pairs* handle = nullptr;
      Check(model_compute_pair_statistics(&f.model, percentile, &handle, m.gpu_index));
      int32_t num_images = 0;
      size_t n = 0;
      model_pairs_size(handle, &num_images, &n);
      row_offsets.resize((size_t)num_images + 1);
      other.resize(n);
      count.resize(n);
      angle.resize(n);
      model_pairs_get(handle, row_offsets.data(), other.data(), count.data(), angle.data());
      model_pairs_free(handle);
    }
  };

  std::vector<std::string> image_names_;
  std::unordered_map<std::string, int> image_name_to_idx_;
};

}  // namespace mvs
}  // namespace colmap_amd
#endif  // COLMAP_AMD_MODEL_HPP_
