// observation_manager.hpp -- C++ host side of observation / point filtering (reference sfm/observation_manager.h: the
// filter methods of ObservationManager; scene/reconstruction.h: UpdatePoint3DErrors and the Compute* statistics) over
// the C ABI of colmap_amd_obs.h. Header-only, standard library only.
//
//   colmap_amd::obs::Reconstruction rec = ...;                  // cameras, images with their points2D, points3D
//   colmap_amd::obs::ObservationManager om(rec);
//   size_t n = om.FilterAllPoints3D(4.0, 1.5);                  // on the GPU; rec loses the filtered tracks and points
//   n += om.FilterPoints3DWithShortTracks(2);
//
// The library decides (one keep byte per observation, one status byte per point); this class flattens the
// reconstruction, applies the deletions and returns the reference's counts. Errors are std::runtime_error carrying
// obs_last_error().
#pragma once

#include <array>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../colmap_amd_obs.h"
#include "camera.hpp"

namespace colmap_amd {
namespace obs {

enum class ReprojectionErrorType { PIXEL = OBS_ERROR_PIXEL, NORMALIZED = OBS_ERROR_NORMALIZED, ANGULAR = OBS_ERROR_ANGULAR };

constexpr int64_t kInvalidPoint3DId = -1;

using Camera = ::colmap_amd::Camera;

struct Point2D {
  double xy[2] = {0.0, 0.0};
  int64_t point3D_id = kInvalidPoint3DId;
  bool HasPoint3D() const { return point3D_id != kInvalidPoint3DId; }
};

struct Image {
  int camera_id = 0;
  std::array<double, 7> cam_from_world{{0, 0, 0, 1, 0, 0, 0}};  // qx qy qz qw tx ty tz
  std::vector<Point2D> points2D;
};

struct TrackElement {
  int image_id = 0;
  int point2D_idx = 0;
  bool operator==(const TrackElement& o) const { return image_id == o.image_id && point2D_idx == o.point2D_idx; }
};

struct Point3D {
  double xyz[3] = {0.0, 0.0, 0.0};
  double error = -1.0;
  std::vector<TrackElement> track;
  bool HasError() const { return error != -1.0; }
};

struct Reconstruction {  // the slice of scene/reconstruction.h the filters touch
  std::map<int, Camera> cameras;
  std::map<int, Image> images;
  std::map<int64_t, Point3D> points3D;

  int64_t AddPoint3D(double x, double y, double z, const std::vector<TrackElement>& track = {}) {
    const int64_t id = ++last_point3D_id_;
    Point3D& p = points3D[id];
    p.xyz[0] = x;
    p.xyz[1] = y;
    p.xyz[2] = z;
    for (const TrackElement& el : track) AddObservation(id, el);
    return id;
  }
  void AddObservation(int64_t point3D_id, const TrackElement& el) {
    points3D.at(point3D_id).track.push_back(el);
    images.at(el.image_id).points2D.at(el.point2D_idx).point3D_id = point3D_id;
  }
  void DeletePoint3D(int64_t point3D_id) {
    for (const TrackElement& el : points3D.at(point3D_id).track)
      images.at(el.image_id).points2D.at(el.point2D_idx).point3D_id = kInvalidPoint3DId;
    points3D.erase(point3D_id);
  }
  size_t NumPoints3D() const { return points3D.size(); }
  size_t ComputeNumObservations() const {  // scene/reconstruction.cc:918-924
    size_t n = 0;
    for (const auto& kv : images)
      for (const Point2D& p : kv.second.points2D) n += p.HasPoint3D() ? 1 : 0;
    return n;
  }
  double ComputeMeanTrackLength() const {  // :926-932
    return points3D.empty() ? 0.0 : ComputeNumObservations() / static_cast<double>(points3D.size());
  }
  double ComputeMeanReprojectionError() const {  // :942-957
    double sum = 0.0;
    size_t n = 0;
    for (const auto& kv : points3D)
      if (kv.second.HasError()) {
        sum += kv.second.error;
        ++n;
      }
    return n == 0 ? 0.0 : sum / n;
  }
  inline void UpdatePoint3DErrors(int gpu_index = 0);  // :959-975, on the GPU (obs_point_errors)

 private:
  int64_t last_point3D_id_ = 0;
};

namespace detail {

struct Flat {
  std::vector<obs_camera> cameras;
  std::vector<double> poses, points, xy;
  std::vector<int32_t> image_camera, obs_image;
  std::vector<int64_t> offsets{0};
  std::vector<int64_t> ids;
  std::vector<uint8_t> keep, status;
  std::vector<double> error;
  obs_model model{};
  obs_result result{};
};

// the given points of the reconstruction (all of them when `subset` is null); ids that do not exist are skipped
inline void Flatten(const Reconstruction& rec, const std::vector<int64_t>* subset, Flat* f) {
  std::map<int, int32_t> cam_index, img_index;
  for (const auto& kv : rec.cameras) {
    obs_camera c{};
    c.model_id = kv.second.model_id;
    c.width = kv.second.width;
    c.height = kv.second.height;
    if (kv.second.params.size() > 16) throw std::runtime_error("a camera has more than 16 parameters");
    c.num_params = static_cast<int32_t>(kv.second.params.size());
    for (size_t i = 0; i < kv.second.params.size(); ++i) c.params[i] = kv.second.params[i];
    cam_index[kv.first] = static_cast<int32_t>(f->cameras.size());
    f->cameras.push_back(c);
  }
  for (const auto& kv : rec.images) {
    img_index[kv.first] = static_cast<int32_t>(f->image_camera.size());
    f->image_camera.push_back(cam_index.at(kv.second.camera_id));
    f->poses.insert(f->poses.end(), kv.second.cam_from_world.begin(), kv.second.cam_from_world.end());
  }
  auto add = [&](int64_t id, const Point3D& p) {
    f->ids.push_back(id);
    f->points.insert(f->points.end(), p.xyz, p.xyz + 3);
    for (const TrackElement& el : p.track) {
      f->obs_image.push_back(img_index.at(el.image_id));
      const Point2D& p2 = rec.images.at(el.image_id).points2D.at(el.point2D_idx);
      f->xy.push_back(p2.xy[0]);
      f->xy.push_back(p2.xy[1]);
    }
    f->offsets.push_back(static_cast<int64_t>(f->obs_image.size()));
  };
  if (subset) {
    std::unordered_set<int64_t> seen;
    for (int64_t id : *subset) {
      auto it = rec.points3D.find(id);
      if (it != rec.points3D.end() && seen.insert(id).second) add(id, it->second);
    }
  } else {
    for (const auto& kv : rec.points3D) add(kv.first, kv.second);
  }
  f->keep.resize(f->obs_image.size());
  f->status.resize(f->ids.size());
  f->error.resize(f->ids.size());
  obs_model& m = f->model;
  m.num_cameras = static_cast<int32_t>(f->cameras.size());
  m.num_images = static_cast<int32_t>(f->image_camera.size());
  m.num_points = static_cast<int64_t>(f->ids.size());
  m.num_observations = static_cast<int64_t>(f->obs_image.size());
  m.cameras = f->cameras.data();
  m.image_poses = f->poses.data();
  m.image_camera = f->image_camera.data();
  m.points = f->points.data();
  m.obs_offsets = f->offsets.data();
  m.obs_image = f->obs_image.data();
  m.obs_xy = f->xy.data();
  f->result.obs_keep = f->keep.data();
  f->result.point_status = f->status.data();
  f->result.point_error = f->error.data();
  f->result.point_count = nullptr;
}

inline void Check(int rc) {
  if (rc != 0) throw std::runtime_error(obs_last_error());
}

inline size_t Apply(Reconstruction* rec, const Flat& f, bool set_error) {
  for (size_t k = 0; k < f.ids.size(); ++k) {
    if (f.status[k] != OBS_POINT_KEPT) {
      rec->DeletePoint3D(f.ids[k]);
      continue;
    }
    Point3D& p = rec->points3D.at(f.ids[k]);
    std::vector<TrackElement> left;
    for (size_t j = 0; j < p.track.size(); ++j) {
      if (f.keep[f.offsets[k] + j]) {
        left.push_back(p.track[j]);
      } else {
        rec->images.at(p.track[j].image_id).points2D.at(p.track[j].point2D_idx).point3D_id = kInvalidPoint3DId;
      }
    }
    p.track.swap(left);
    if (set_error) p.error = f.error[k];
  }
  return static_cast<size_t>(f.result.num_filtered);
}

}  // namespace detail

inline void Reconstruction::UpdatePoint3DErrors(int gpu_index) {
  detail::Flat f;
  detail::Flatten(*this, nullptr, &f);
  detail::Check(obs_point_errors(&f.model, &f.result, gpu_index));
  for (size_t k = 0; k < f.ids.size(); ++k) points3D.at(f.ids[k]).error = f.error[k];
}

class ObservationManager {  // the filter methods of sfm/observation_manager.h
 public:
  explicit ObservationManager(Reconstruction& reconstruction, int gpu_index = 0)
      : reconstruction_(reconstruction), gpu_index_(gpu_index) {}

  // observation_manager.cc:353-363
  size_t FilterPoints3D(double max_reproj_error, double min_tri_angle, const std::vector<int64_t>& point3D_ids) {
    return Filter(&point3D_ids, OBS_RULE_REPROJ_ERROR | OBS_RULE_TRI_ANGLE, max_reproj_error, min_tri_angle,
                  ReprojectionErrorType::PIXEL);
  }
  // :365-379
  size_t FilterPoints3DInImages(double max_reproj_error, double min_tri_angle, const std::vector<int>& image_ids) {
    std::vector<int64_t> ids;
    for (int image_id : image_ids)
      for (const Point2D& p : reconstruction_.images.at(image_id).points2D)
        if (p.HasPoint3D()) ids.push_back(p.point3D_id);
    return FilterPoints3D(max_reproj_error, min_tri_angle, ids);
  }
  // :381-393
  size_t FilterAllPoints3D(double max_reproj_error, double min_tri_angle) {
    return Filter(nullptr, OBS_RULE_REPROJ_ERROR | OBS_RULE_TRI_ANGLE, max_reproj_error, min_tri_angle,
                  ReprojectionErrorType::PIXEL);
  }
  // :395-407
  size_t FilterPoints3DWithShortTracks(size_t min_track_length) {
    detail::Flat f;
    detail::Flatten(reconstruction_, nullptr, &f);
    obs_filter_options o;
    obs_filter_options_init(&o);
    o.min_track_len = static_cast<int32_t>(min_track_length);
    detail::Check(obs_filter_short_tracks(&f.model, &o, &f.result, gpu_index_));
    return detail::Apply(&reconstruction_, f, false);
  }
  // :409-433
  size_t FilterObservationsWithNegativeDepth() {
    detail::Flat f;
    detail::Flatten(reconstruction_, nullptr, &f);
    detail::Check(obs_filter_negative_depth(&f.model, &f.result, gpu_index_));
    return detail::Apply(&reconstruction_, f, false);
  }
  // :496-585
  size_t FilterPoints3DWithLargeReprojectionError(double max_error, const std::vector<int64_t>& point3D_ids,
                                                  ReprojectionErrorType error_type = ReprojectionErrorType::PIXEL) {
    return Filter(&point3D_ids, OBS_RULE_REPROJ_ERROR, max_error, 0.0, error_type);
  }
  // :435-494
  size_t FilterPoints3DWithSmallTriangulationAngle(double min_tri_angle, const std::vector<int64_t>& point3D_ids) {
    return Filter(&point3D_ids, OBS_RULE_TRI_ANGLE, 0.0, min_tri_angle, ReprojectionErrorType::PIXEL);
  }

 private:
  size_t Filter(const std::vector<int64_t>* ids, int rules, double max_reproj_error, double min_tri_angle,
                ReprojectionErrorType error_type) {
    detail::Flat f;
    detail::Flatten(reconstruction_, ids, &f);
    obs_filter_options o;
    obs_filter_options_init(&o);
    o.max_reproj_error = max_reproj_error;
    o.min_tri_angle = min_tri_angle;
    o.error_type = static_cast<int32_t>(error_type);
    o.rules = rules;
    detail::Check(obs_filter_all_points3D(&f.model, &o, &f.result, gpu_index_));
    return detail::Apply(&reconstruction_, f, (rules & OBS_RULE_REPROJ_ERROR) != 0);
  }

  Reconstruction& reconstruction_;
  int gpu_index_;
};

}  // namespace obs
}  // namespace colmap_amd
