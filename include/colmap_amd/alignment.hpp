// alignment.hpp -- C++ host side of model alignment and comparison (reference estimators/alignment.h, geometry/sim3.h,
// solvers/similarity_transform.h: EstimateSim3dRobust) over the C ABI of colmap_amd_align.h. Header-only, standard
// library only.
//
//   colmap_amd::obs::Reconstruction src = ..., tgt = ...;
//   colmap_amd::align::Sim3d tgt_from_src;
//   if (colmap_amd::align::AlignReconstructionsViaReprojections(src, tgt, 0.3, 8.0, &tgt_from_src)) {
//     auto errors = colmap_amd::align::ComputeImageAlignmentError(src, tgt, tgt_from_src);
//     colmap_amd::align::Transform(&src, tgt_from_src);
//   }
//
// The hypotheses are scored on the GPU and the search loop of the library decides; the association step of
// AlignReconstructionsViaPoints, ComputeImageAlignmentError and the poses stay on the host. The Reconstruction is the
// slice of observation_manager.hpp, which carries no image names: images correspond by image id. Errors are
// std::runtime_error carrying align_last_error().
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <iomanip>
#include <limits>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../colmap_amd_align.h"
#include "observation_manager.hpp"

namespace colmap_amd {
namespace align {

using obs::Reconstruction;

inline void Check(int rc) {
  if (rc != 0) throw std::runtime_error(align_last_error());
}

inline void QuatToRotation(const double q[4] /* w x y z */, double R[9]) {
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}

// geometry/sim3.h: x -> scale * (R x) + translation
struct Sim3d {
  double scale = 1.0;
  std::array<double, 4> rotation{{1, 0, 0, 0}};  // w x y z
  std::array<double, 3> translation{{0, 0, 0}};

  std::array<double, 8> params() const {  // the order of ToFile and of the C ABI
    return {{scale, rotation[0], rotation[1], rotation[2], rotation[3], translation[0], translation[1], translation[2]}};
  }
  static Sim3d FromParams(const double p[8]) {
    Sim3d t;
    t.scale = p[0];
    for (int k = 0; k < 4; ++k) t.rotation[(size_t)k] = p[1 + k];
    for (int k = 0; k < 3; ++k) t.translation[(size_t)k] = p[5 + k];
    return t;
  }
  std::array<double, 3> operator*(const std::array<double, 3>& x) const {
    double R[9];
    QuatToRotation(rotation.data(), R);
    std::array<double, 3> o;
    for (int r = 0; r < 3; ++r) o[(size_t)r] = scale * (R[3 * r] * x[0] + R[3 * r + 1] * x[1] + R[3 * r + 2] * x[2]) + translation[(size_t)r];
    return o;
  }
  // geometry/sim3.cc:39-63: one line, 17 significant digits
  void ToFile(const std::string& path) const {
    std::ofstream file(path, std::ios::trunc);
    if (!file.good()) throw std::runtime_error("cannot write " + path);
    file.imbue(std::locale::classic());
    file.precision(17);
    const auto p = params();
    for (int k = 0; k < 8; ++k) file << p[(size_t)k] << (k < 7 ? " " : "\n");
  }
  static Sim3d FromFile(const std::string& path) {
    std::ifstream file(path);
    if (!file.good()) throw std::runtime_error("cannot read " + path);
    file.imbue(std::locale::classic());
    double p[8];
    for (int k = 0; k < 8; ++k)
      if (!(file >> p[k])) throw std::runtime_error(path + ": a Sim3d file holds 8 numbers");
    return FromParams(p);
  }
};

// geometry/sim3.h:98-105
inline Sim3d Inverse(const Sim3d& b_from_a) {
  Sim3d a_from_b;
  const double* q = b_from_a.rotation.data();
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  a_from_b.scale = 1 / b_from_a.scale;
  a_from_b.rotation = {{q[0] / n, -q[1] / n, -q[2] / n, -q[3] / n}};
  double R[9];
  QuatToRotation(a_from_b.rotation.data(), R);
  const auto& t = b_from_a.translation;
  for (int r = 0; r < 3; ++r)
    a_from_b.translation[(size_t)r] = (R[3 * r] * t[0] + R[3 * r + 1] * t[1] + R[3 * r + 2] * t[2]) / -b_from_a.scale;
  return a_from_b;
}

// colmap::RANSACOptions (optim/ransac.h:50-83); random_seed: the sample stream is deterministic, -1 does not exist
struct RANSACOptions {
  double max_error = 0.0;
  double min_inlier_ratio = 0.1;
  double confidence = 0.99;
  double dyn_num_trials_multiplier = 3.0;
  int min_num_trials = 0;
  int max_num_trials = std::numeric_limits<int>::max();
  int random_seed = 0;
  int batch_size = 0;  // hypotheses per launch, 0 = the library's default; the report does not depend on it
};

struct Report {  // RANSAC::Report
  bool success = false;
  size_t num_trials = 0;
  size_t num_inliers = 0;
  double residual_sum = 0.0;
  Sim3d model;
  std::vector<char> inlier_mask;
};

namespace detail {

inline align_options ToC(const RANSACOptions& o, double min_inlier_observations) {
  align_options c;
  align_options_init(&c);
  c.max_error = o.max_error;
  c.min_inlier_observations = min_inlier_observations;
  c.min_inlier_ratio = o.min_inlier_ratio;
  c.confidence = o.confidence;
  c.dyn_num_trials_multiplier = o.dyn_num_trials_multiplier;
  c.min_num_trials = o.min_num_trials;
  c.max_num_trials = o.max_num_trials;
  c.random_seed = o.random_seed;
  c.batch_size = o.batch_size;
  return c;
}

struct Handle {
  align_handle* h = nullptr;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() { align_destroy(h); }
};

template <typename Estimate>
Report Run(Estimate&& estimate, align_handle* h, const align_options& c, size_t num_samples) {
  std::vector<uint8_t> mask(num_samples, 0);
  align_report r{};
  r.inlier_mask = mask.empty() ? nullptr : mask.data();
  Check(estimate(h, &c, &r));
  Report out;
  out.success = r.success != 0;
  out.num_trials = (size_t)r.num_trials;
  out.num_inliers = (size_t)r.num_inliers;
  out.residual_sum = r.residual_sum;
  out.model = Sim3d::FromParams(r.model);
  out.inlier_mask.assign(mask.begin(), mask.end());
  return out;
}

inline align_camera ToC(const obs::Camera& c) {
  align_camera a{};
  a.model_id = c.model_id;
  a.width = c.width;
  a.height = c.height;
  if (c.params.size() > 16) throw std::runtime_error("a camera has at most 16 parameters");
  a.num_params = (int32_t)c.params.size();
  for (size_t k = 0; k < c.params.size(); ++k) a.params[k] = c.params[k];
  return a;
}

inline std::array<double, 3> ProjectionCenter(const std::array<double, 7>& p) {
  const double q[4] = {p[3], p[0], p[1], p[2]};
  double R[9];
  QuatToRotation(q, R);
  return {{-(R[0] * p[4] + R[3] * p[5] + R[6] * p[6]), -(R[1] * p[4] + R[4] * p[5] + R[7] * p[6]),
           -(R[2] * p[4] + R[5] * p[5] + R[8] * p[6])}};
}

}  // namespace detail

// Reconstruction::FindCommonRegImageIds (scene/reconstruction.cc:856-871); images correspond by id here
inline std::vector<std::pair<int, int>> FindCommonRegImageIds(const Reconstruction& src, const Reconstruction& tgt) {
  std::vector<std::pair<int, int>> ids;
  for (const auto& kv : src.images)
    if (tgt.images.count(kv.first)) ids.emplace_back(kv.first, kv.first);
  return ids;
}

// solvers/similarity_transform.cc:103-115 on the GPU
inline Report EstimateSim3dRobust(const std::vector<std::array<double, 3>>& src, const std::vector<std::array<double, 3>>& tgt,
                                  const RANSACOptions& options, int gpu_index = 0) {
  if (src.size() != tgt.size()) throw std::runtime_error("src and tgt must have the same number of points");
  detail::Handle handle;
  Check(align_positions_create(src.empty() ? nullptr : src[0].data(), tgt.empty() ? nullptr : tgt[0].data(), (int64_t)src.size(),
                               gpu_index, &handle.h));
  return detail::Run(align_positions_estimate, handle.h, detail::ToC(options, 0.0), src.size());
}

// alignment.cc:301-342. `options` replaces the reference's RANSACOptions (min_inlier_ratio = 0.2); its max_error is not
// used: the residual threshold is 1 - min_inlier_observations as there.
inline Report AlignReconstructionsViaReprojectionsReport(const Reconstruction& src, const Reconstruction& tgt,
                                                         double min_inlier_observations, double max_reproj_error,
                                                         RANSACOptions options, int gpu_index = 0) {
  const auto ids = FindCommonRegImageIds(src, tgt);
  std::vector<align_camera> sc, tc;
  std::vector<double> sp, tp, sxyz, txyz, sxy, txy;
  std::vector<int32_t> sn, tn, rec_image;
  for (size_t slot = 0; slot < ids.size(); ++slot) {
    const obs::Image& a = src.images.at(ids[slot].first);
    const obs::Image& b = tgt.images.at(ids[slot].second);
    sc.push_back(detail::ToC(src.cameras.at(a.camera_id)));
    tc.push_back(detail::ToC(tgt.cameras.at(b.camera_id)));
    sp.insert(sp.end(), a.cam_from_world.begin(), a.cam_from_world.end());
    tp.insert(tp.end(), b.cam_from_world.begin(), b.cam_from_world.end());
    sn.push_back((int32_t)a.points2D.size());
    tn.push_back((int32_t)b.points2D.size());
    for (size_t k = 0; k < std::min(a.points2D.size(), b.points2D.size()); ++k) {
      if (!a.points2D[k].HasPoint3D() || !b.points2D[k].HasPoint3D()) continue;
      rec_image.push_back((int32_t)slot);
      const obs::Point3D& pa = src.points3D.at(a.points2D[k].point3D_id);
      const obs::Point3D& pb = tgt.points3D.at(b.points2D[k].point3D_id);
      sxyz.insert(sxyz.end(), pa.xyz, pa.xyz + 3);
      txyz.insert(txyz.end(), pb.xyz, pb.xyz + 3);
      sxy.insert(sxy.end(), a.points2D[k].xy, a.points2D[k].xy + 2);
      txy.insert(txy.end(), b.points2D[k].xy, b.points2D[k].xy + 2);
    }
  }
  align_reproj_pair pair{};
  pair.num_images = (int32_t)ids.size();
  pair.num_records = (int64_t)rec_image.size();
  pair.src_cameras = sc.data();
  pair.tgt_cameras = tc.data();
  pair.src_poses = sp.data();
  pair.tgt_poses = tp.data();
  pair.src_num_points2D = sn.data();
  pair.tgt_num_points2D = tn.data();
  pair.rec_image = rec_image.data();
  pair.rec_src_xyz = sxyz.data();
  pair.rec_tgt_xyz = txyz.data();
  pair.rec_src_xy = sxy.data();
  pair.rec_tgt_xy = txy.data();
  detail::Handle handle;
  Check(align_reproj_create(&pair, gpu_index, &handle.h));
  options.max_error = max_reproj_error;
  return detail::Run(align_reproj_estimate, handle.h, detail::ToC(options, min_inlier_observations), ids.size());
}

inline bool AlignReconstructionsViaReprojections(const Reconstruction& src, const Reconstruction& tgt,
                                                 double min_inlier_observations, double max_reproj_error, Sim3d* tgt_from_src,
                                                 int gpu_index = 0) {
  if (!(min_inlier_observations >= 0.0 && min_inlier_observations <= 1.0))
    throw std::runtime_error("min_inlier_observations must lie in [0, 1]");
  if (FindCommonRegImageIds(src, tgt).size() < 3) return false;
  RANSACOptions options;
  options.min_inlier_ratio = 0.2;
  const Report report = AlignReconstructionsViaReprojectionsReport(src, tgt, min_inlier_observations, max_reproj_error, options, gpu_index);
  if (report.success) *tgt_from_src = report.model;
  return report.success;
}

// alignment.cc:185-238; tgt_image_ids stands for the reference's image names
inline bool AlignReconstructionToLocations(const Reconstruction& src, const std::vector<int>& tgt_image_ids,
                                           const std::vector<std::array<double, 3>>& tgt_image_locations, int min_common_images,
                                           const RANSACOptions& ransac_options, Sim3d* tgt_from_src, int gpu_index = 0) {
  if (min_common_images < 3) throw std::runtime_error("min_common_images must be at least 3");
  if (tgt_image_ids.size() != tgt_image_locations.size()) throw std::runtime_error("one location per image");
  std::set<int> common;
  std::vector<std::array<double, 3>> a, b;
  for (size_t i = 0; i < tgt_image_ids.size(); ++i) {
    const auto it = src.images.find(tgt_image_ids[i]);
    if (it == src.images.end()) continue;
    if (!common.insert(it->first).second) continue;  // duplicates are ignored
    a.push_back(detail::ProjectionCenter(it->second.cam_from_world));
    b.push_back(tgt_image_locations[i]);
  }
  if (common.size() < (size_t)min_common_images) return false;
  const Report report = EstimateSim3dRobust(a, b, ransac_options, gpu_index);
  if (report.num_inliers < (size_t)min_common_images) return false;
  if (tgt_from_src) *tgt_from_src = report.model;
  return true;
}

// alignment.cc:344-369
inline bool AlignReconstructionsViaProjCenters(const Reconstruction& src, const Reconstruction& tgt, double max_proj_center_error,
                                               Sim3d* tgt_from_src, int gpu_index = 0) {
  if (!(max_proj_center_error > 0)) throw std::runtime_error("max_proj_center_error must be positive");
  std::vector<int> ids;
  std::vector<std::array<double, 3>> centers;
  for (const auto& kv : tgt.images) {
    ids.push_back(kv.first);
    centers.push_back(detail::ProjectionCenter(kv.second.cam_from_world));
  }
  RANSACOptions options;
  options.max_error = max_proj_center_error;
  return AlignReconstructionToLocations(src, ids, centers, 3, options, tgt_from_src, gpu_index);
}

// The association step of AlignReconstructionsViaPoints (alignment.cc:411-447) as written: the count of a tgt point
// starts at 0, so it is the number of votes minus one; the first point with the largest count wins.
inline void AssociatePoints(const Reconstruction& src, const Reconstruction& tgt, size_t min_common_observations,
                            std::vector<std::array<double, 3>>* src_xyz, std::vector<std::array<double, 3>>* tgt_xyz) {
  for (const auto& kv : src.points3D) {
    std::vector<std::pair<int64_t, size_t>> counts;  // in order of first appearance
    for (const obs::TrackElement& el : kv.second.track) {
      const auto it = tgt.images.find(el.image_id);
      if (it == tgt.images.end()) continue;
      const obs::Point2D& p2 = it->second.points2D.at((size_t)el.point2D_idx);
      if (!p2.HasPoint3D()) continue;
      auto c = std::find_if(counts.begin(), counts.end(), [&](const std::pair<int64_t, size_t>& e) { return e.first == p2.point3D_id; });
      if (c != counts.end()) ++c->second; else counts.emplace_back(p2.point3D_id, 0);
    }
    if (counts.empty()) continue;
    const auto best = std::max_element(counts.begin(), counts.end(),
                                       [](const std::pair<int64_t, size_t>& a, const std::pair<int64_t, size_t>& b) { return a.second < b.second; });
    if (best->second >= min_common_observations) {
      const obs::Point3D& q = tgt.points3D.at(best->first);
      src_xyz->push_back({{kv.second.xyz[0], kv.second.xyz[1], kv.second.xyz[2]}});
      tgt_xyz->push_back({{q.xyz[0], q.xyz[1], q.xyz[2]}});
    }
  }
}

// alignment.cc:400-458
inline bool AlignReconstructionsViaPoints(const Reconstruction& src, const Reconstruction& tgt, size_t min_common_observations,
                                          double max_error, double min_inlier_ratio, Sim3d* tgt_from_src, int gpu_index = 0) {
  if (!(min_common_observations > 0 && max_error > 0.0 && min_inlier_ratio >= 0.0 && min_inlier_ratio <= 1.0))
    throw std::runtime_error("min_common_observations and max_error must be positive, min_inlier_ratio in [0, 1]");
  std::vector<std::array<double, 3>> a, b;
  AssociatePoints(src, tgt, min_common_observations, &a, &b);
  RANSACOptions options;
  options.max_error = max_error;
  options.min_inlier_ratio = min_inlier_ratio;
  const Report report = EstimateSim3dRobust(a, b, options, gpu_index);
  if (report.success) *tgt_from_src = report.model;
  return report.success;
}

struct ImageAlignmentError {
  int image_id = 0;  // stands for the reference's image_name
  double rotation_error_deg = 0.0;
  double proj_center_error = 0.0;
};

// alignment.cc:371-398, on the host
inline std::vector<ImageAlignmentError> ComputeImageAlignmentError(const Reconstruction& src, const Reconstruction& tgt,
                                                                   const Sim3d& tgt_from_src) {
  std::vector<ImageAlignmentError> errors;
  double R[9];
  QuatToRotation(tgt_from_src.rotation.data(), R);
  for (const auto& ids : FindCommonRegImageIds(src, tgt)) {
    const auto& pa = src.images.at(ids.first).cam_from_world;
    const auto& pb = tgt.images.at(ids.second).cam_from_world;
    const double qa[4] = {pa[3], pa[0], pa[1], pa[2]}, qb[4] = {pb[3], pb[0], pb[1], pb[2]};
    double Rc[9], Rb[9], Rn[9], tn[3];
    QuatToRotation(qa, Rc);
    QuatToRotation(qb, Rb);
    for (int r = 0; r < 3; ++r)  // TransformCameraWorld: R' = R_c R^T, t' = s t_c - R' t
      for (int c = 0; c < 3; ++c) Rn[3 * r + c] = Rc[3 * r] * R[3 * c] + Rc[3 * r + 1] * R[3 * c + 1] + Rc[3 * r + 2] * R[3 * c + 2];
    for (int r = 0; r < 3; ++r)
      tn[r] = tgt_from_src.scale * pa[4 + (size_t)r] - (Rn[3 * r] * tgt_from_src.translation[0] + Rn[3 * r + 1] * tgt_from_src.translation[1] +
                                                       Rn[3 * r + 2] * tgt_from_src.translation[2]);
    double diff2 = 0.0, dc2 = 0.0;
    for (int k = 0; k < 9; ++k) diff2 += (Rn[k] - Rb[k]) * (Rn[k] - Rb[k]);
    for (int c = 0; c < 3; ++c) {
      const double ca = -(Rn[c] * tn[0] + Rn[3 + c] * tn[1] + Rn[6 + c] * tn[2]);
      const double cb = -(Rb[c] * pb[4] + Rb[3 + c] * pb[5] + Rb[6 + c] * pb[6]);
      dc2 += (ca - cb) * (ca - cb);
    }
    ImageAlignmentError e;
    e.image_id = ids.first;
    // the angle between two rotations: 2 asin(|Ra - Rb|_F / (2 sqrt 2)), what angularDistance returns
    e.rotation_error_deg = 2.0 * std::asin(std::min(1.0, std::sqrt(diff2) / (2.0 * std::sqrt(2.0)))) * 57.29577951308232;
    e.proj_center_error = std::sqrt(dc2);
    errors.push_back(e);
  }
  return errors;
}

// new_from_old * X for every point, on the GPU (align_transform_points)
inline void TransformPoints(std::vector<std::array<double, 3>>* points, const Sim3d& new_from_old, int gpu_index = 0) {
  const auto p = new_from_old.params();
  Check(align_transform_points(points->empty() ? nullptr : (*points)[0].data(), (int64_t)points->size(), p.data(), gpu_index));
}

// Reconstruction::Transform (scene/reconstruction.cc:788-805) on the slice of observation_manager.hpp: the points on the
// GPU, the image poses on the host.
inline void Transform(Reconstruction* rec, const Sim3d& new_from_old, int gpu_index = 0) {
  std::vector<std::array<double, 3>> pts;
  for (const auto& kv : rec->points3D) pts.push_back({{kv.second.xyz[0], kv.second.xyz[1], kv.second.xyz[2]}});
  TransformPoints(&pts, new_from_old, gpu_index);
  size_t k = 0;
  for (auto& kv : rec->points3D) {
    for (int c = 0; c < 3; ++c) kv.second.xyz[c] = pts[k][(size_t)c];
    ++k;
  }
  const Sim3d inv = Inverse(new_from_old);
  for (auto& kv : rec->images) {
    auto& p = kv.second.cam_from_world;
    // cam_from_new = cam_from_old * old_from_new: rotation q_c * q_inv, translation s t_c - R' t
    const double a[4] = {p[3], p[0], p[1], p[2]};
    const double* b = inv.rotation.data();
    const double q[4] = {a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]};
    double Rn[9];
    QuatToRotation(q, Rn);
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    double t[3];
    for (int r = 0; r < 3; ++r)
      t[r] = new_from_old.scale * p[4 + (size_t)r] - (Rn[3 * r] * new_from_old.translation[0] + Rn[3 * r + 1] * new_from_old.translation[1] +
                                                       Rn[3 * r + 2] * new_from_old.translation[2]);
    p = {{q[1] / n, q[2] / n, q[3] / n, q[0] / n, t[0], t[1], t[2]}};
  }
}

}  // namespace align
}  // namespace colmap_amd
