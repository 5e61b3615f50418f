// two_view_geometry.hpp -- C++ host side of two-view geometry estimation (reference estimators/two_view_geometry.h,
// scene/two_view_geometry.h) over the C ABI of colmap_amd_tvg.h. Header-only, standard library only.
//
//   colmap_amd::tvg::TwoViewGeometryOptions options;
//   colmap_amd::tvg::Camera cam1{PINHOLE, 1000, 800, 1, false}, cam2{PINHOLE, 1000, 800, 2, false};
//   auto geometry = colmap_amd::tvg::EstimateTwoViewGeometry(cam1, points1, cam2, points2, matches, options);
//   if (geometry.config == TVG_CONFIG_UNCALIBRATED) use(*geometry.F, geometry.inlier_matches);
//
// Built are the routes of EstimateTwoViewGeometry that need only a fundamental matrix and a homography; a pair on
// another route (calibrated, shared focal, one-sided focal, spherical) comes back with config TVG_CONFIG_NOT_BUILT from
// EstimateTwoViewGeometries and makes EstimateTwoViewGeometry throw. Samples are solved and models scored on the GPU; the
// search and the decisions are the library's. Errors are std::runtime_error carrying tvg_last_error().
#pragma once

#include <array>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../colmap_amd_tvg.h"

namespace colmap_amd {
namespace tvg {

inline void Check(int rc) {
  if (rc != 0) throw std::runtime_error(tvg_last_error());
}

// estimators/two_view_geometry.h:44-131, the options of the built routes; the defaults are the reference's
struct TwoViewGeometryOptions : tvg_options {
  TwoViewGeometryOptions() { tvg_options_init(this); }
};

// what the router reads of a colmap::Camera
struct Camera {
  int model_id = 0;
  int width = 0, height = 0;
  int camera_id = 0;
  bool has_prior_focal_length = false;
  tvg_camera c() const { return tvg_camera{model_id, width, height, camera_id, has_prior_focal_length ? 1 : 0}; }
};

using Point2D = std::array<double, 2>;
using FeatureMatch = std::pair<uint32_t, uint32_t>;  // point2D_idx1, point2D_idx2
using Matrix3d = std::array<double, 9>;              // row-major

// scene/two_view_geometry.h
struct TwoViewGeometry {
  int config = TVG_CONFIG_UNDEFINED;
  int route = TVG_ROUTE_UNCALIBRATED;
  std::vector<FeatureMatch> inlier_matches;
  std::optional<Matrix3d> F, H;
};

struct ImagePair {
  Camera camera1, camera2;
  const std::vector<Point2D>* points1 = nullptr;
  const std::vector<Point2D>* points2 = nullptr;
  const std::vector<FeatureMatch>* matches = nullptr;
  uint64_t stream_id = 0;  // the key of the pair's sample stream, e.g. its pair id
};

// EstimateTwoViewGeometry for a batch of pairs in one call
inline std::vector<TwoViewGeometry> EstimateTwoViewGeometries(const std::vector<ImagePair>& pairs,
                                                              const TwoViewGeometryOptions& options = TwoViewGeometryOptions(),
                                                              int gpu_index = 0) {
  const size_t P = pairs.size();
  std::vector<tvg_camera> c1(P), c2(P);
  std::vector<int64_t> offsets(P + 1, 0);
  std::vector<double> points;
  std::vector<uint64_t> streams(P);
  for (size_t p = 0; p < P; ++p) {
    const ImagePair& q = pairs[p];
    if (!q.points1 || !q.points2 || !q.matches) throw std::runtime_error("pair " + std::to_string(p) + ": null points or matches");
    c1[p] = q.camera1.c();
    c2[p] = q.camera2.c();
    streams[p] = q.stream_id;
    for (const FeatureMatch& m : *q.matches) {
      if (m.first >= q.points1->size() || m.second >= q.points2->size())
        throw std::runtime_error("pair " + std::to_string(p) + ": a match points past the points of its image");
      const Point2D &a = (*q.points1)[m.first], &b = (*q.points2)[m.second];
      points.insert(points.end(), {a[0], a[1], b[0], b[1]});
    }
    offsets[p + 1] = (int64_t)(points.size() / 4);
  }
  std::vector<int32_t> route(P), config(P), has_F(P), has_H(P);
  std::vector<double> F(9 * P), H(9 * P);
  std::vector<uint8_t> mask(points.size() / 4 + 1);
  tvg_handle* handle = nullptr;
  Check(tvg_create(gpu_index, &handle));
  const int rc = tvg_verify_pairs(handle, &options, (int32_t)P, c1.data(), c2.data(), offsets.data(), points.data(), streams.data(),
                                  route.data(), config.data(), has_F.data(), F.data(), has_H.data(), H.data(), mask.data(), nullptr);
  tvg_destroy(handle);
  Check(rc);
  std::vector<TwoViewGeometry> out(P);
  for (size_t p = 0; p < P; ++p) {
    TwoViewGeometry& g = out[p];
    g.config = config[p];
    g.route = route[p];
    Matrix3d m;
    if (has_F[p]) {
      for (int k = 0; k < 9; ++k) m[(size_t)k] = F[9 * p + (size_t)k];
      g.F = m;
    }
    if (has_H[p]) {
      for (int k = 0; k < 9; ++k) m[(size_t)k] = H[9 * p + (size_t)k];
      g.H = m;
    }
    for (int64_t i = offsets[p]; i < offsets[p + 1]; ++i)
      if (mask[(size_t)i]) g.inlier_matches.push_back((*pairs[p].matches)[(size_t)(i - offsets[p])]);
  }
  return out;
}

// EstimateTwoViewGeometry (estimators/two_view_geometry.cc:552-640) of one pair; throws for a route that is not built
inline TwoViewGeometry EstimateTwoViewGeometry(const Camera& camera1, const std::vector<Point2D>& points1, const Camera& camera2,
                                               const std::vector<Point2D>& points2, const std::vector<FeatureMatch>& matches,
                                               const TwoViewGeometryOptions& options = TwoViewGeometryOptions(),
                                               uint64_t stream_id = 0, int gpu_index = 0) {
  ImagePair pair{camera1, camera2, &points1, &points2, &matches, stream_id};
  TwoViewGeometry g = EstimateTwoViewGeometries({pair}, options, gpu_index)[0];
  if (g.config == TVG_CONFIG_NOT_BUILT)
    throw std::runtime_error(std::string("the ") + tvg_route_name(g.route) +
                             " route of EstimateTwoViewGeometry is not built: it needs an essential matrix or a focal solver");
  return g;
}

}  // namespace tvg
}  // namespace colmap_amd
