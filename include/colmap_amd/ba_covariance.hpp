// ba_covariance.hpp -- C++ host side of the bundle-adjustment covariance (reference estimators/covariance.h:
// BACovarianceOptions, BACovariance, EstimateBACovariance) over the C ABI of colmap_amd_ba_covariance.h. Header-only,
// standard library only; BACovariance owns the ba_covariance handle (and with it L^-1 in device memory).
//
//   auto ba = CreateDefaultBundleAdjuster(options, config, reconstruction);
//   ba->Solve();
//   std::optional<BACovariance> cov = EstimateBACovariance(BACovarianceOptions(), reconstruction, *ba);
//   if (cov) { auto c = cov->GetCamCovFromWorld(image_id); ... }
//
// Matrices are MatrixXd (row-major, rows x cols doubles). "No result" is std::nullopt; when the estimate itself is not
// possible (rank-deficient system), EstimateBACovariance returns std::nullopt and ba_last_error() states the number of
// columns and the rank.
#pragma once

#include <array>
#include <cmath>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../colmap_amd_ba_covariance.h"
#include "bundle_adjustment.hpp"

namespace colmap_amd {

struct BACovarianceOptions {  // covariance.h
  enum class Params { POSES = BA_COV_POSES, POINTS = BA_COV_POINTS, POSES_AND_POINTS = BA_COV_POSES_AND_POINTS, ALL = BA_COV_ALL };
  Params params = Params::ALL;
  double damping = 1e-8;
};

struct MatrixXd {
  int rows = 0, cols = 0;
  std::vector<double> values;  // row-major
  MatrixXd() = default;
  MatrixXd(int r, int c) : rows(r), cols(c), values(static_cast<size_t>(r) * c, 0.0) {}
  double& operator()(int r, int c) { return values[static_cast<size_t>(r) * cols + c]; }
  double operator()(int r, int c) const { return values[static_cast<size_t>(r) * cols + c]; }
};

// Rigid3d::Adjoint / AdjointInverse and GetCovarianceForRelativeRigid3d (geometry/rigid3.h): tangent order
// [rotation, translation].
inline std::array<double, 36> Rigid3dAdjoint(const Rigid3d& t, bool inverse) {
  double R[9];
  QuatToRot(t.params.data(), R);
  const double* p = t.params.data() + 4;
  const double X[9] = {0, -p[2], p[1], p[2], 0, -p[0], -p[1], p[0], 0};  // [t]x
  std::array<double, 36> A{};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double rot = inverse ? R[3 * c + r] : R[3 * r + c];
      A[6 * r + c] = rot;
      A[6 * (r + 3) + c + 3] = rot;
      double m = 0.0;  // [t]x R, or -R^T [t]x
      for (int k = 0; k < 3; ++k) m += inverse ? -R[3 * k + r] * X[3 * k + c] : X[3 * r + k] * R[3 * k + c];
      A[6 * (r + 3) + c] = m;
    }
  return A;
}

inline MatrixXd GetCovarianceForRelativeRigid3d(const Rigid3d& a_from_c, const Rigid3d& b_from_c, const MatrixXd& covar) {
  if (covar.rows != 12 || covar.cols != 12) throw std::invalid_argument("covar must be 12 x 12");
  const auto Ab = Rigid3dAdjoint(b_from_c, false), Ai = Rigid3dAdjoint(a_from_c, true);
  MatrixXd J(6, 12);
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) {
      double m = 0.0;
      for (int k = 0; k < 6; ++k) m += Ab[6 * r + k] * Ai[6 * k + c];
      J(r, c) = -m;
    }
    J(r, 6 + r) = 1.0;
  }
  MatrixXd JC(6, 12), out(6, 6);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 12; ++c)
      for (int k = 0; k < 12; ++k) JC(r, c) += J(r, k) * covar(k, c);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c)
      for (int k = 0; k < 12; ++k) out(r, c) += JC(r, k) * J(c, k);
  return out;
}

class BACovariance {  // covariance.h
 public:
  struct Slots {
    std::map<image_t, int> pose_of_image;          // variable pose block of an image
    std::map<point3D_t, int> point_of_id;          // point block
    std::map<const double*, std::pair<int, int>> other_of_params;  // parameter array -> (BA_COV_KIND_*, index)
  };
  BACovariance(ba_covariance* handle, Slots slots) : handle_(handle, &ba_covariance_destroy), slots_(std::move(slots)) {}

  std::optional<MatrixXd> GetPointCov(point3D_t point3D_id) const {
    const auto it = slots_.point_of_id.find(point3D_id);
    if (it == slots_.point_of_id.end()) return std::nullopt;
    MatrixXd m(3, 3);
    if (ba_covariance_point(handle_.get(), it->second, m.values.data()) != BA_COV_OK) return std::nullopt;
    return m;
  }
  std::optional<MatrixXd> GetCamCovFromWorld(image_t image_id) const { return GetCamCrossCovFromWorld(image_id, image_id); }
  std::optional<MatrixXd> GetCamCrossCovFromWorld(image_t image_id1, image_t image_id2) const {
    const auto a = slots_.pose_of_image.find(image_id1), b = slots_.pose_of_image.find(image_id2);
    if (a == slots_.pose_of_image.end() || b == slots_.pose_of_image.end()) return std::nullopt;
    return Block(BA_COV_KIND_POSE, a->second, BA_COV_KIND_POSE, b->second);
  }
  std::optional<MatrixXd> GetCam2CovFromCam1(image_t image_id1, const Rigid3d& cam1_from_world, image_t image_id2,
                                             const Rigid3d& cam2_from_world) const {
    const auto c11 = GetCamCovFromWorld(image_id1), c22 = GetCamCovFromWorld(image_id2);
    if (!c11 || !c22 || c11->rows != 6 || c22->rows != 6) return std::nullopt;  // (partially) constant pose
    const auto c12 = GetCamCrossCovFromWorld(image_id1, image_id2);
    if (!c12) return std::nullopt;
    MatrixXd cov(12, 12);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        cov(r, c) = (*c11)(r, c);
        cov(6 + r, 6 + c) = (*c22)(r, c);
        cov(r, 6 + c) = (*c12)(r, c);
        cov(6 + c, r) = (*c12)(r, c);
      }
    return GetCovarianceForRelativeRigid3d(cam1_from_world, cam2_from_world, cov);
  }
  // Looked up by the identity of the parameter array (Camera::params.data(), a sensor_from_rig's params.data()).
  std::optional<MatrixXd> GetOtherParamsCov(const double* params) const {
    const auto it = slots_.other_of_params.find(params);
    if (it == slots_.other_of_params.end()) return std::nullopt;
    return Block(it->second.first, it->second.second, it->second.first, it->second.second);
  }

 private:
  std::optional<MatrixXd> Block(int kind_a, int index_a, int kind_b, int index_b) const {
    int32_t da = 0, db = 0;
    if (ba_covariance_block_dim(handle_.get(), kind_a, index_a, &da) != BA_COV_OK ||
        ba_covariance_block_dim(handle_.get(), kind_b, index_b, &db) != BA_COV_OK)
      return std::nullopt;
    const ba_covariance_pair pair{kind_a, index_a, kind_b, index_b};
    std::vector<double> out(BA_COV_SLOT);
    int32_t found = 0;
    if (ba_covariance_blocks(handle_.get(), 1, &pair, out.data(), &found) != BA_COV_OK) throw std::runtime_error(ba_last_error());
    if (!found) return std::nullopt;
    MatrixXd m(da, db);
    std::copy(out.begin(), out.begin() + static_cast<size_t>(da) * db, m.values.begin());
    return m;
  }

  std::unique_ptr<ba_covariance, void (*)(ba_covariance*)> handle_;
  Slots slots_;
};

// EstimateBACovariance (covariance.h) for an adjuster of this backend: the problem it built (blocks, manifolds, loss,
// priors) at its current values -- after Solve(), the solution. Images that are not the reference sensor of their
// frame throw, like the reference's THROW_CHECK(image.IsRefInFrame()).
inline std::optional<BACovariance> EstimateBACovariance(const BACovarianceOptions& options, const Reconstruction& reconstruction,
                                                        BundleAdjuster& bundle_adjuster) {
  auto* ba = dynamic_cast<Mi355xBundleAdjuster*>(&bundle_adjuster);
  if (!ba) throw std::invalid_argument("EstimateBACovariance: not an MI355X bundle adjuster");
  for (const auto& kv : reconstruction.images)
    if (!reconstruction.IsRefInFrame(kv.second))
      throw std::invalid_argument("EstimateBACovariance: an image is not the reference sensor of its frame");
  if (ba_abi_version() != COLMAP_AMD_BA_ABI_VERSION)
    throw std::runtime_error("libcolmap_amd.so and colmap_amd_ba.h disagree on the layout of ba_options / ba_result");
  ba_problem p = ba->Problem();
  const ba_options so = ba->SolveOptions();
  ba_covariance_options co;
  ba_covariance_options_init(&co);
  co.params = static_cast<int32_t>(options.params);
  co.damping = options.damping;
  ba_covariance* h = nullptr;
  const int rc = ba_estimate_covariance(&p, &so, &co, ba->GpuIndex(), &h);
  if (rc == BA_COV_NOT_ESTIMABLE) return std::nullopt;
  if (rc != BA_COV_OK) throw std::runtime_error(ba_last_error());
  std::unique_ptr<ba_covariance, void (*)(ba_covariance*)> guard(h, &ba_covariance_destroy);
  BACovariance::Slots slots;
  for (const auto& kv : reconstruction.images) {
    const int s = ba->VariablePoseSlotOfImage(kv.second);
    if (s >= 0) slots.pose_of_image.emplace(kv.first, s);
  }
  for (const auto& kv : reconstruction.points3D) {
    const int s = ba->PointSlotOf(kv.first);
    if (s >= 0) slots.point_of_id.emplace(kv.first, s);
  }
  for (const auto& kv : reconstruction.cameras) {
    const int s = ba->CamSlotOf(kv.first);
    if (s >= 0) slots.other_of_params.emplace(kv.second.params.data(), std::make_pair(static_cast<int>(BA_COV_KIND_CAMERA), s));
  }
  for (const auto& rig : reconstruction.rigs)
    for (const auto& kv : rig.second.sensors_from_rig) {
      const int s = ba->SensorSlotOf(kv.first);
      if (s >= 0) slots.other_of_params.emplace(kv.second.params.data(), std::make_pair(static_cast<int>(BA_COV_KIND_SENSOR), s));
    }
  return BACovariance(guard.release(), std::move(slots));
}

}  // namespace colmap_amd
