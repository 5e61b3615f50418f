// undistort_plan.h -- everything image undistortion decides on the host: the option and argument checks, the undistorted
// camera (UndistortCamera), the rectifying homographies (RectifyStereoCameras), and per image one ImagePlan: its route, its
// cameras, the homography the kernel receives, buffer sizes and launch grids. Plain C++17: no HIP runtime -- undistort.hip
// plans with it, then uploads and launches what a plan says; tests/cpp/test_undistort_plan.cc checks it without a GPU.
// (camera_projection.h wants __host__, __device__ and __forceinline__ to exist: a host-only includer defines them empty.)
#ifndef COLMAP_AMD_UNDISTORT_PLAN_H_
#define COLMAP_AMD_UNDISTORT_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_undistort.h"
#include "camera_projection.h"

namespace undistort_plan {

namespace ud = camera;

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};
#define UD_CHECK(cond, msg) \
  do {                      \
    if (!(cond)) throw ::undistort_plan::Fail(msg); \
  } while (0)

constexpr int kPixelsPerLane = 4;             // a lane of the image kernels owns 4 adjacent pixels of a row
constexpr unsigned kBlockX = 64, kBlockY = 4;  // their workgroup

inline void check_camera(const undistort_cam& c) {
  UD_CHECK(ud::num_params(c.model_id) > 0, "unknown camera model id " + std::to_string(c.model_id));
  UD_CHECK(c.width > 0 && c.height > 0, "camera width and height must be positive");
}

// a device image of W x H x C bytes whose rows hold whole 4-pixel groups
inline int padded_pitch(int W, int C) { return (W + kPixelsPerLane - 1) / kPixelsPerLane * kPixelsPerLane * C; }

struct Grid { unsigned x, y; };  // of a launch with the block above
inline Grid image_grid(int W, int H) {
  return Grid{((W + kPixelsPerLane - 1) / kPixelsPerLane + kBlockX - 1) / kBlockX, (H + kBlockY - 1) / kBlockY};
}

inline void options_init(undistort_options* o) {
  o->blank_pixels = 0.0;
  o->min_scale = 0.2;
  o->max_scale = 2.0;
  o->max_image_size = -1;
  o->interpolation = UNDISTORT_BILINEAR;
  o->roi_min_x = 0.0;
  o->roi_min_y = 0.0;
  o->roi_max_x = 1.0;
  o->roi_max_y = 1.0;
  o->max_cam_point_norm = -1.0;
  o->direct_warp_min_scale = 0.5;
}

inline void check_options(const undistort_options& o) {  // image/undistortion.cc:60-70
  UD_CHECK(o.blank_pixels >= 0, "Check failed: options.blank_pixels >= 0");
  UD_CHECK(o.blank_pixels <= 1, "Check failed: options.blank_pixels <= 1");
  UD_CHECK(o.min_scale > 0.0, "Check failed: options.min_scale > 0.0");
  UD_CHECK(o.min_scale <= o.max_scale, "Check failed: options.min_scale <= options.max_scale");
  UD_CHECK(o.max_image_size != 0, "Check failed: options.max_image_size != 0");
  UD_CHECK(o.roi_min_x >= 0.0, "Check failed: options.roi_min_x >= 0.0");
  UD_CHECK(o.roi_min_y >= 0.0, "Check failed: options.roi_min_y >= 0.0");
  UD_CHECK(o.roi_max_x <= 1.0, "Check failed: options.roi_max_x <= 1.0");
  UD_CHECK(o.roi_max_y <= 1.0, "Check failed: options.roi_max_y <= 1.0");
  UD_CHECK(o.roi_min_x < o.roi_max_x, "Check failed: options.roi_min_x < options.roi_max_x");
  UD_CHECK(o.roi_min_y < o.roi_max_y, "Check failed: options.roi_min_y < options.roi_max_y");
}

// Camera::Rescale(new_width, new_height) (scene/camera.cc:123-131) with CameraModelRescale (sensor/models.h:376-387,
// :399-405)
inline void rescale_camera(undistort_cam* c, int new_width, int new_height) {
  const double sx = (double)new_width / (double)c->width, sy = (double)new_height / (double)c->height;
  c->width = new_width;
  c->height = new_height;
  if (ud::is_spherical(c->model_id)) {
    c->params[0] *= sx;
    c->params[1] *= sy;
  } else if (ud::one_focal(c->model_id)) {
    c->params[0] *= 0.5 * (sx + sy);
    c->params[1] *= sx;
    c->params[2] *= sy;
  } else {
    c->params[0] *= sx;
    c->params[1] *= sy;
    c->params[2] *= sx;
    c->params[3] *= sy;
  }
}

// RescaleToMaxImageSize (image/undistortion.cc:43-54) through Camera::Rescale(scale) (scene/camera.cc:113-121)
inline void rescale_to_max_image_size(const undistort_options& o, undistort_cam* c) {
  if (o.max_image_size < 0) return;
  const double scale = std::min(o.max_image_size / (double)c->width, o.max_image_size / (double)c->height);
  if (scale < 1.0)
    rescale_camera(c, (int)std::round(scale * c->width), (int)std::round(scale * c->height));
}

inline void undistort_camera_impl(const undistort_options& o, const undistort_cam& cam, undistort_cam* out) {
  check_options(o);
  check_camera(cam);
  UD_CHECK(ud::is_perspective(cam.model_id), "Check failed: camera.IsPerspective()");
  const int m = cam.model_id;
  const ud::Intrinsics k = ud::intrinsics(m, cam.params);
  undistort_cam u;
  std::memset(&u, 0, sizeof(u));
  u.model_id = ud::PINHOLE;
  u.width = cam.width;
  u.height = cam.height;
  u.params[0] = k.f1;
  u.params[1] = k.f2;
  u.params[2] = k.c1;
  u.params[3] = k.c2;

  long long roi_min_x = 0, roi_min_y = 0, roi_max_x = cam.width, roi_max_y = cam.height;
  const bool roi_enabled = o.roi_min_x > 0.0 || o.roi_min_y > 0.0 || o.roi_max_x < 1.0 || o.roi_max_y < 1.0;
  if (roi_enabled) {  // :104-127
    roi_min_x = (long long)std::round(o.roi_min_x * (double)cam.width);
    roi_min_y = (long long)std::round(o.roi_min_y * (double)cam.height);
    roi_max_x = (long long)std::round(o.roi_max_x * (double)cam.width);
    roi_max_y = (long long)std::round(o.roi_max_y * (double)cam.height);
    roi_min_x = std::min<long long>(roi_min_x, cam.width - 1);
    roi_min_y = std::min<long long>(roi_min_y, cam.height - 1);
    roi_max_x = std::max(roi_max_x, roi_min_x + 1);
    roi_max_y = std::max(roi_max_y, roi_min_y + 1);
    u.width = (int)(roi_max_x - roi_min_x);
    u.height = (int)(roi_max_y - roi_min_y);
    u.params[2] = k.c1 - (double)roi_min_x;
    u.params[3] = k.c2 - (double)roi_min_y;
  }

  if (roi_enabled || (m != ud::SIMPLE_PINHOLE && m != ud::PINHOLE)) {  // :130-257
    UD_CHECK(o.max_cam_point_norm != 0, "Check failed: options.max_cam_point_norm != 0");
    const double max_norm_sq = o.max_cam_point_norm < 0 ? std::numeric_limits<double>::infinity()
                                                        : o.max_cam_point_norm * o.max_cam_point_norm;
    const double dmax = std::numeric_limits<double>::max(), dlow = std::numeric_limits<double>::lowest();
    // traces one border point into the undistorted camera; false = skipped
    auto trace = [&](double x, double y, double* ux, double* uy) {
      double cu, cv;
      if (!ud::cam_from_img(m, cam.params, x, y, &cu, &cv)) return false;
      if (!(cu * cu + cv * cv < max_norm_sq)) return false;
      return ud::img_from_normalized(ud::PINHOLE, u.params, cu, cv, ux, uy);
    };
    double left_min_x = dmax, left_max_x = dlow, right_min_x = dmax, right_max_x = dlow;
    for (long long y = roi_min_y; y < roi_max_y; ++y) {
      double ux, uy;
      if (trace(0.5, y + 0.5, &ux, &uy)) {
        left_min_x = std::min(left_min_x, ux);
        left_max_x = std::max(left_max_x, ux);
      }
      if (trace(cam.width - 0.5, y + 0.5, &ux, &uy)) {
        right_min_x = std::min(right_min_x, ux);
        right_max_x = std::max(right_max_x, ux);
      }
    }
    double top_min_y = dmax, top_max_y = dlow, bottom_min_y = dmax, bottom_max_y = dlow;
    for (long long x = roi_min_x; x < roi_max_x; ++x) {
      double ux, uy;
      if (trace(x + 0.5, 0.5, &ux, &uy)) {
        top_min_y = std::min(top_min_y, uy);
        top_max_y = std::max(top_max_y, uy);
      }
      if (trace(x + 0.5, cam.height - 0.5, &ux, &uy)) {
        bottom_min_y = std::min(bottom_min_y, uy);
        bottom_max_y = std::max(bottom_max_y, uy);
      }
    }
    const double cx = u.params[2], cy = u.params[3];
    const double min_scale_x = std::min(cx / (cx - left_min_x), (u.width - 0.5 - cx) / (right_max_x - cx));
    const double min_scale_y = std::min(cy / (cy - top_min_y), (u.height - 0.5 - cy) / (bottom_max_y - cy));
    const double max_scale_x = std::max(cx / (cx - left_max_x), (u.width - 0.5 - cx) / (right_min_x - cx));
    const double max_scale_y = std::max(cy / (cy - top_max_y), (u.height - 0.5 - cy) / (bottom_min_y - cy));
    double scale_x = 1.0 / (min_scale_x * o.blank_pixels + max_scale_x * (1.0 - o.blank_pixels));
    double scale_y = 1.0 / (min_scale_y * o.blank_pixels + max_scale_y * (1.0 - o.blank_pixels));
    // Clamp (util/math.h): std::max(low, std::min(value, high))
    scale_x = std::max(o.min_scale, std::min(scale_x, o.max_scale));
    scale_y = std::max(o.min_scale, std::min(scale_y, o.max_scale));
    const int orig_w = u.width, orig_h = u.height;
    u.width = (int)std::max(1.0, scale_x * u.width);
    u.height = (int)std::max(1.0, scale_y * u.height);
    u.params[2] = u.params[2] * (double)u.width / (double)orig_w;
    u.params[3] = u.params[3] * (double)u.height / (double)orig_h;
  }
  if (o.max_image_size > 0) rescale_to_max_image_size(o, &u);
  *out = u;
}

// Camera::CamFromImg for n pixels xy [n][2] -> uv [n][2]; NaN where the reference returns no value
inline void cam_from_img(const undistort_cam& camera, const double* xy, int64_t n, double* uv) {
  check_camera(camera);
  for (int64_t i = 0; i < n; ++i) {
    double u, v;
    if (!ud::cam_from_img(camera.model_id, camera.params, xy[2 * i], xy[2 * i + 1], &u, &v))
      u = v = std::numeric_limits<double>::quiet_NaN();
    uv[2 * i] = u;
    uv[2 * i + 1] = v;
  }
}

// ShouldWarpDirectly (image/warp.cc:72-89)
inline bool should_warp_directly(const undistort_cam& s, const undistort_cam& t, double direct_warp_min_scale) {
  UD_CHECK(direct_warp_min_scale >= 0, "Check failed: options.direct_warp_min_scale >= 0");
  if (t.width == s.width && t.height == s.height) return true;
  const double scale_x = (double)t.width / (double)s.width, scale_y = (double)t.height / (double)s.height;
  return std::min(scale_x, scale_y) >= direct_warp_min_scale;
}

// ---- RectifyStereoCameras (image/undistortion.cc:384-445), Eigen's operations restated on row-major 3x3 arrays ----
inline void mat3_mul(const double* a, const double* b, double* c) {
  double r[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
  std::memcpy(c, r, sizeof(r));
}

inline void mat3_vec(const double* a, const double* v, double* out) {
  double r[3];
  for (int i = 0; i < 3; ++i) r[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
  std::memcpy(out, r, sizeof(r));
}

// Eigen::AngleAxisd::toRotationMatrix
inline void rotation_from_angle_axis(double angle, const double* axis, double* m) {
  const double s = std::sin(angle), c = std::cos(angle);
  const double sa[3] = {s * axis[0], s * axis[1], s * axis[2]};
  const double ca[3] = {(1.0 - c) * axis[0], (1.0 - c) * axis[1], (1.0 - c) * axis[2]};
  double tmp = ca[0] * axis[1];
  m[1] = tmp - sa[2];
  m[3] = tmp + sa[2];
  tmp = ca[0] * axis[2];
  m[2] = tmp + sa[1];
  m[6] = tmp - sa[1];
  tmp = ca[1] * axis[2];
  m[5] = tmp - sa[0];
  m[7] = tmp + sa[0];
  m[0] = ca[0] * axis[0] + c;
  m[4] = ca[1] * axis[1] + c;
  m[8] = ca[2] * axis[2] + c;
}

// Eigen::AngleAxisd(Matrix3d): through the quaternion (Eigen/src/Geometry/Quaternion.h quaternionbase_assign_impl,
// AngleAxis.h operator=(QuaternionBase)); angle in [0, pi], axis (1, 0, 0) for the identity
inline void angle_axis_from_rotation(const double* m, double* angle, double* axis) {
  double q[4];  // x, y, z, w
  double t = m[0] + m[4] + m[8];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
    q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
    q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
  }
  double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  if (n != 0.0) {
    *angle = 2.0 * std::atan2(n, std::fabs(q[3]));
    if (q[3] < 0.0) n = -n;
    axis[0] = q[0] / n;
    axis[1] = q[1] / n;
    axis[2] = q[2] / n;
  } else {
    *angle = 0.0;
    axis[0] = 1.0;
    axis[1] = axis[2] = 0.0;
  }
}

// the inverse of a 3x3 matrix by cofactors; false when the determinant is 0 or not finite
inline bool mat3_inverse(const double* a, double* inv) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
  const double r[9] = {c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                       c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                       c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det};
  std::memcpy(inv, r, sizeof(r));
  return true;
}

inline void rectify_cameras_impl(const undistort_cam& cam1, const undistort_cam& cam2, const double* R, const double* t_in,
                                 double* H1, double* H2, double* Q) {
  check_camera(cam1);
  check_camera(cam2);
  UD_CHECK(cam1.model_id == ud::SIMPLE_PINHOLE || cam1.model_id == ud::PINHOLE,
           "Check failed: camera1.model_id == SimplePinholeCameraModel::model_id || camera1.model_id == "
           "PinholeCameraModel::model_id");
  UD_CHECK(cam2.model_id == ud::SIMPLE_PINHOLE || cam2.model_id == ud::PINHOLE,
           "Check failed: camera2.model_id == SimplePinholeCameraModel::model_id || camera2.model_id == "
           "PinholeCameraModel::model_id");
  // the average rotation between the first and the second camera (:395-400)
  double angle, axis[3], R1[9], R2[9], t[3];
  angle_axis_from_rotation(R, &angle, axis);
  angle *= -0.5;
  rotation_from_angle_axis(angle, axis, R2);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R1[3 * i + j] = R2[3 * j + i];
  // the translation, such that it coincides with the x axis (:402-419)
  mat3_vec(R2, t_in, t);
  double x_unit[3] = {1.0, 0.0, 0.0};
  if (t[0] * x_unit[0] + t[1] * x_unit[1] + t[2] * x_unit[2] < 0.0) x_unit[0] = -1.0;
  const double rot_axis[3] = {t[1] * x_unit[2] - t[2] * x_unit[1], t[2] * x_unit[0] - t[0] * x_unit[2],
                              t[0] * x_unit[1] - t[1] * x_unit[0]};
  const double rot_norm = std::sqrt(rot_axis[0] * rot_axis[0] + rot_axis[1] * rot_axis[1] + rot_axis[2] * rot_axis[2]);
  double R_x[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (!(rot_norm < std::numeric_limits<double>::epsilon())) {
    const double t_norm = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    const double x_norm = std::sqrt(x_unit[0] * x_unit[0] + x_unit[1] * x_unit[1] + x_unit[2] * x_unit[2]);
    const double a = std::acos(std::fabs(t[0] * x_unit[0] + t[1] * x_unit[1] + t[2] * x_unit[2]) / (t_norm * x_norm));
    const double n[3] = {rot_axis[0] / rot_norm, rot_axis[1] / rot_norm, rot_axis[2] / rot_norm};
    rotation_from_angle_axis(a, n, R_x);
  }
  mat3_mul(R_x, R1, R1);
  mat3_mul(R_x, R2, R2);
  mat3_vec(R_x, t, t);
  // the intrinsic calibration matrix (:426-431)
  const ud::Intrinsics k1 = ud::intrinsics(cam1.model_id, cam1.params), k2 = ud::intrinsics(cam2.model_id, cam2.params);
  const double f = std::min((k1.f1 + k1.f2) / 2.0, (k2.f1 + k2.f2) / 2.0);
  const double K[9] = {f, 0, k1.c1, 0, f, (k1.c2 + k2.c2) / 2.0, 0, 0, 1};
  double K1[9] = {k1.f1, 0, k1.c1, 0, k1.f2, k1.c2, 0, 0, 1}, K2[9] = {k2.f1, 0, k2.c1, 0, k2.f2, k2.c2, 0, 0, 1};
  UD_CHECK(mat3_inverse(K1, K1) && mat3_inverse(K2, K2), "a calibration matrix is singular");
  mat3_mul(K, R1, H1);
  mat3_mul(H1, K1, H1);
  mat3_mul(K, R2, H2);
  mat3_mul(H2, K2, H2);
  // [x, y, disparity, 1] * Q = [X, Y, Z, 1] * w (:437-444), entries as the reference writes them
  for (int i = 0; i < 16; ++i) Q[i] = (i % 5 == 0) ? 1.0 : 0.0;
  Q[12] = -K[5];
  Q[13] = -K[2];
  Q[14] = K[0];
  Q[11] = -1.0 / t[0];
  Q[15] = 0.0;
}

// ---- the plan of one image: what the device loop of undistort.hip executes without deciding anything ----
enum Route {
  kClone,    // a spherical source whose target has its size: a host memcpy (Bitmap::Clone), no device work
  kResize,   // the resize kernel alone (a spherical source with max_image_size; undistort_resize)
  kDirect,   // one warp or rectify launch
  kIndirect  // image/warp.cc:103-106, 141-143: a launch on the mid camera at the source's resolution, then the shrink
};

struct ImagePlan {
  Route route;
  undistort_cam source, target, mid;  // mid (kIndirect): the target camera rescaled to the source's size
  bool has_homography;                // a homography in front of the launch's camera: the rectify kernel, else the warp kernel
  double hinv[9];                     // what that kernel receives; for kIndirect conjugated with the pixel scaling
  int interpolation, channels;
  size_t in_bytes, out_words, mid_words;  // the source image; the padded device images of target and mid, in dwords
  Grid grid, mid_grid;                    // of the launch into the target image / into the mid image
};

// everything of a plan that follows from its route: sizes, grids and, for kIndirect, the mid camera and the conjugation
inline ImagePlan make_plan(Route route, const undistort_cam& src, const undistort_cam& tgt, int channels, int interpolation,
                           const double* hinv) {
  ImagePlan p = {};
  p.route = route;
  p.source = src;
  p.target = tgt;
  p.has_homography = hinv != nullptr;
  if (hinv) std::memcpy(p.hinv, hinv, sizeof(p.hinv));
  p.interpolation = interpolation;
  p.channels = channels;
  p.in_bytes = (size_t)src.width * src.height * channels;
  p.out_words = (size_t)padded_pitch(tgt.width, channels) / 4 * tgt.height;
  p.grid = image_grid(tgt.width, tgt.height);
  if (route != kIndirect) return p;
  p.mid = tgt;
  rescale_camera(&p.mid, src.width, src.height);
  p.mid_words = (size_t)padded_pitch(p.mid.width, channels) / 4 * p.mid.height;
  p.mid_grid = image_grid(p.mid.width, p.mid.height);
  if (hinv) {  // S Hinv S^-1 with S = diag(sx, sy, 1), the pixel scaling of the mid camera (see the ABI header)
    const double sx = (double)p.mid.width / (double)tgt.width, sy = (double)p.mid.height / (double)tgt.height;
    p.hinv[1] = p.hinv[1] * sx / sy;
    p.hinv[2] = p.hinv[2] * sx;
    p.hinv[3] = p.hinv[3] * sy / sx;
    p.hinv[5] = p.hinv[5] * sy;
    p.hinv[6] = p.hinv[6] / sx;
    p.hinv[7] = p.hinv[7] / sy;
  }
  return p;
}

inline void check_interpolation(const undistort_options& o) {
  UD_CHECK(o.interpolation == UNDISTORT_BILINEAR || o.interpolation == UNDISTORT_NEAREST,
           "Invalid warp image interpolation mode: " + std::to_string(o.interpolation));
}

// what undistort_images and undistort_rectify_images check before their first image or pair
inline void check_batch(const undistort_options* o, int32_t n, const void* items) {
  UD_CHECK(o && (n == 0 || items) && n >= 0, "null argument");
  check_options(*o);
  check_interpolation(*o);
}

inline void check_pixels(const undistort_image& im, const std::string& who) {
  UD_CHECK(im.data && im.out, who + "null pixel buffer");
  UD_CHECK(im.channels == 1 || im.channels == 3, who + "channels must be 1 (grey) or 3 (RGB)");
}

inline void check_capacity(const undistort_image& im, const undistort_cam& tgt, const std::string& who) {
  const size_t need = (size_t)tgt.width * tgt.height * im.channels;
  UD_CHECK(im.out_capacity >= need, who + "output buffer of " + std::to_string(im.out_capacity) + " bytes, " +
                                        std::to_string(need) + " needed");
}

// image i of undistort_images (image/undistortion.cc:266-301)
inline ImagePlan plan_image(const undistort_options& o, const undistort_image& im, int i) {
  const std::string who = "image " + std::to_string(i) + ": ";
  check_camera(im.camera);
  check_pixels(im, who);
  const undistort_cam& src = im.camera;
  undistort_cam tgt;
  if (ud::is_spherical(src.model_id)) {  // :274-290
    tgt = src;
    rescale_to_max_image_size(o, &tgt);
  } else {
    undistort_camera_impl(o, src, &tgt);
  }
  check_capacity(im, tgt, who);
  Route route = tgt.width == src.width && tgt.height == src.height ? kClone : kResize;
  if (!ud::is_spherical(src.model_id)) route = should_warp_directly(src, tgt, o.direct_warp_min_scale) ? kDirect : kIndirect;
  return make_plan(route, src, tgt, im.channels, o.interpolation, nullptr);
}

// what the two images of pair i of undistort_rectify_images share (image/undistortion.cc:447-490)
struct PairPlan {
  undistort_cam target;  // from camera 1 only (:462)
  double Hinv[2][9];     // the inverses of H1 and H2 of RectifyStereoCameras of the target with itself (:475-476)
  double Q[16];
};

inline PairPlan plan_pair(const undistort_options& o, const undistort_stereo_pair& pr, int i) {
  const std::string who = "pair " + std::to_string(i) + ": ";
  const undistort_image* im[2] = {&pr.image1, &pr.image2};
  for (int s = 0; s < 2; ++s) {
    check_camera(im[s]->camera);
    UD_CHECK(ud::is_perspective(im[s]->camera.model_id), who + "Check failed: camera.IsPerspective()");
    check_pixels(*im[s], who);
  }
  PairPlan pp;
  undistort_camera_impl(o, pr.image1.camera, &pp.target);
  double H1[9], H2[9];
  rectify_cameras_impl(pp.target, pp.target, pr.R, pr.t, H1, H2, pp.Q);
  UD_CHECK(mat3_inverse(H1, pp.Hinv[0]) && mat3_inverse(H2, pp.Hinv[1]), who + "a rectifying homography is singular");
  for (int s = 0; s < 2; ++s) check_capacity(*im[s], pp.target, who);
  return pp;
}

// side s (0 = image1, 1 = image2) of a planned pair
inline ImagePlan plan_pair_side(const undistort_options& o, const PairPlan& pp, const undistort_image& im, int s) {
  const Route route = should_warp_directly(im.camera, pp.target, o.direct_warp_min_scale) ? kDirect : kIndirect;
  return make_plan(route, im.camera, pp.target, im.channels, o.interpolation, pp.Hinv[s]);
}

// undistort_warp_homography: the direct path only
inline ImagePlan plan_warp_homography(const undistort_options* o, const double* Hinv, const undistort_cam* target_camera,
                                      const undistort_image* image) {
  UD_CHECK(o && Hinv && target_camera && image, "null argument");
  check_interpolation(*o);
  check_camera(image->camera);
  check_camera(*target_camera);
  UD_CHECK(ud::is_perspective(image->camera.model_id), "Check failed: camera.IsPerspective()");
  UD_CHECK(target_camera->model_id == ud::PINHOLE, "the warp target is a PINHOLE camera");
  check_pixels(*image, "");
  check_capacity(*image, *target_camera, "");
  return make_plan(kDirect, image->camera, *target_camera, image->channels, o->interpolation, Hinv);
}

// undistort_resize: the cameras of the plan carry the two sizes and nothing else
inline ImagePlan plan_resize(const uint8_t* src, int32_t src_width, int32_t src_height, int32_t channels, const uint8_t* dst,
                             int32_t dst_width, int32_t dst_height) {
  UD_CHECK(src && dst, "null argument");
  UD_CHECK(src_width > 0 && src_height > 0 && dst_width > 0 && dst_height > 0, "image sizes must be positive");
  UD_CHECK(channels == 1 || channels == 3, "channels must be 1 (grey) or 3 (RGB)");
  undistort_cam s = {}, t = {};
  s.width = src_width;
  s.height = src_height;
  t.width = dst_width;
  t.height = dst_height;
  return make_plan(kResize, s, t, channels, 0, nullptr);
}

}  // namespace undistort_plan
#endif  // COLMAP_AMD_UNDISTORT_PLAN_H_
