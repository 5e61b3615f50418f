// camera_projection.h -- the projections of the camera models, once, for host and device: image undistortion
// (undistort.hip) and observation filtering (obs_filter.hip) both read it. What a model IS (id, parameters, family)
// comes from include/colmap_amd/camera_models.hpp.
//
// Restates, for the 17 perspective models and EQUIRECTANGULAR (reference src/colmap/sensor/models.h):
//   Distortion(extra, u, v) -> (du, dv)       the additive distortion of each model, in the reference's order of
//                                             operations, together with its ANALYTIC Jacobian d(du, dv) / d(u, v)
//                                             (the reference differentiates with ceres::Jet, models.h:1157-1174)
//   img_from_normalized()                     ImgFromCam(u, v, w = 1) with the validity rules of each model
//   img_from_cam()                            ImgFromCam(u, v, w) with each model's own validity / cheirality rule
//   cam_ray_from_img()                        CamRayFromImg: the unit bearing of a pixel (the whole sphere for
//                                             EQUIRECTANGULAR)
//   cam_from_img()                            CamFromImg: closed forms where the reference has them (pinholes, FOV,
//                                             division models, SIMPLE_FISHEYE / FISHEYE, EUCM), IterativeUndistortion
//                                             (models.h:1141-1197) for the rest
// A `false` return is the reference's empty std::optional.
//
// Everything is double; the build has -ffp-contract=off, so an expression rounds the same on the host and on gfx950.
// What may differ between the two is libm (atan, tan, sin, cos): see DESIGN.md section 1.9 for the parity rule.
#ifndef COLMAP_AMD_CAMERA_PROJECTION_H_
#define COLMAP_AMD_CAMERA_PROJECTION_H_

#include <math.h>

#include "../../include/colmap_amd/camera_models.hpp"  // after the HIP header: its functions are host/device here

#define CAM_HD __host__ __device__ __forceinline__

namespace camera {

using namespace colmap_amd::camera_models;  // the ids, kMaxParams, num_params, the predicates, intrinsics

constexpr double kEps = 2.220446049250313e-16;  // std::numeric_limits<double>::epsilon()
constexpr double kPi = 3.141592653589793238462643383279502884;

// FisheyeFromNormal / NormalFromFisheye (models.h:429-451)
CAM_HD void fisheye_from_normal(double u, double v, double* uu, double* vv) {
  *uu = u;
  *vv = v;
  const double r = sqrt(u * u + v * v);
  if (r > kEps) {
    const double theta = atan(r);
    *uu *= theta / r;
    *vv *= theta / r;
  }
}
CAM_HD void normal_from_fisheye(double uu, double vv, double* u, double* v) {
  *u = uu;
  *v = vv;
  const double theta = sqrt(uu * uu + vv * vv);
  const double theta_cos_theta = theta * cos(theta);
  if (theta_cos_theta > kEps) {
    const double scale = sin(theta) / theta_cos_theta;
    *u *= scale;
    *v *= scale;
  }
}

// radial polynomial + tangential + thin-prism family:
//   du = u * rad + 2 t1 u v + t2 (r2 + 2 u^2) + sx r2,   dv = v * rad + 2 t2 u v + t1 (r2 + 2 v^2) + sy r2
// with rad = rad(r2), drad = d rad / d r2. J = d(du, dv) / d(u, v), row-major.
CAM_HD void family_jacobian(double u, double v, double rad, double drad, double t1, double t2, double sx, double sy,
                            double* J) {
  J[0] = rad + 2.0 * u * u * drad + 2.0 * t1 * v + 6.0 * t2 * u + 2.0 * sx * u;
  J[1] = 2.0 * u * v * drad + 2.0 * t1 * u + 2.0 * t2 * v + 2.0 * sx * v;
  J[2] = 2.0 * u * v * drad + 2.0 * t2 * v + 2.0 * t1 * u + 2.0 * sy * u;
  J[3] = rad + 2.0 * v * v * drad + 2.0 * t2 * u + 6.0 * t1 * v + 2.0 * sy * v;
}

// CameraModel::Distortion of the models that have an additive one; e = extra parameters. J may be null. For the
// fisheye models (u, v) are the equidistant coordinates. Operation order of the values as in the reference.
CAM_HD void distortion(int m, const double* e, double u, double v, double* du, double* dv, double* J) {
  const double u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
  switch (m) {
    case SIMPLE_RADIAL: case SIMPLE_RADIAL_FISHEYE: {  // models.h:1392-1403, 2013-2022
      const double radial = e[0] * r2;
      *du = u * radial;
      *dv = v * radial;
      if (J) family_jacobian(u, v, radial, e[0], 0, 0, 0, 0, J);
      return;
    }
    case RADIAL: {  // :1474-1486
      const double radial = e[0] * r2 + e[1] * r2 * r2;
      *du = u * radial;
      *dv = v * radial;
      if (J) family_jacobian(u, v, radial, e[0] + 2.0 * e[1] * r2, 0, 0, 0, 0, J);
      return;
    }
    case RADIAL_FISHEYE: {  // :2106-2117
      const double r4 = r2 * r2;
      const double radial = e[0] * r2 + e[1] * r4;
      *du = u * radial;
      *dv = v * radial;
      if (J) family_jacobian(u, v, radial, e[0] + 2.0 * e[1] * r2, 0, 0, 0, 0, J);
      return;
    }
    case OPENCV: {  // :1559-1574
      const double radial = e[0] * r2 + e[1] * r2 * r2;
      *du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2);
      *dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2);
      if (J) family_jacobian(u, v, radial, e[0] + 2.0 * e[1] * r2, e[2], e[3], 0, 0, J);
      return;
    }
    case OPENCV_FISHEYE: {  // :1660-1675
      const double t4 = r2 * r2, t6 = t4 * r2, t8 = t4 * t4;
      const double radial = e[0] * r2 + e[1] * t4 + e[2] * t6 + e[3] * t8;
      *du = u * radial;
      *dv = v * radial;
      if (J) family_jacobian(u, v, radial, e[0] + 2.0 * e[1] * r2 + 3.0 * e[2] * t4 + 4.0 * e[3] * t6, 0, 0, 0, 0, J);
      return;
    }
    case FULL_OPENCV: {  // :1759-1781; k1 k2 p1 p2 k3 k4 k5 k6
      const double r4 = r2 * r2, r6 = r4 * r2;
      const double num = 1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6;
      const double den = 1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6;
      const double radial = num / den;
      *du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u;
      *dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v;
      if (J) {
        const double dnum = e[0] + 2.0 * e[1] * r2 + 3.0 * e[4] * r4;
        const double dden = e[5] + 2.0 * e[6] * r2 + 3.0 * e[7] * r4;
        family_jacobian(u, v, radial - 1.0, (dnum * den - num * dden) / (den * den), e[2], e[3], 0, 0, J);
      }
      return;
    }
    case THIN_PRISM_FISHEYE: {  // :2215-2237; k1 k2 p1 p2 k3 k4 sx1 sy1
      const double r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2;
      const double radial = e[0] * r2 + e[1] * r4 + e[4] * r6 + e[5] * r8;
      *du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) + e[6] * r2;
      *dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) + e[7] * r2;
      if (J)
        family_jacobian(u, v, radial, e[0] + 2.0 * e[1] * r2 + 3.0 * e[4] * r4 + 4.0 * e[5] * r6, e[2], e[3], e[6], e[7], J);
      return;
    }
    case RAD_TAN_THIN_PRISM_FISHEYE: {  // :2332-2378; k0..k5 p0 p1 s0 s1 s2 s3
      double th = 1.0, dth = 0.0, pw = 1.0;
      for (int i = 0; i < 6; ++i) {
        dth += (i + 1) * e[i] * pw;
        pw *= r2;
        th += e[i] * pw;
      }
      const double x = th * u, y = th * v;
      const double x2 = x * x, y2 = y * y, xy = x * y, q2 = x2 + y2, q4 = q2 * q2;
      const double p0 = e[6], p1 = e[7], s0 = e[8], s1 = e[9], s2 = e[10], s3 = e[11];
      const double dx_tang = 2.0 * p1 * xy + p0 * (q2 + 2.0 * x2);
      const double dy_tang = 2.0 * p0 * xy + p1 * (q2 + 2.0 * y2);
      const double dx_tp = s0 * q2 + s1 * q4;
      const double dy_tp = s2 * q2 + s3 * q4;
      *du = x + dx_tang + dx_tp - u;
      *dv = y + dy_tang + dy_tp - v;
      if (J) {
        // (x, y) by (u, v)
        const double a00 = th + 2.0 * u2 * dth, a01 = 2.0 * uv * dth, a10 = a01, a11 = th + 2.0 * v2 * dth;
        // (X, Y) by (x, y)
        const double b00 = 1.0 + 2.0 * p1 * y + 6.0 * p0 * x + 2.0 * s0 * x + 4.0 * s1 * q2 * x;
        const double b01 = 2.0 * p1 * x + 2.0 * p0 * y + 2.0 * s0 * y + 4.0 * s1 * q2 * y;
        const double b10 = 2.0 * p0 * y + 2.0 * p1 * x + 2.0 * s2 * x + 4.0 * s3 * q2 * x;
        const double b11 = 1.0 + 2.0 * p0 * x + 6.0 * p1 * y + 2.0 * s2 * y + 4.0 * s3 * q2 * y;
        J[0] = b00 * a00 + b01 * a10 - 1.0;
        J[1] = b00 * a01 + b01 * a11;
        J[2] = b10 * a00 + b11 * a10;
        J[3] = b10 * a01 + b11 * a11 - 1.0;
      }
      return;
    }
    default:  // no additive distortion
      *du = 0.0;
      *dv = 0.0;
      if (J) J[0] = J[1] = J[2] = J[3] = 0.0;
  }
}

// FOVCameraModel::Distortion / Undistortion (models.h:1852-1926): multiplicative, (u, v) -> (u, v) * factor
CAM_HD double fov_distortion_factor(double omega, double radius2) {
  const double kEpsilon = 1e-4;
  const double omega2 = omega * omega;
  if (omega2 < kEpsilon) return (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
  if (radius2 < kEpsilon) {
    const double t = tan(omega / 2.0);
    return (-2.0 * t * (4.0 * radius2 * t * t - 3.0)) / (3.0 * omega);
  }
  const double radius = sqrt(radius2);
  return atan(radius * 2.0 * tan(omega / 2.0)) / (radius * omega);
}
CAM_HD double fov_undistortion_factor(double omega, double radius2) {
  const double kEpsilon = 1e-4;
  const double omega2 = omega * omega;
  if (omega2 < kEpsilon) return (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
  if (radius2 < kEpsilon) return (omega * (omega * omega * radius2 + 3.0)) / (6.0 * tan(omega / 2.0));
  const double radius = sqrt(radius2);
  return tan(radius * omega) / (radius * 2.0 * tan(omega / 2.0));
}

// CameraModel::ImgFromCam(u, v, w = 1, check_cheirality = true): w = 1 always has a projectable depth.
CAM_HD bool img_from_normalized(int m, const double* p, double u, double v, double* x, double* y) {
  if (m == EQUIRECTANGULAR) {  // models.h:2852-2877 at (u, v, 1): never the zero vector
    const double horizontal = sqrt(u * u + 1.0);
    *x = (atan2(u, 1.0) / (2.0 * kPi) + 0.5) * p[0];
    *y = (0.5 - atan2(-v, horizontal) / kPi) * p[1];
    return true;
  }
  const Intrinsics k = intrinsics(m, p);
  switch (m) {
    case SIMPLE_PINHOLE: case PINHOLE:  // :1223-1246, 1284-1308
      *x = k.f1 * u + k.c1;
      *y = k.f2 * v + k.c2;
      return true;
    case SIMPLE_DIVISION: case DIVISION: {  // :2405-2436, 2494-2526
      const double rho = sqrt(u * u + v * v);
      const double disc_sq = 1.0 - 4.0 * rho * rho * k.extra[0];
      if (disc_sq < 0.0) return false;
      const double r = 2.0 / (1.0 + sqrt(disc_sq));
      *x = k.f1 * r * u + k.c1;
      *y = k.f2 * r * v + k.c2;
      return true;
    }
    case EUCM: {  // :2757-2794
      const double alpha = k.extra[0], beta = k.extra[1];
      const double rho2 = beta * (u * u + v * v) + 1.0;
      if (rho2 < 0.0) return false;
      const double den = alpha * sqrt(rho2) + (1.0 - alpha);
      if (!(den >= kEps)) return false;
      *x = k.f1 * (u / den) + k.c1;
      *y = k.f2 * (v / den) + k.c2;
      return true;
    }
    case FOV: {  // :1808-1833
      const double factor = fov_distortion_factor(k.extra[0], u * u + v * v);
      *x = k.f1 * (u * factor) + k.c1;
      *y = k.f2 * (v * factor) + k.c2;
      return true;
    }
    default: {
      double uu = u, vv = v;
      if (is_fisheye(m)) fisheye_from_normal(u, v, &uu, &vv);
      double du, dv;
      distortion(m, k.extra, uu, vv, &du, &dv, nullptr);
      *x = k.f1 * (uu + du) + k.c1;
      *y = k.f2 * (vv + dv) + k.c2;
      return true;
    }
  }
}

// BasePerspectiveCameraModel::IterativeUndistortion (models.h:1141-1197): Newton on x + Distortion(x) = x0 with a trust
// region, 100 iterations, done when the squared step is below 1e-10. The 2x2 system is solved by elimination with
// partial pivoting (Eigen's partialPivLu).
CAM_HD bool iterative_undistortion(int m, const double* e, double* u, double* v) {
  const double x0 = *u, y0 = *v;
  double x = x0, y = y0;
  for (int it = 0; it < 100; ++it) {
    double du, dv, J[4];
    distortion(m, e, x, y, &du, &dv, J);
    double a = J[0] + 1.0, b = J[1], c = J[2], d = J[3] + 1.0;
    double r0 = x + du - x0, r1 = y + dv - y0;
    if (fabs(c) > fabs(a)) {  // row swap
      double t;
      t = a; a = c; c = t;
      t = b; b = d; d = t;
      t = r0; r0 = r1; r1 = t;
    }
    const double l = c / a;
    double sy = (r1 - l * r0) / (d - l * b);
    double sx = (r0 - b * sy) / a;
    const double radius_sqr = fmax((x * x + y * y) * 0.1 * 0.1, 0.1 * 0.1);
    const double step_sqr = sx * sx + sy * sy;
    if (step_sqr > radius_sqr) {
      const double s = sqrt(radius_sqr / step_sqr);
      sx *= s;
      sy *= s;
    }
    x -= sx;
    y -= sy;
    if (sx * sx + sy * sy < 1e-10) {
      *u = x;
      *v = y;
      return true;
    }
  }
  *u = x;
  *v = y;
  return false;
}

// CameraModel::CamFromImg
CAM_HD bool cam_from_img(int m, const double* p, double x, double y, double* u, double* v) {
  if (m == EQUIRECTANGULAR) {  // models.h:2883-2903: forward hemisphere only
    const double theta = 2.0 * kPi * (x / p[0] - 0.5);
    const double phi = kPi * (0.5 - y / p[1]);
    const double cos_phi = cos(phi);
    const double rz = cos_phi * cos(theta);
    if (rz <= kEps) return false;
    *u = cos_phi * sin(theta) / rz;
    *v = -sin(phi) / rz;
    return true;
  }
  const Intrinsics k = intrinsics(m, p);
  const double xn = (x - k.c1) / k.f1, yn = (y - k.c2) / k.f2;
  switch (m) {
    case SIMPLE_PINHOLE: case PINHOLE:  // :1248-1258, 1310-1321
      *u = xn;
      *v = yn;
      return true;
    case SIMPLE_DIVISION: case DIVISION: {  // :2438-2456, 2528-2547
      const double denom = 1.0 + k.extra[0] * (xn * xn + yn * yn);
      *u = xn / denom;
      *v = yn / denom;
      return true;
    }
    case FOV: {  // :1835-1850
      const double factor = fov_undistortion_factor(k.extra[0], xn * xn + yn * yn);
      *u = xn * factor;
      *v = yn * factor;
      return true;
    }
    case SIMPLE_FISHEYE: case FISHEYE:  // :2630-2637, 2710-2717
      normal_from_fisheye(xn, yn, u, v);
      return true;
    case EUCM: {  // :2796-2832
      const double alpha = k.extra[0], beta = k.extra[1];
      const double r2 = xn * xn + yn * yn;
      const double gamma = 1.0 - alpha;
      const double radicand = 1.0 - (alpha - gamma) * beta * r2;
      if (radicand < 0.0) return false;
      const double helper_den = alpha * sqrt(radicand) + gamma;
      if (helper_den < kEps) return false;
      const double helper = (1.0 - alpha * alpha * beta * r2) / helper_den;
      if (helper < kEps) return false;
      *u = xn / helper;
      *v = yn / helper;
      return true;
    }
    default: {
      double uu = xn, vv = yn;
      if (!iterative_undistortion(m, k.extra, &uu, &vv)) return false;
      if (is_fisheye(m)) {
        normal_from_fisheye(uu, vv, u, v);
      } else {
        *u = uu;
        *v = vv;
      }
      return true;
    }
  }
}

// CameraModel::ImgFromCam(u, v, w, check_cheirality = true) with each model's own validity rule:
//   the division models take any depth (models.h:2405-2436, 2494-2526: the quadratic is solved with w itself),
//   EUCM wants w >= epsilon AND its denominator >= epsilon (:2757-2794),
//   EQUIRECTANGULAR takes every direction but the zero vector (:2852-2877),
//   every other model wants HasProjectableDepth(w) = w >= epsilon (:281-285) and then projects (u / w, v / w).
CAM_HD bool img_from_cam(int m, const double* p, double u, double v, double w, double* x, double* y) {
  if (m == EQUIRECTANGULAR) {
    const double horizontal = sqrt(u * u + w * w);
    if (horizontal + fabs(v) < kEps) return false;
    *x = (atan2(u, w) / (2.0 * kPi) + 0.5) * p[0];
    *y = (0.5 - atan2(-v, horizontal) / kPi) * p[1];
    return true;
  }
  if (m == SIMPLE_DIVISION || m == DIVISION) {
    const Intrinsics k = intrinsics(m, p);
    const double rho = sqrt(u * u + v * v);
    const double disc_sq = w * w - 4.0 * rho * rho * k.extra[0];
    if (disc_sq < 0.0) return false;
    const double r = 2.0 / (w + sqrt(disc_sq));
    *x = k.f1 * r * u + k.c1;
    *y = k.f2 * r * v + k.c2;
    return true;
  }
  if (!(w >= kEps)) return false;
  if (m == EUCM) {
    const Intrinsics k = intrinsics(m, p);
    const double alpha = k.extra[0], beta = k.extra[1];
    const double rho2 = beta * (u * u + v * v) + w * w;
    if (rho2 < 0.0) return false;
    const double den = alpha * sqrt(rho2) + (1.0 - alpha) * w;
    if (!(den >= kEps)) return false;
    *x = k.f1 * (u / den) + k.c1;
    *y = k.f2 * (v / den) + k.c2;
    return true;
  }
  return img_from_normalized(m, p, u / w, v / w, x, y);
}

// CameraModel::CamRayFromImg: the unit bearing of a pixel. EQUIRECTANGULAR covers the whole sphere and always has a
// value (models.h:813-828); every other model normalises (CamFromImg, 1) (:353-369).
CAM_HD bool cam_ray_from_img(int m, const double* p, double x, double y, double* rx, double* ry, double* rz) {
  if (m == EQUIRECTANGULAR) {
    const double theta = 2.0 * kPi * (x / p[0] - 0.5);
    const double phi = kPi * (0.5 - y / p[1]);
    const double cos_phi = cos(phi);
    *rx = cos_phi * sin(theta);
    *ry = -sin(phi);
    *rz = cos_phi * cos(theta);
    return true;
  }
  double u, v;
  if (!cam_from_img(m, p, x, y, &u, &v)) return false;
  const double norm = sqrt(u * u + v * v + 1.0);
  *rx = u / norm;
  *ry = v / norm;
  *rz = 1.0 / norm;
  return true;
}

}  // namespace camera
#undef CAM_HD
#endif  // COLMAP_AMD_CAMERA_PROJECTION_H_
