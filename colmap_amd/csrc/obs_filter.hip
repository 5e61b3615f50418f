// obs_filter.hip -- observation and point filtering of a sparse model on gfx950 behind include/colmap_amd_obs.h.
//
// Three kernels, all geometry in double:
//   obs_image_kernel      one lane per image: rotation matrix of cam_from_world and the projection centre -R^T t
//                         (Image::ProjectionCenter), once, for the two passes below.
//   obs_eval_kernel       Pass A, one lane per observation: X_cam = R X + t, the negative-depth flag
//                         (HasPointPositiveDepth, scene/projection.cc:137-141) and the observation error of the
//                         requested ReprojectionErrorType (sfm/observation_manager.cc:523-563). Lane t takes observation
//                         eval_order[t] of the host plan, which is sorted by camera model: a wave takes one branch of
//                         the model switch even when the model mixes lenses.
//   obs_point_kernel<G>   Pass B, one point per group of G lanes (G = 1, 16 or 64 by track length, obs_plan.h): reads
//                         Pass A's values in track order and decides.
//
// The reference deletes as it walks; a point only ever looks at its own track, so every rule has a closed form per
// point with track length L (err_j the error of observation j, in track order):
//   large error (observation_manager.cc:496-585)
//       L < 2                      -> point deleted, L observations filtered
//       marked = #{j: err_j > max}; marked >= L - 1 -> point deleted, L filtered
//       otherwise the marked observations go (the loop of DeleteObservation calls never meets a track of length <= 2,
//       because marked < L - 1 leaves at least 2), marked filtered, error = (sum of the unmarked err_j, in track
//       order) / (L - marked)
//   small triangulation angle (:435-494), on the track the error rule left
//       kept iff some pair of its images has min(angle, pi - angle) >= min_tri_angle; otherwise the point is deleted
//       and its remaining observations are filtered. The pair order of the reference only decides WHICH pair is found
//       first, not whether one exists.
//   short track (:395-407)         L < min_track_len -> point deleted, L filtered
//   negative depth (:409-433)      k = #{j: image not spherical and depth_j < DBL_EPSILON}. The reference deletes these
//       one at a time through DeleteObservation (:311-326), which deletes the whole point instead when the track has
//       length <= 2 at that moment -- and then the other observations of the point are gone before the loop reaches
//       them. After i deletions the track has L - i elements, so deletion number i + 1 takes the point when
//       L - i <= 2, i.e. from deletion number max(L - 1, 1) on. Hence: the point dies iff k >= max(L - 1, 1), and the
//       loop counted min(k, max(L - 1, 1)) observations -- not k. (L = 3, k = 3: two are counted, the second one
//       takes the point.) Which of the negative observations come first does not matter for either number.
//   point errors (scene/reconstruction.cc:959-975)   error = (sum of err_j in track order) / L, 0 for L = 0
// The sums run in track order in every lane of the group (the values are a broadcast load), so an error is the same
// double the sequential loop produces from the same err_j, and the same on every run. Counts are integers per point;
// the host adds them in point order (obs_plan::sum_counts). There is no atomic anywhere.
//
// The pair loop is O(L^2): lane g of the group takes i1 = g, g + G, ... and walks i2 < i1; a lane stops at its first
// good pair, a whole wave stops when any lane has one (__any), and the group's verdict is one __ballot.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_obs.h"
#include "camera_projection.h"
#include "obs_plan.h"

#define OBS_API __attribute__((visibility("default")))

namespace {

namespace ud = camera;

thread_local std::string g_error;
thread_local double g_kernel_ms = 0.0, g_total_ms = 0.0;

using Fail = obs_plan::Fail;
#define OBS_HIP(call)                                                                    \
  do {                                                                                   \
    const hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess) throw Fail(std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <typename F>
int Guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

enum Mode : int { MODE_FILTER = 0, MODE_SHORT = 1, MODE_DEPTH = 2, MODE_ERRORS = 3 };

constexpr int kImageStride = 16;  // doubles per image: R (9, row-major), t (3), projection centre (3), unused (1)
constexpr int kBlock = 256;
constexpr double kDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;  // DegToRad, math/math.h
constexpr double kRadToDeg = 57.29577951308232286464772187173366546630859375;                // RadToDeg

struct DevCamera {
  int model, width;
  double p[ud::kMaxParams];
};

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void obs_image_kernel(const double* __restrict__ poses, int num_images,
                                                            double* __restrict__ imgs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_images) return;
  const double* q = poses + (size_t)7 * i;
  const double x = q[0], y = q[1], z = q[2], w = q[3], tx = q[4], ty = q[5], tz = q[6];
  double* o = imgs + (size_t)kImageStride * i;
  const double r00 = 1.0 - 2.0 * (y * y + z * z), r01 = 2.0 * (x * y - z * w), r02 = 2.0 * (x * z + y * w);
  const double r10 = 2.0 * (x * y + z * w), r11 = 1.0 - 2.0 * (x * x + z * z), r12 = 2.0 * (y * z - x * w);
  const double r20 = 2.0 * (x * z - y * w), r21 = 2.0 * (y * z + x * w), r22 = 1.0 - 2.0 * (x * x + y * y);
  o[0] = r00; o[1] = r01; o[2] = r02;
  o[3] = r10; o[4] = r11; o[5] = r12;
  o[6] = r20; o[7] = r21; o[8] = r22;
  o[9] = tx; o[10] = ty; o[11] = tz;
  o[12] = -(r00 * tx + r10 * ty + r20 * tz);  // -R^T t
  o[13] = -(r01 * tx + r11 * ty + r21 * tz);
  o[14] = -(r02 * tx + r12 * ty + r22 * tz);
  o[15] = 0.0;
}

// CalculateAngularReprojectionError (scene/projection.cc:93-135) in radians; pi when the pixel has no ray.
__device__ __forceinline__ double angular_error(int m, const double* p, double x, double y, const double pc[3]) {
  double rx, ry, rz;
  if (!ud::cam_ray_from_img(m, p, x, y, &rx, &ry, &rz)) return ud::kPi;
  double nx = pc[0], ny = pc[1], nz = pc[2];
  const double n2 = nx * nx + ny * ny + nz * nz;
  if (n2 > 0.0) {  // Eigen's normalized() leaves the zero vector alone
    const double n = sqrt(n2);
    nx /= n;
    ny /= n;
    nz /= n;
  }
  const double c = rx * nx + ry * ny + rz * nz;
  return acos(fmin(fmax(c, -1.0), 1.0));
}

// the observation error of FilterPoints3DWithLargeReprojectionError (sfm/observation_manager.cc:523-563)
__device__ __forceinline__ double observation_error(int type, int m, const double* p, int width, double x, double y,
                                                    const double pc[3]) {
  if (type == OBS_ERROR_PIXEL) {  // sqrt(CalculateSquaredReprojectionError), scene/projection.cc:40-91
    if (ud::is_spherical(m)) {
      const double pixels_per_radian = (double)width / (2.0 * ud::kPi);
      const double pixel_error = angular_error(m, p, x, y, pc) * pixels_per_radian;
      return sqrt(pixel_error * pixel_error);
    }
    double px, py;
    if (!ud::img_from_cam(m, p, pc[0], pc[1], pc[2], &px, &py)) return sqrt(DBL_MAX);
    const double dx = px - x, dy = py - y;
    return sqrt(dx * dx + dy * dy);
  }
  if (type == OBS_ERROR_NORMALIZED) {  // :532-557
    const double inf = __builtin_huge_val();
    if (ud::is_perspective(m)) {
      double u, v;
      const bool has = ud::cam_from_img(m, p, x, y, &u, &v);
      if (!(pc[2] >= 1e-12 && has)) return inf;
      const double du = pc[0] / pc[2] - u, dv = pc[1] / pc[2] - v;
      return sqrt(du * du + dv * dv);
    }
    double rx, ry, rz;
    if (!ud::cam_ray_from_img(m, p, x, y, &rx, &ry, &rz)) return inf;
    double nx = pc[0], ny = pc[1], nz = pc[2];
    const double n2 = nx * nx + ny * ny + nz * nz;
    if (n2 > 0.0) {
      const double n = sqrt(n2);
      nx /= n;
      ny /= n;
      nz /= n;
    }
    const double dx = nx - rx, dy = ny - ry, dz = nz - rz;
    return sqrt(dx * dx + dy * dy + dz * dz);
  }
  return angular_error(m, p, x, y, pc) * kRadToDeg;  // ANGULAR, in degrees
}

__global__ __launch_bounds__(kBlock) void obs_eval_kernel(const DevCamera* __restrict__ cams,
                                                           const double* __restrict__ imgs,
                                                           const int* __restrict__ image_camera,
                                                           const double* __restrict__ points,
                                                           const int* __restrict__ obs_image,
                                                           const int* __restrict__ obs_point,
                                                           const double* __restrict__ obs_xy,
                                                           const int* __restrict__ eval_order, int num_obs,
                                                           int error_type, double* __restrict__ obs_err,
                                                           uint8_t* __restrict__ obs_negative) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= num_obs) return;
  const int o = eval_order[t];
  const int img = obs_image[o];
  const double* M = imgs + (size_t)kImageStride * img;
  const double* X = points + (size_t)3 * obs_point[o];
  const DevCamera* cam = cams + image_camera[img];
  const int m = cam->model;
  double pc[3];
  pc[0] = M[0] * X[0] + M[1] * X[1] + M[2] * X[2] + M[9];
  pc[1] = M[3] * X[0] + M[4] * X[1] + M[5] * X[2] + M[10];
  pc[2] = M[6] * X[0] + M[7] * X[1] + M[8] * X[2] + M[11];  // cam_from_world.row(2) . [X; 1]
  obs_negative[o] = (!ud::is_spherical(m) && !(pc[2] >= ud::kEps)) ? 1 : 0;
  obs_err[o] = observation_error(error_type, m, cam->p, cam->width, obs_xy[2 * (size_t)o], obs_xy[2 * (size_t)o + 1], pc);
}

struct PointArgs {
  const long long* obs_offsets;
  const int* obs_image;
  const double* imgs;
  const double* points;
  const double* obs_err;
  const uint8_t* obs_negative;
  uint8_t* obs_keep;
  uint8_t* point_status;
  double* point_error;
  unsigned* point_count;
  int mode, rules, min_track_len;
  double max_error, min_tri_angle_rad;
};

// CalculateTriangulationAngle (geometry/triangulation.cc:217-249) of the rays X - c1, X - c2
__device__ __forceinline__ double triangulation_angle(const double v1[3], const double v2[3]) {
  const double n1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
  const double n2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  double angle = 0.0;
  if (!(n1 == 0.0 || n2 == 0.0)) {
    const double c = (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) / sqrt(n1 * n2);
    angle = acos(fmin(fmax(c, -1.0), 1.0));
  }
  return fmin(angle, ud::kPi - angle);
}

// true in every lane of a group of G lanes iff `pred` holds in one of them. Every lane of the wave calls it.
template <int G>
__device__ __forceinline__ bool group_any(bool pred) {
  if (G == 1) return pred;
  const unsigned long long b = __ballot(pred ? 1 : 0);
  if (G == 64) return b != 0ull;
  const int lane = threadIdx.x & 63;
  return ((b >> (lane & ~(G - 1))) & ((1ull << (G & 63)) - 1ull)) != 0ull;
}

template <int G>
__global__ __launch_bounds__(kBlock) void obs_point_kernel(PointArgs a, const int* __restrict__ class_points,
                                                            int num_class_points) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int group = tid / G, gl = tid % G;
  // no lane leaves before the group vote below: a wave holds 64 / G groups, and the vote is wave-wide
  const bool valid = group < num_class_points;
  const int p = valid ? class_points[group] : 0;
  const long long begin = valid ? a.obs_offsets[p] : 0;
  const int L = valid ? (int)(a.obs_offsets[p + 1] - begin) : 0;
  const bool use_err = a.mode == MODE_FILTER && (a.rules & OBS_RULE_REPROJ_ERROR);

  int status = OBS_POINT_KEPT;
  unsigned count = 0u;
  double error = -1.0;
  int marked = 0;  // observations the rule takes out of a track that stays
  if (a.mode == MODE_FILTER) {
    if (use_err) {
      double sum = 0.0;
      for (int j = 0; j < L; ++j) {
        const double e = a.obs_err[begin + j];
        if (e > a.max_error) ++marked; else sum += e;
      }
      if (L < 2 || marked >= L - 1) {
        status = OBS_POINT_DELETED_ERROR;
        count = (unsigned)L;
      } else {
        count = (unsigned)marked;
        error = sum / (double)(L - marked);
      }
    }
  } else if (a.mode == MODE_SHORT) {
    if (L < a.min_track_len) {
      status = OBS_POINT_DELETED_SHORT;
      count = (unsigned)L;
    }
  } else if (a.mode == MODE_DEPTH) {
    for (int j = 0; j < L; ++j) marked += a.obs_negative[begin + j];
    const int limit = L - 1 > 1 ? L - 1 : 1;
    if (marked >= limit) {
      status = OBS_POINT_DELETED_DEPTH;
      count = (unsigned)limit;
    } else {
      count = (unsigned)marked;
    }
  } else {  // MODE_ERRORS
    double sum = 0.0;
    for (int j = 0; j < L; ++j) sum += a.obs_err[begin + j];
    error = L == 0 ? 0.0 : sum / (double)L;
  }

  // triangulation angles of the surviving track
  const bool search = valid && a.mode == MODE_FILTER && (a.rules & OBS_RULE_TRI_ANGLE) && status == OBS_POINT_KEPT;
  bool found = false;
  {
    const double* X = a.points + (size_t)3 * p;
    // G = 64: the group is the wave, `search` and L are uniform and the wave leaves together at the first good pair.
    // G < 64: groups of one wave have different L; each lane walks its own pairs and the vote comes after the loop.
    const int Ls = search ? L : 0;
    for (int base = 0; base < Ls; base += G) {
      const int i1 = base + gl;
      if (i1 < Ls && !found && !(use_err && a.obs_err[begin + i1] > a.max_error)) {
        const double* c1 = a.imgs + (size_t)kImageStride * a.obs_image[begin + i1] + 12;
        const double v1[3] = {X[0] - c1[0], X[1] - c1[1], X[2] - c1[2]};
        for (int i2 = 0; i2 < i1; ++i2) {
          if (use_err && a.obs_err[begin + i2] > a.max_error) continue;
          const double* c2 = a.imgs + (size_t)kImageStride * a.obs_image[begin + i2] + 12;
          const double v2[3] = {X[0] - c2[0], X[1] - c2[1], X[2] - c2[2]};
          if (triangulation_angle(v1, v2) >= a.min_tri_angle_rad) {
            found = true;
            break;
          }
        }
      }
      if (G == 64) {
        if (__any(found ? 1 : 0)) break;
      } else if (found) {
        break;
      }
    }
  }
  const bool any_found = group_any<G>(found);
  if (!valid) return;
  if (search && !any_found) {
    status = OBS_POINT_DELETED_ANGLE;
    count += (unsigned)(L - marked);
  }

  const bool point_deleted = status != OBS_POINT_KEPT;
  for (int j = gl; j < L; j += G) {
    bool keep = !point_deleted;
    if (keep && use_err) keep = !(a.obs_err[begin + j] > a.max_error);
    if (keep && a.mode == MODE_DEPTH) keep = a.obs_negative[begin + j] == 0;
    a.obs_keep[begin + j] = keep ? 1 : 0;
  }
  if (gl == 0) {
    a.point_status[p] = (uint8_t)status;
    a.point_error[p] = point_deleted ? -1.0 : error;
    a.point_count[p] = count;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

void bind_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Fail("no HIP device available: observation filtering runs on the GPU (there is no CPU path)");
  if (!(gpu_index >= 0 && gpu_index < ndev)) throw Fail("gpu_index " + std::to_string(gpu_index) + " out of range");
  OBS_HIP(hipSetDevice(gpu_index));
}

template <typename T>
struct DeviceBuffer {
  T* p = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  void alloc(size_t n) {
    if (n == 0) return;
    OBS_HIP(hipMalloc((void**)&p, n * sizeof(T)));
  }
  void upload(const T* host, size_t n) {
    alloc(n);
    if (n) OBS_HIP(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
  }
  void download(T* host, size_t n) const {
    if (n && host) OBS_HIP(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost));
  }
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  Timer() {
    OBS_HIP(hipEventCreate(&a));
    OBS_HIP(hipEventCreate(&b));
  }
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

void run(Mode mode, const obs_model* model, const obs_filter_options* options, obs_result* result, int gpu_index) {
  if (!model || !options || !result) throw Fail("null argument");
  const obs_filter_options& opt = *options;
  if (mode == MODE_FILTER) {
    OBS_CHECK(opt.error_type == OBS_ERROR_PIXEL || opt.error_type == OBS_ERROR_NORMALIZED || opt.error_type == OBS_ERROR_ANGULAR,
              "unknown error_type " + std::to_string(opt.error_type));
    OBS_CHECK(opt.rules != 0 && (opt.rules & ~(OBS_RULE_REPROJ_ERROR | OBS_RULE_TRI_ANGLE)) == 0,
              "rules must be a combination of OBS_RULE_REPROJ_ERROR and OBS_RULE_TRI_ANGLE");
  }
  if (mode == MODE_SHORT) OBS_CHECK(opt.min_track_len >= 0, "min_track_len must not be negative");
  obs_plan::validate(*model);
  const obs_model& m = *model;
  bind_device(gpu_index);
  const auto t0 = std::chrono::steady_clock::now();

  const bool need_eval = mode != MODE_SHORT;
  const bool need_images = need_eval || mode == MODE_FILTER;
  const obs_plan::Plan plan = obs_plan::make_plan(m, need_eval);
  const size_t P = (size_t)m.num_points, O = (size_t)m.num_observations, I = (size_t)m.num_images;

  std::vector<DevCamera> cams((size_t)m.num_cameras);
  for (size_t c = 0; c < cams.size(); ++c) {
    cams[c].model = m.cameras[c].model_id;
    cams[c].width = m.cameras[c].width;
    for (int k = 0; k < ud::kMaxParams; ++k) cams[c].p[k] = k < m.cameras[c].num_params ? m.cameras[c].params[k] : 0.0;
  }

  DeviceBuffer<DevCamera> d_cams;
  DeviceBuffer<double> d_poses, d_imgs, d_points, d_xy, d_err, d_error;
  DeviceBuffer<int> d_image_camera, d_obs_image, d_obs_point, d_order, d_class[obs_plan::kNumClasses];
  DeviceBuffer<long long> d_off;
  DeviceBuffer<uint8_t> d_neg, d_keep, d_status;
  DeviceBuffer<unsigned> d_count;
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are uploaded as they are");
  d_off.upload((const long long*)m.obs_offsets, P + 1);
  d_obs_image.upload(m.obs_image, O);
  d_points.upload(m.points, 3 * P);
  if (need_images) {
    d_poses.upload(m.image_poses, 7 * I);
    d_imgs.alloc((size_t)kImageStride * I);
  }
  if (need_eval) {
    d_cams.upload(cams.data(), cams.size());
    d_image_camera.upload(m.image_camera, I);
    d_obs_point.upload(plan.obs_point.data(), O);
    d_order.upload(plan.eval_order.data(), O);
    d_xy.upload(m.obs_xy, 2 * O);
    d_err.alloc(O);
    d_neg.alloc(O);
  }
  for (int k = 0; k < obs_plan::kNumClasses; ++k) d_class[k].upload(plan.class_points[k].data(), plan.class_points[k].size());
  d_keep.alloc(O);
  d_status.alloc(P);
  d_error.alloc(P);
  d_count.alloc(P);

  Timer ev;
  OBS_HIP(hipEventRecord(ev.a, 0));
  if (need_images && I > 0) {
    hipLaunchKernelGGL(obs_image_kernel, dim3(blocks_for(I)), dim3(kBlock), 0, 0, d_poses.p, (int)I, d_imgs.p);
    OBS_HIP(hipGetLastError());
  }
  if (need_eval && O > 0) {
    const int error_type = mode == MODE_FILTER ? opt.error_type : OBS_ERROR_PIXEL;
    hipLaunchKernelGGL(obs_eval_kernel, dim3(blocks_for(O)), dim3(kBlock), 0, 0, d_cams.p, d_imgs.p, d_image_camera.p,
                       d_points.p, d_obs_image.p, d_obs_point.p, d_xy.p, d_order.p, (int)O, error_type, d_err.p, d_neg.p);
    OBS_HIP(hipGetLastError());
  }
  PointArgs a;
  a.obs_offsets = d_off.p;
  a.obs_image = d_obs_image.p;
  a.imgs = d_imgs.p;
  a.points = d_points.p;
  a.obs_err = d_err.p;
  a.obs_negative = d_neg.p;
  a.obs_keep = d_keep.p;
  a.point_status = d_status.p;
  a.point_error = d_error.p;
  a.point_count = d_count.p;
  a.mode = mode;
  a.rules = mode == MODE_FILTER ? opt.rules : 0;
  a.min_track_len = opt.min_track_len;
  a.max_error = opt.max_reproj_error;
  a.min_tri_angle_rad = opt.min_tri_angle * kDegToRad;
  for (int k = 0; k < obs_plan::kNumClasses; ++k) {
    const size_t n = plan.class_points[k].size();
    if (n == 0) continue;
    const dim3 grid(blocks_for(n * (size_t)obs_plan::kClassWidth[k])), block(kBlock);
    if (k == 0) hipLaunchKernelGGL((obs_point_kernel<1>), grid, block, 0, 0, a, d_class[k].p, (int)n);
    else if (k == 1) hipLaunchKernelGGL((obs_point_kernel<16>), grid, block, 0, 0, a, d_class[k].p, (int)n);
    else hipLaunchKernelGGL((obs_point_kernel<64>), grid, block, 0, 0, a, d_class[k].p, (int)n);
    OBS_HIP(hipGetLastError());
  }
  OBS_HIP(hipEventRecord(ev.b, 0));
  OBS_HIP(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  OBS_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));

  std::vector<unsigned> counts(P);
  d_count.download(counts.data(), P);
  d_keep.download(result->obs_keep, O);
  d_status.download(result->point_status, P);
  d_error.download(result->point_error, P);
  if (result->point_count) std::memcpy(result->point_count, counts.data(), P * sizeof(unsigned));
  result->num_filtered = obs_plan::sum_counts(counts.data(), (int64_t)P);
  g_kernel_ms = ms;
  g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

OBS_API void obs_filter_options_init(obs_filter_options* o) {
  o->max_reproj_error = 4.0;
  o->min_tri_angle = 1.5;
  o->min_track_len = 2;
  o->error_type = OBS_ERROR_PIXEL;
  o->rules = OBS_RULE_REPROJ_ERROR | OBS_RULE_TRI_ANGLE;
  o->reserved = 0;
}

OBS_API int obs_filter_all_points3D(const obs_model* model, const obs_filter_options* options, obs_result* result,
                                    int32_t gpu_index) {
  return Guard([&] { run(MODE_FILTER, model, options, result, gpu_index); });
}

OBS_API int obs_filter_short_tracks(const obs_model* model, const obs_filter_options* options, obs_result* result,
                                    int32_t gpu_index) {
  return Guard([&] { run(MODE_SHORT, model, options, result, gpu_index); });
}

OBS_API int obs_filter_negative_depth(const obs_model* model, obs_result* result, int32_t gpu_index) {
  return Guard([&] {
    obs_filter_options o;
    obs_filter_options_init(&o);
    run(MODE_DEPTH, model, &o, result, gpu_index);
  });
}

OBS_API int obs_point_errors(const obs_model* model, obs_result* result, int32_t gpu_index) {
  return Guard([&] {
    obs_filter_options o;
    obs_filter_options_init(&o);
    run(MODE_ERRORS, model, &o, result, gpu_index);
  });
}

OBS_API void obs_last_timing(double* kernel_ms, double* total_ms) {
  if (kernel_ms) *kernel_ms = g_kernel_ms;
  if (total_ms) *total_ms = g_total_ms;
}

OBS_API const char* obs_last_error(void) { return g_error.c_str(); }

}  // extern "C"
