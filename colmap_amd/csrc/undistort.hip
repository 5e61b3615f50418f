// undistort.hip -- image undistortion on gfx950 behind include/colmap_amd_undistort.h.
//
// Four kernels, all geometry in double:
//   undistort_warp_kernel<INTERP, C>   one target pixel = target pinhole CamFromImg -> source ImgFromCam -> sample
//                                      (reference image/warp.cc:91-144, sensor/bitmap.cc InterpolateBilinear /
//                                      InterpolateNearestNeighbor). The source model is a kernel argument, uniform over
//                                      the launch: the kernel branches on it ONCE and runs a pixel loop compiled for
//                                      that model. Lanes run along the output row, each lane owns 4 adjacent pixels and
//                                      stores them as whole dwords (1 for grey, 3 for RGB) into a device image whose row
//                                      pitch is padded to whole groups. Source texels are read through the caches:
//                                      neighbouring lanes read neighbouring texels, nothing is staged in LDS.
//   undistort_rectify_kernel<INTERP, C> the same work shape with a homography in front of the target camera: one target
//                                      pixel = Hinv (x + 1/2, y + 1/2, 1) -> target pinhole CamFromImg -> source
//                                      ImgFromCam -> sample (image/warp.cc:196-250), for stereo rectification
//   undistort_points_kernel            one lane per observation (image/undistortion.cc:334-381)
//   undistort_resize_kernel<C>         the triangle filter defined at the kernel (indirect path of
//                                      WarpImageBetweenCameras, and spherical images with max_image_size)
// undistort_camera / undistort_cam_from_img / undistort_rectify_cameras are host functions over the same camera_projection.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_undistort.h"
#include "camera_projection.h"

#define UNDISTORT_API __attribute__((visibility("default")))

namespace {

namespace ud = camera;

thread_local std::string g_error;
thread_local double g_kernel_ms = 0.0, g_total_ms = 0.0;

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};
#define UD_CHECK(cond, msg) \
  do {                      \
    if (!(cond)) throw Fail(msg); \
  } while (0)
#define UD_HIP(call)                                                                                   \
  do {                                                                                                 \
    const hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) throw Fail(std::string(#call) + ": " + hipGetErrorString(e_));              \
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

struct CamArgs {  // a camera as kernel argument (scalar registers)
  int model, width, height, pad;
  double p[ud::kMaxParams];
};

CamArgs to_args(const undistort_cam& c) {
  CamArgs a;
  a.model = c.model_id;
  a.width = c.width;
  a.height = c.height;
  a.pad = 0;
  for (int i = 0; i < ud::kMaxParams; ++i) a.p[i] = c.params[i];
  return a;
}

void check_camera(const undistort_cam& c) {
  UD_CHECK(ud::num_params(c.model_id) > 0, "unknown camera model id " + std::to_string(c.model_id));
  UD_CHECK(c.width > 0 && c.height > 0, "camera width and height must be positive");
}

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

constexpr int kPixelsPerLane = 4;

// BitmapColor<float>::Cast<uint8_t> (sensor/bitmap.h:216-223) of a double-valued interpolant that the reference first
// narrows to float (sensor/bitmap.cc InterpolateBilinear returns BitmapColor<float>)
__device__ __forceinline__ unsigned to_u8(double value) {
  const float r = roundf((float)value);
  return (unsigned)fminf(255.0f, fmaxf(0.0f, r));
}

// Bitmap::InterpolateBilinear / InterpolateNearestNeighbor at (x, y) in pixel-index coordinates; false = out of range.
template <int INTERP, int C>
__device__ __forceinline__ bool sample(const uint8_t* __restrict__ src, int pitch, int W, int H, double x, double y,
                                       unsigned* out) {
  if (INTERP == UNDISTORT_NEAREST) {
    const double xr = round(x), yr = round(y);
    if (!(xr >= 0.0 && xr <= (double)(W - 1) && yr >= 0.0 && yr <= (double)(H - 1))) return false;
    const uint8_t* px = src + (size_t)(int)yr * pitch + (int)xr * C;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = px[c];
    return true;
  }
  const double xf = floor(x), yf = floor(y);
  // x0 < 0 || x1 >= W || y0 < 0 || y1 >= H, written so that NaN and values beyond int fail too
  if (!(xf >= 0.0 && xf + 1.0 <= (double)(W - 1) && yf >= 0.0 && yf + 1.0 <= (double)(H - 1))) return false;
  const int x0 = (int)xf, y0 = (int)yf;
  const double dx = x - xf, dy = y - yf, dx_1 = 1.0 - dx, dy_1 = 1.0 - dy;
  const uint8_t* line0 = src + (size_t)y0 * pitch + x0 * C;
  const uint8_t* line1 = line0 + pitch;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double v0 = dx_1 * line0[c] + dx * line0[C + c];
    const double v1 = dx_1 * line1[c] + dx * line1[C + c];
    out[c] = to_u8(dy_1 * v0 + dy * v1);
  }
  return true;
}

template <int MODEL, int INTERP, int C>
__device__ __forceinline__ void warp_group(const CamArgs& src, double tfx, double tfy, double tcx, double tcy,
                                           const uint8_t* __restrict__ in, int in_pitch, uint32_t* __restrict__ out,
                                           int out_pitch_dwords, int W, int H) {
  const int gx = (blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerLane;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (gx >= W || y >= H) return;
  const double v = ((double)y + 0.5 - tcy) / tfy;  // PinholeCameraModel::CamFromImg of the target
  unsigned px[kPixelsPerLane * C];
#pragma unroll
  for (int k = 0; k < kPixelsPerLane; ++k) {
    unsigned* o = px + k * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0u;
    const int x = gx + k;
    if (x >= W) continue;
    const double u = ((double)x + 0.5 - tcx) / tfx;
    double sx, sy;
    if (!ud::img_from_normalized(MODEL, src.p, u, v, &sx, &sy)) continue;
    unsigned s[C];
    if (sample<INTERP, C>(in, in_pitch, src.width, src.height, sx - 0.5, sy - 0.5, s)) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = s[c];
    }
  }
  // kPixelsPerLane * C bytes = C dwords, little endian
  uint32_t* dst = out + (size_t)y * out_pitch_dwords + (size_t)(gx / kPixelsPerLane) * C;
#pragma unroll
  for (int d = 0; d < C; ++d)
    dst[d] = px[4 * d] | (px[4 * d + 1] << 8) | (px[4 * d + 2] << 16) | (px[4 * d + 3] << 24);
}

template <int INTERP, int C>
__global__ void __launch_bounds__(256)
undistort_warp_kernel(CamArgs src, double tfx, double tfy, double tcx, double tcy, const uint8_t* __restrict__ in,
                      int in_pitch, uint32_t* __restrict__ out, int out_pitch_dwords, int W, int H) {
#define UD_CASE(M)                                                                                        \
  case ud::M:                                                                                             \
    warp_group<ud::M, INTERP, C>(src, tfx, tfy, tcx, tcy, in, in_pitch, out, out_pitch_dwords, W, H); \
    break;
  switch (src.model) {  // uniform over the launch
    UD_CASE(SIMPLE_PINHOLE) UD_CASE(PINHOLE) UD_CASE(SIMPLE_RADIAL) UD_CASE(RADIAL) UD_CASE(OPENCV)
    UD_CASE(OPENCV_FISHEYE) UD_CASE(FULL_OPENCV) UD_CASE(FOV) UD_CASE(SIMPLE_RADIAL_FISHEYE) UD_CASE(RADIAL_FISHEYE)
    UD_CASE(THIN_PRISM_FISHEYE) UD_CASE(RAD_TAN_THIN_PRISM_FISHEYE) UD_CASE(SIMPLE_DIVISION) UD_CASE(DIVISION)
    UD_CASE(SIMPLE_FISHEYE) UD_CASE(FISHEYE) UD_CASE(EUCM)
    default: break;  // the host never launches a spherical source
  }
#undef UD_CASE
}

// ---- stereo rectification (undistort_rectify_kernel, WarpImageWithHomographyBetweenCameras image/warp.cc:196-250) ----
struct Homography {  // row-major 3x3, the inverse of H1 / H2 of RectifyStereoCameras: target pixel -> unrectified target pixel
  double h[9];
};

// warp_group with a homography in front of the target camera (image/warp.cc:214-245): w = Hinv (x + 1/2, y + 1/2, 1); a
// pixel with w.z == 0 is 0; otherwise the target pinhole CamFromImg of w.hnormalized(), the source ImgFromCam, the sample.
template <int MODEL, int INTERP, int C>
__device__ __forceinline__ void rectify_group(const CamArgs& src, const Homography& Hinv, double tfx, double tfy,
                                              double tcx, double tcy, const uint8_t* __restrict__ in, int in_pitch,
                                              uint32_t* __restrict__ out, int out_pitch_dwords, int W, int H) {
  const int gx = (blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerLane;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (gx >= W || y >= H) return;
  const double py = (double)y + 0.5;
  unsigned px[kPixelsPerLane * C];
#pragma unroll
  for (int k = 0; k < kPixelsPerLane; ++k) {
    unsigned* o = px + k * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0u;
    const int x = gx + k;
    if (x >= W) continue;
    const double pxc = (double)x + 0.5;
    const double wx = Hinv.h[0] * pxc + Hinv.h[1] * py + Hinv.h[2];
    const double wy = Hinv.h[3] * pxc + Hinv.h[4] * py + Hinv.h[5];
    const double wz = Hinv.h[6] * pxc + Hinv.h[7] * py + Hinv.h[8];
    if (wz == 0.0) continue;
    const double u = (wx / wz - tcx) / tfx;  // PinholeCameraModel::CamFromImg of the target
    const double v = (wy / wz - tcy) / tfy;
    double sx, sy;
    if (!ud::img_from_normalized(MODEL, src.p, u, v, &sx, &sy)) continue;
    unsigned s[C];
    if (sample<INTERP, C>(in, in_pitch, src.width, src.height, sx - 0.5, sy - 0.5, s)) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = s[c];
    }
  }
  uint32_t* dst = out + (size_t)y * out_pitch_dwords + (size_t)(gx / kPixelsPerLane) * C;
#pragma unroll
  for (int d = 0; d < C; ++d)
    dst[d] = px[4 * d] | (px[4 * d + 1] << 8) | (px[4 * d + 2] << 16) | (px[4 * d + 3] << 24);
}

template <int INTERP, int C>
__global__ void __launch_bounds__(256)
undistort_rectify_kernel(CamArgs src, Homography Hinv, double tfx, double tfy, double tcx, double tcy,
                         const uint8_t* __restrict__ in, int in_pitch, uint32_t* __restrict__ out, int out_pitch_dwords,
                         int W, int H) {
#define UD_CASE(M)                                                                                             \
  case ud::M:                                                                                                  \
    rectify_group<ud::M, INTERP, C>(src, Hinv, tfx, tfy, tcx, tcy, in, in_pitch, out, out_pitch_dwords, W, H); \
    break;
  switch (src.model) {  // uniform over the launch
    UD_CASE(SIMPLE_PINHOLE) UD_CASE(PINHOLE) UD_CASE(SIMPLE_RADIAL) UD_CASE(RADIAL) UD_CASE(OPENCV)
    UD_CASE(OPENCV_FISHEYE) UD_CASE(FULL_OPENCV) UD_CASE(FOV) UD_CASE(SIMPLE_RADIAL_FISHEYE) UD_CASE(RADIAL_FISHEYE)
    UD_CASE(THIN_PRISM_FISHEYE) UD_CASE(RAD_TAN_THIN_PRISM_FISHEYE) UD_CASE(SIMPLE_DIVISION) UD_CASE(DIVISION)
    UD_CASE(SIMPLE_FISHEYE) UD_CASE(FISHEYE) UD_CASE(EUCM)
    default: break;  // the host never launches a spherical source
  }
#undef UD_CASE
}

__global__ void __launch_bounds__(256)
undistort_points_kernel(CamArgs distorted, CamArgs undistorted, double* __restrict__ xy, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double x = xy[2 * i], y = xy[2 * i + 1];
  if (ud::is_spherical(distorted.model)) {  // image/undistortion.cc:343-359
    x *= (double)undistorted.width / (double)distorted.width;
    y *= (double)undistorted.height / (double)distorted.height;
  } else {
    double u, v;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (!ud::cam_from_img(distorted.model, distorted.p, x, y, &u, &v) ||
        !ud::img_from_normalized(undistorted.model, undistorted.p, u, v, &x, &y))
      x = y = nan;
  }
  xy[2 * i] = x;
  xy[2 * i + 1] = y;
}

// ---- the resize filter (undistort_resize_kernel, the indirect path of WarpImageBetweenCameras) ----
// The reference shrinks with OpenImageIO's default filter, which is not restated here. This library shrinks with an
// antialiased separable triangle filter: per axis with s = source size / target size and support r = max(s, 1), target
// pixel i has its centre at c = (i + 0.5) * s in source coordinates and takes source pixel j (centre j + 0.5) with weight
// w(j) = max(0, 1 - |j + 0.5 - c| / r) for j = floor(c - r) .. ceil(c + r), restricted to 0 <= j < source size. The value
// is sum_y wy * (sum_x wx * p(x, y)) divided by (sum_x wx) * (sum_y wy) over the taken pixels (so that a border pixel is
// a weighted mean of what exists), summed in that order in double, then cast to float, rounded and clamped to [0, 255]
// like every other pixel (sensor/bitmap.h:216-223). At s = 1 it is the identity; for s <= 1 it is bilinear interpolation.
//
// one axis of the filter: taps [j0, j1], weight of tap j, for target index i
struct Taps {
  int j0, j1;
  double c, r;
  __device__ __forceinline__ double weight(int j) const { return fmax(0.0, 1.0 - fabs((double)j + 0.5 - c) / r); }
};
__device__ __forceinline__ Taps make_taps(int i, int src_size, int dst_size) {
  const double s = (double)src_size / (double)dst_size;
  Taps t;
  t.r = fmax(s, 1.0);
  t.c = ((double)i + 0.5) * s;
  t.j0 = max((int)floor(t.c - t.r), 0);
  t.j1 = min((int)ceil(t.c + t.r), src_size - 1);
  return t;
}

template <int C>
__global__ void __launch_bounds__(256)
undistort_resize_kernel(const uint8_t* __restrict__ src, int src_pitch, int SW, int SH, uint32_t* __restrict__ out,
                        int out_pitch_dwords, int W, int H) {
  const int gx = (blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerLane;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (gx >= W || y >= H) return;
  const Taps ty = make_taps(y, SH, H);
  double wy_sum = 0.0;
  for (int j = ty.j0; j <= ty.j1; ++j) wy_sum += ty.weight(j);
  unsigned px[kPixelsPerLane * C];
#pragma unroll
  for (int k = 0; k < kPixelsPerLane; ++k) {
    unsigned* o = px + k * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0u;
    const int x = gx + k;
    if (x >= W) continue;
    const Taps tx = make_taps(x, SW, W);
    double wx_sum = 0.0;
    for (int j = tx.j0; j <= tx.j1; ++j) wx_sum += tx.weight(j);
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int jy = ty.j0; jy <= ty.j1; ++jy) {
      const uint8_t* line = src + (size_t)jy * src_pitch;
      double row[C];
#pragma unroll
      for (int c = 0; c < C; ++c) row[c] = 0.0;
      for (int jx = tx.j0; jx <= tx.j1; ++jx) {
        const double w = tx.weight(jx);
#pragma unroll
        for (int c = 0; c < C; ++c) row[c] += w * line[jx * C + c];
      }
      const double wy = ty.weight(jy);
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += wy * row[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = to_u8(acc[c] / (wx_sum * wy_sum));
  }
  uint32_t* dst = out + (size_t)y * out_pitch_dwords + (size_t)(gx / kPixelsPerLane) * C;
#pragma unroll
  for (int d = 0; d < C; ++d)
    dst[d] = px[4 * d] | (px[4 * d + 1] << 8) | (px[4 * d + 2] << 16) | (px[4 * d + 3] << 24);
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

void bind_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Fail("no HIP device available: image undistortion runs on the GPU (there is no CPU path)");
  UD_CHECK(gpu_index >= 0 && gpu_index < ndev, "gpu_index " + std::to_string(gpu_index) + " out of range");
  UD_HIP(hipSetDevice(gpu_index));
}

template <typename T>
struct DeviceBuffer {  // grows, never shrinks, freed with its owner
  T* p = nullptr;
  size_t cap = 0;
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    UD_HIP(hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
  }
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  Timer() {
    UD_HIP(hipEventCreate(&a));
    UD_HIP(hipEventCreate(&b));
  }
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// a device image of W x H x C bytes whose rows hold whole 4-pixel groups
inline int padded_pitch(int W, int C) { return (W + kPixelsPerLane - 1) / kPixelsPerLane * kPixelsPerLane * C; }

inline dim3 image_grid(int W, int H, dim3 block) {
  return dim3(((W + kPixelsPerLane - 1) / kPixelsPerLane + block.x - 1) / block.x, (H + block.y - 1) / block.y);
}

void launch_warp(const undistort_cam& source, const undistort_cam& target, int interpolation, int channels,
                 const uint8_t* d_in, uint32_t* d_out) {
  UD_CHECK(target.model_id == ud::PINHOLE, "the warp target is a PINHOLE camera");
  const CamArgs src = to_args(source);
  const int W = target.width, H = target.height;
  const int in_pitch = source.width * channels, out_pitch = padded_pitch(W, channels) / 4;
  const dim3 block(64, 4);
  const dim3 grid = image_grid(W, H, block);
  const double fx = target.params[0], fy = target.params[1], cx = target.params[2], cy = target.params[3];
#define UD_LAUNCH(I, C) \
  hipLaunchKernelGGL((undistort_warp_kernel<I, C>), grid, block, 0, 0, src, fx, fy, cx, cy, d_in, in_pitch, d_out, out_pitch, W, H)
  if (interpolation == UNDISTORT_BILINEAR) {
    if (channels == 1) UD_LAUNCH(UNDISTORT_BILINEAR, 1); else UD_LAUNCH(UNDISTORT_BILINEAR, 3);
  } else {
    if (channels == 1) UD_LAUNCH(UNDISTORT_NEAREST, 1); else UD_LAUNCH(UNDISTORT_NEAREST, 3);
  }
#undef UD_LAUNCH
  UD_HIP(hipGetLastError());
}

void launch_rectify(const undistort_cam& source, const undistort_cam& target, const Homography& Hinv, int interpolation,
                    int channels, const uint8_t* d_in, uint32_t* d_out) {
  UD_CHECK(target.model_id == ud::PINHOLE, "the warp target is a PINHOLE camera");
  const CamArgs src = to_args(source);
  const int W = target.width, H = target.height;
  const int in_pitch = source.width * channels, out_pitch = padded_pitch(W, channels) / 4;
  const dim3 block(64, 4);
  const dim3 grid = image_grid(W, H, block);
  const double fx = target.params[0], fy = target.params[1], cx = target.params[2], cy = target.params[3];
#define UD_LAUNCH(I, C)                                                                                             \
  hipLaunchKernelGGL((undistort_rectify_kernel<I, C>), grid, block, 0, 0, src, Hinv, fx, fy, cx, cy, d_in, in_pitch, \
                     d_out, out_pitch, W, H)
  if (interpolation == UNDISTORT_BILINEAR) {
    if (channels == 1) UD_LAUNCH(UNDISTORT_BILINEAR, 1); else UD_LAUNCH(UNDISTORT_BILINEAR, 3);
  } else {
    if (channels == 1) UD_LAUNCH(UNDISTORT_NEAREST, 1); else UD_LAUNCH(UNDISTORT_NEAREST, 3);
  }
#undef UD_LAUNCH
  UD_HIP(hipGetLastError());
}

void launch_resize(const uint8_t* d_src, int src_pitch, int SW, int SH, int channels, uint32_t* d_out, int W, int H) {
  const dim3 block(64, 4);
  const dim3 grid = image_grid(W, H, block);
  const int out_pitch = padded_pitch(W, channels) / 4;
  if (channels == 1)
    hipLaunchKernelGGL((undistort_resize_kernel<1>), grid, block, 0, 0, d_src, src_pitch, SW, SH, d_out, out_pitch, W, H);
  else
    hipLaunchKernelGGL((undistort_resize_kernel<3>), grid, block, 0, 0, d_src, src_pitch, SW, SH, d_out, out_pitch, W, H);
  UD_HIP(hipGetLastError());
}

void download(uint8_t* host, const uint32_t* d_img, int W, int H, int C) {
  UD_HIP(hipMemcpy2DAsync(host, (size_t)W * C, d_img, (size_t)padded_pitch(W, C), (size_t)W * C, (size_t)H,
                          hipMemcpyDeviceToHost, 0));
  UD_HIP(hipStreamSynchronize(0));
}

void check_options(const undistort_options& o) {  // image/undistortion.cc:60-70
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
void rescale_camera(undistort_cam* c, int new_width, int new_height) {
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
void rescale_to_max_image_size(const undistort_options& o, undistort_cam* c) {
  if (o.max_image_size < 0) return;
  const double scale = std::min(o.max_image_size / (double)c->width, o.max_image_size / (double)c->height);
  if (scale < 1.0)
    rescale_camera(c, (int)std::round(scale * c->width), (int)std::round(scale * c->height));
}

void undistort_camera_impl(const undistort_options& o, const undistort_cam& cam, undistort_cam* out) {
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

// ShouldWarpDirectly (image/warp.cc:72-89)
bool should_warp_directly(const undistort_cam& s, const undistort_cam& t, double direct_warp_min_scale) {
  UD_CHECK(direct_warp_min_scale >= 0, "Check failed: options.direct_warp_min_scale >= 0");
  if (t.width == s.width && t.height == s.height) return true;
  const double scale_x = (double)t.width / (double)s.width, scale_y = (double)t.height / (double)s.height;
  return std::min(scale_x, scale_y) >= direct_warp_min_scale;
}

// ---- RectifyStereoCameras (image/undistortion.cc:384-445), Eigen's operations restated on row-major 3x3 arrays ----
void mat3_mul(const double* a, const double* b, double* c) {
  double r[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
  std::memcpy(c, r, sizeof(r));
}

void mat3_vec(const double* a, const double* v, double* out) {
  double r[3];
  for (int i = 0; i < 3; ++i) r[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
  std::memcpy(out, r, sizeof(r));
}

// Eigen::AngleAxisd::toRotationMatrix
void rotation_from_angle_axis(double angle, const double* axis, double* m) {
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
void angle_axis_from_rotation(const double* m, double* angle, double* axis) {
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
bool mat3_inverse(const double* a, double* inv) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
  const double r[9] = {c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                       c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                       c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det};
  std::memcpy(inv, r, sizeof(r));
  return true;
}

void rectify_cameras_impl(const undistort_cam& cam1, const undistort_cam& cam2, const double* R, const double* t_in,
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

}  // namespace

extern "C" {

UNDISTORT_API void undistort_options_init(undistort_options* o) {
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

UNDISTORT_API int undistort_camera(const undistort_options* options, const undistort_cam* camera, undistort_cam* undistorted) {
  return Guard([&] {
    UD_CHECK(options && camera && undistorted, "null argument");
    undistort_camera_impl(*options, *camera, undistorted);
  });
}

UNDISTORT_API int undistort_cam_from_img(const undistort_cam* camera, const double* xy, int64_t n, double* uv) {
  return Guard([&] {
    UD_CHECK(camera && (n == 0 || (xy && uv)) && n >= 0, "null argument");
    check_camera(*camera);
    for (int64_t i = 0; i < n; ++i) {
      double u, v;
      if (!ud::cam_from_img(camera->model_id, camera->params, xy[2 * i], xy[2 * i + 1], &u, &v))
        u = v = std::numeric_limits<double>::quiet_NaN();
      uv[2 * i] = u;
      uv[2 * i + 1] = v;
    }
  });
}

UNDISTORT_API int undistort_images(const undistort_options* options, int32_t num_images, undistort_image* images,
                                   int32_t gpu_index) {
  return Guard([&] {
    UD_CHECK(options && (num_images == 0 || images) && num_images >= 0, "null argument");
    check_options(*options);
    UD_CHECK(options->interpolation == UNDISTORT_BILINEAR || options->interpolation == UNDISTORT_NEAREST,
             "Invalid warp image interpolation mode: " + std::to_string(options->interpolation));
    // everything the caller can get wrong is checked before the first byte moves
    std::vector<undistort_cam> targets(num_images);
    for (int i = 0; i < num_images; ++i) {
      undistort_image& im = images[i];
      check_camera(im.camera);
      UD_CHECK(im.data && im.out, "image " + std::to_string(i) + ": null pixel buffer");
      UD_CHECK(im.channels == 1 || im.channels == 3, "image " + std::to_string(i) + ": channels must be 1 (grey) or 3 (RGB)");
      if (ud::is_spherical(im.camera.model_id)) {  // image/undistortion.cc:274-290
        targets[i] = im.camera;
        rescale_to_max_image_size(*options, &targets[i]);
      } else {
        undistort_camera_impl(*options, im.camera, &targets[i]);
      }
      const size_t need = (size_t)targets[i].width * targets[i].height * im.channels;
      UD_CHECK(im.out_capacity >= need, "image " + std::to_string(i) + ": output buffer of " + std::to_string(im.out_capacity) +
                                            " bytes, " + std::to_string(need) + " needed");
    }
    bind_device(gpu_index);
    const auto t0 = std::chrono::steady_clock::now();
    DeviceBuffer<uint8_t> d_in;
    DeviceBuffer<uint32_t> d_out, d_mid;
    Timer ev;
    double kernel_ms = 0.0;
    for (int i = 0; i < num_images; ++i) {
      undistort_image& im = images[i];
      const undistort_cam& src = im.camera;
      const undistort_cam& tgt = targets[i];
      const int C = im.channels;
      const size_t in_bytes = (size_t)src.width * src.height * C;
      im.out_camera = tgt;
      if (ud::is_spherical(src.model_id) && tgt.width == src.width && tgt.height == src.height) {
        std::memcpy(im.out, im.data, in_bytes);  // Bitmap::Clone
        continue;
      }
      d_in.reserve(in_bytes);
      d_out.reserve((size_t)padded_pitch(tgt.width, C) / 4 * tgt.height);
      UD_HIP(hipMemcpyAsync(d_in.p, im.data, in_bytes, hipMemcpyHostToDevice, 0));
      UD_HIP(hipEventRecord(ev.a, 0));
      if (ud::is_spherical(src.model_id)) {
        launch_resize(d_in.p, src.width * C, src.width, src.height, C, d_out.p, tgt.width, tgt.height);
      } else if (should_warp_directly(src, tgt, options->direct_warp_min_scale)) {
        launch_warp(src, tgt, options->interpolation, C, d_in.p, d_out.p);
      } else {  // image/warp.cc:103-106, 141-143: warp at the source's resolution, then shrink
        undistort_cam mid = tgt;
        rescale_camera(&mid, src.width, src.height);
        d_mid.reserve((size_t)padded_pitch(mid.width, C) / 4 * mid.height);
        launch_warp(src, mid, options->interpolation, C, d_in.p, d_mid.p);
        launch_resize((const uint8_t*)d_mid.p, padded_pitch(mid.width, C), mid.width, mid.height, C, d_out.p, tgt.width,
                      tgt.height);
      }
      UD_HIP(hipEventRecord(ev.b, 0));
      download(im.out, d_out.p, tgt.width, tgt.height, C);
      UD_HIP(hipEventSynchronize(ev.b));
      float ms = 0.0f;
      UD_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
      kernel_ms += ms;
    }
    g_kernel_ms = kernel_ms;
    g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
}

UNDISTORT_API int undistort_rectify_cameras(const undistort_cam* camera1, const undistort_cam* camera2, const double* R,
                                            const double* t, double* H1, double* H2, double* Q) {
  return Guard([&] {
    UD_CHECK(camera1 && camera2 && R && t && H1 && H2 && Q, "null argument");
    rectify_cameras_impl(*camera1, *camera2, R, t, H1, H2, Q);
  });
}

UNDISTORT_API int undistort_rectify_images(const undistort_options* options, int32_t num_pairs, undistort_stereo_pair* pairs,
                                           int32_t gpu_index) {
  return Guard([&] {
    UD_CHECK(options && (num_pairs == 0 || pairs) && num_pairs >= 0, "null argument");
    check_options(*options);
    UD_CHECK(options->interpolation == UNDISTORT_BILINEAR || options->interpolation == UNDISTORT_NEAREST,
             "Invalid warp image interpolation mode: " + std::to_string(options->interpolation));
    // everything the caller can get wrong is checked before the first byte moves
    struct PairPlan {
      undistort_cam target;
      Homography Hinv[2];
    };
    std::vector<PairPlan> plans(num_pairs);
    for (int i = 0; i < num_pairs; ++i) {
      undistort_stereo_pair& pr = pairs[i];
      undistort_image* im[2] = {&pr.image1, &pr.image2};
      const std::string who = "pair " + std::to_string(i);
      for (int s = 0; s < 2; ++s) {
        check_camera(im[s]->camera);
        UD_CHECK(ud::is_perspective(im[s]->camera.model_id), who + ": Check failed: camera.IsPerspective()");
        UD_CHECK(im[s]->data && im[s]->out, who + ": null pixel buffer");
        UD_CHECK(im[s]->channels == 1 || im[s]->channels == 3, who + ": channels must be 1 (grey) or 3 (RGB)");
      }
      undistort_camera_impl(*options, pr.image1.camera, &plans[i].target);  // camera 1 only (:462, :475-476)
      double H1[9], H2[9];
      rectify_cameras_impl(plans[i].target, plans[i].target, pr.R, pr.t, H1, H2, pr.Q);
      UD_CHECK(mat3_inverse(H1, plans[i].Hinv[0].h) && mat3_inverse(H2, plans[i].Hinv[1].h),
               who + ": a rectifying homography is singular");
      for (int s = 0; s < 2; ++s) {
        const size_t need = (size_t)plans[i].target.width * plans[i].target.height * im[s]->channels;
        UD_CHECK(im[s]->out_capacity >= need, who + ": output buffer of " + std::to_string(im[s]->out_capacity) +
                                                  " bytes, " + std::to_string(need) + " needed");
      }
    }
    bind_device(gpu_index);
    const auto t0 = std::chrono::steady_clock::now();
    DeviceBuffer<uint8_t> d_in;
    DeviceBuffer<uint32_t> d_out, d_mid;
    Timer ev;
    double kernel_ms = 0.0;
    for (int i = 0; i < num_pairs; ++i) {
      undistort_image* im[2] = {&pairs[i].image1, &pairs[i].image2};
      const undistort_cam& tgt = plans[i].target;
      for (int s = 0; s < 2; ++s) {
        const undistort_cam& src = im[s]->camera;
        const int C = im[s]->channels;
        const size_t in_bytes = (size_t)src.width * src.height * C;
        im[s]->out_camera = tgt;
        d_in.reserve(in_bytes);
        d_out.reserve((size_t)padded_pitch(tgt.width, C) / 4 * tgt.height);
        UD_HIP(hipMemcpyAsync(d_in.p, im[s]->data, in_bytes, hipMemcpyHostToDevice, 0));
        UD_HIP(hipEventRecord(ev.a, 0));
        if (should_warp_directly(src, tgt, options->direct_warp_min_scale)) {
          launch_rectify(src, tgt, plans[i].Hinv[s], options->interpolation, C, d_in.p, d_out.p);
        } else {
          // The consistent indirect path (see the header): the target camera rescaled to the source's size
          // (image/warp.cc:103-106), the homography conjugated with that pixel scaling S = diag(sx, sy, 1) -- S Hinv S^-1,
          // which in front of the rescaled camera is Hinv diag(1/sx, 1/sy, 1) in front of the target camera --, the warp
          // at source size, then the shrink.
          undistort_cam mid = tgt;
          rescale_camera(&mid, src.width, src.height);
          const double sx = (double)mid.width / (double)tgt.width, sy = (double)mid.height / (double)tgt.height;
          Homography Hs = plans[i].Hinv[s];
          Hs.h[1] = Hs.h[1] * sx / sy;
          Hs.h[2] = Hs.h[2] * sx;
          Hs.h[3] = Hs.h[3] * sy / sx;
          Hs.h[5] = Hs.h[5] * sy;
          Hs.h[6] = Hs.h[6] / sx;
          Hs.h[7] = Hs.h[7] / sy;
          d_mid.reserve((size_t)padded_pitch(mid.width, C) / 4 * mid.height);
          launch_rectify(src, mid, Hs, options->interpolation, C, d_in.p, d_mid.p);
          launch_resize((const uint8_t*)d_mid.p, padded_pitch(mid.width, C), mid.width, mid.height, C, d_out.p, tgt.width,
                        tgt.height);
        }
        UD_HIP(hipEventRecord(ev.b, 0));
        download(im[s]->out, d_out.p, tgt.width, tgt.height, C);
        UD_HIP(hipEventSynchronize(ev.b));
        float ms = 0.0f;
        UD_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        kernel_ms += ms;
      }
    }
    g_kernel_ms = kernel_ms;
    g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
}

UNDISTORT_API int undistort_warp_homography(const undistort_options* options, const double* Hinv,
                                            const undistort_cam* target_camera, undistort_image* image, int32_t gpu_index) {
  return Guard([&] {
    UD_CHECK(options && Hinv && target_camera && image, "null argument");
    UD_CHECK(options->interpolation == UNDISTORT_BILINEAR || options->interpolation == UNDISTORT_NEAREST,
             "Invalid warp image interpolation mode: " + std::to_string(options->interpolation));
    check_camera(image->camera);
    check_camera(*target_camera);
    UD_CHECK(ud::is_perspective(image->camera.model_id), "Check failed: camera.IsPerspective()");
    UD_CHECK(target_camera->model_id == ud::PINHOLE, "the warp target is a PINHOLE camera");
    UD_CHECK(image->data && image->out, "null pixel buffer");
    UD_CHECK(image->channels == 1 || image->channels == 3, "channels must be 1 (grey) or 3 (RGB)");
    const undistort_cam& src = image->camera;
    const undistort_cam& tgt = *target_camera;
    const int C = image->channels;
    const size_t need = (size_t)tgt.width * tgt.height * C;
    UD_CHECK(image->out_capacity >= need, "output buffer of " + std::to_string(image->out_capacity) + " bytes, " +
                                              std::to_string(need) + " needed");
    bind_device(gpu_index);
    Homography H;
    for (int i = 0; i < 9; ++i) H.h[i] = Hinv[i];
    DeviceBuffer<uint8_t> d_in;
    DeviceBuffer<uint32_t> d_out;
    const size_t in_bytes = (size_t)src.width * src.height * C;
    d_in.reserve(in_bytes);
    d_out.reserve((size_t)padded_pitch(tgt.width, C) / 4 * tgt.height);
    UD_HIP(hipMemcpyAsync(d_in.p, image->data, in_bytes, hipMemcpyHostToDevice, 0));
    launch_rectify(src, tgt, H, options->interpolation, C, d_in.p, d_out.p);
    download(image->out, d_out.p, tgt.width, tgt.height, C);
    image->out_camera = tgt;
  });
}

UNDISTORT_API int undistort_points(const undistort_cam* distorted, const undistort_cam* undistorted, double* xy, int64_t n,
                                   int32_t gpu_index) {
  return Guard([&] {
    UD_CHECK(distorted && undistorted && (n == 0 || xy) && n >= 0, "null argument");
    check_camera(*distorted);
    check_camera(*undistorted);
    UD_CHECK(ud::is_spherical(distorted->model_id) == ud::is_spherical(undistorted->model_id),
             "a spherical camera stays spherical, a perspective one becomes perspective");
    bind_device(gpu_index);
    if (n == 0) return;
    DeviceBuffer<double> d_xy;
    d_xy.reserve((size_t)2 * n);
    UD_HIP(hipMemcpyAsync(d_xy.p, xy, (size_t)2 * n * sizeof(double), hipMemcpyHostToDevice, 0));
    hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, to_args(*distorted),
                       to_args(*undistorted), d_xy.p, (long long)n);
    UD_HIP(hipGetLastError());
    UD_HIP(hipMemcpyAsync(xy, d_xy.p, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, 0));
    UD_HIP(hipStreamSynchronize(0));
  });
}

UNDISTORT_API int undistort_resize(const uint8_t* src, int32_t src_width, int32_t src_height, int32_t channels, uint8_t* dst,
                                   int32_t dst_width, int32_t dst_height, int32_t gpu_index) {
  return Guard([&] {
    UD_CHECK(src && dst, "null argument");
    UD_CHECK(src_width > 0 && src_height > 0 && dst_width > 0 && dst_height > 0, "image sizes must be positive");
    UD_CHECK(channels == 1 || channels == 3, "channels must be 1 (grey) or 3 (RGB)");
    bind_device(gpu_index);
    DeviceBuffer<uint8_t> d_in;
    DeviceBuffer<uint32_t> d_out;
    const size_t in_bytes = (size_t)src_width * src_height * channels;
    d_in.reserve(in_bytes);
    d_out.reserve((size_t)padded_pitch(dst_width, channels) / 4 * dst_height);
    UD_HIP(hipMemcpyAsync(d_in.p, src, in_bytes, hipMemcpyHostToDevice, 0));
    launch_resize(d_in.p, src_width * channels, src_width, src_height, channels, d_out.p, dst_width, dst_height);
    download(dst, d_out.p, dst_width, dst_height, channels);
  });
}

UNDISTORT_API void undistort_last_timing(double* kernel_ms, double* total_ms) {
  if (kernel_ms) *kernel_ms = g_kernel_ms;
  if (total_ms) *total_ms = g_total_ms;
}

UNDISTORT_API const char* undistort_last_error(void) { return g_error.c_str(); }

}  // extern "C"
