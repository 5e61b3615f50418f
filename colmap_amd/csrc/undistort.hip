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
// This file decides nothing: every check, camera, homography, route, buffer size and grid of a call comes from
// undistort_plan.h (plain C++17, tested without a GPU); an entry point plans, binds the device and runs the plans.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "undistort_plan.h"

#define UNDISTORT_API __attribute__((visibility("default")))

namespace {

namespace ud = camera;
namespace up = undistort_plan;
using up::Fail;
using up::kPixelsPerLane;

thread_local std::string g_error;
thread_local double g_kernel_ms = 0.0, g_total_ms = 0.0;

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

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

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

struct Buffers {  // the device images of one call, shared by all its plans
  DeviceBuffer<uint8_t> in;
  DeviceBuffer<uint32_t> out, mid;
};

template <int INTERP, int CHANNELS>
struct Variant {
  static constexpr int I = INTERP, C = CHANNELS;
};

// the one switch on interpolation and channels: f receives them as a Variant
template <typename F>
void for_variant(int interpolation, int channels, F&& f) {
  if (interpolation == UNDISTORT_BILINEAR) {
    if (channels == 1) f(Variant<UNDISTORT_BILINEAR, 1>()); else f(Variant<UNDISTORT_BILINEAR, 3>());
  } else {
    if (channels == 1) f(Variant<UNDISTORT_NEAREST, 1>()); else f(Variant<UNDISTORT_NEAREST, 3>());
  }
}

// One launch of a plan onto `target` (the plan's target or mid camera): the rectify kernel when a homography stands in
// front of that camera, the warp kernel otherwise.
void launch_warp(const up::ImagePlan& p, const undistort_cam& target, up::Grid g, const uint8_t* d_in, uint32_t* d_out) {
  UD_CHECK(target.model_id == ud::PINHOLE, "the warp target is a PINHOLE camera");
  const CamArgs src = to_args(p.source);
  Homography Hinv;
  std::memcpy(Hinv.h, p.hinv, sizeof(Hinv.h));
  const int W = target.width, H = target.height;
  const int in_pitch = p.source.width * p.channels, out_pitch = up::padded_pitch(W, p.channels) / 4;
  const dim3 block(up::kBlockX, up::kBlockY), grid(g.x, g.y);
  const double fx = target.params[0], fy = target.params[1], cx = target.params[2], cy = target.params[3];
  if (!p.has_homography)
    for_variant(p.interpolation, p.channels, [&](auto v) {
      hipLaunchKernelGGL((undistort_warp_kernel<decltype(v)::I, decltype(v)::C>), grid, block, 0, 0, src, fx, fy, cx, cy,
                         d_in, in_pitch, d_out, out_pitch, W, H);
    });
  else
    for_variant(p.interpolation, p.channels, [&](auto v) {
      hipLaunchKernelGGL((undistort_rectify_kernel<decltype(v)::I, decltype(v)::C>), grid, block, 0, 0, src, Hinv, fx, fy,
                         cx, cy, d_in, in_pitch, d_out, out_pitch, W, H);
    });
  UD_HIP(hipGetLastError());
}

void launch_resize(const uint8_t* d_src, int src_pitch, int SW, int SH, int channels, uint32_t* d_out, int W, int H,
                   up::Grid g) {
  const dim3 block(up::kBlockX, up::kBlockY), grid(g.x, g.y);
  const int out_pitch = up::padded_pitch(W, channels) / 4;
  if (channels == 1)
    hipLaunchKernelGGL((undistort_resize_kernel<1>), grid, block, 0, 0, d_src, src_pitch, SW, SH, d_out, out_pitch, W, H);
  else
    hipLaunchKernelGGL((undistort_resize_kernel<3>), grid, block, 0, 0, d_src, src_pitch, SW, SH, d_out, out_pitch, W, H);
  UD_HIP(hipGetLastError());
}

void download(uint8_t* host, const uint32_t* d_img, int W, int H, int C) {
  UD_HIP(hipMemcpy2DAsync(host, (size_t)W * C, d_img, (size_t)up::padded_pitch(W, C), (size_t)W * C, (size_t)H,
                          hipMemcpyDeviceToHost, 0));
  UD_HIP(hipStreamSynchronize(0));
}

// Carries out one plan: reserve, upload, one or two launches by route, download. With a timer the launches stand
// between its two events; -> their milliseconds (0 without a timer and for a clone).
double run_image(const up::ImagePlan& p, const uint8_t* data, uint8_t* out, Buffers* d, Timer* ev) {
  if (p.route == up::kClone) {
    std::memcpy(out, data, p.in_bytes);  // Bitmap::Clone
    return 0.0;
  }
  const undistort_cam &src = p.source, &tgt = p.target, &mid = p.mid;
  const int C = p.channels;
  d->in.reserve(p.in_bytes);
  d->out.reserve(p.out_words);
  d->mid.reserve(p.mid_words);
  UD_HIP(hipMemcpyAsync(d->in.p, data, p.in_bytes, hipMemcpyHostToDevice, 0));
  if (ev) UD_HIP(hipEventRecord(ev->a, 0));
  if (p.route == up::kResize) {
    launch_resize(d->in.p, src.width * C, src.width, src.height, C, d->out.p, tgt.width, tgt.height, p.grid);
  } else if (p.route == up::kDirect) {
    launch_warp(p, tgt, p.grid, d->in.p, d->out.p);
  } else {  // image/warp.cc:103-106, 141-143: warp at the source's resolution, then shrink
    launch_warp(p, mid, p.mid_grid, d->in.p, d->mid.p);
    launch_resize((const uint8_t*)d->mid.p, up::padded_pitch(mid.width, C), mid.width, mid.height, C, d->out.p, tgt.width,
                  tgt.height, p.grid);
  }
  if (ev) UD_HIP(hipEventRecord(ev->b, 0));
  download(out, d->out.p, tgt.width, tgt.height, C);
  if (!ev) return 0.0;
  UD_HIP(hipEventSynchronize(ev->b));
  float ms = 0.0f;
  UD_HIP(hipEventElapsedTime(&ms, ev->a, ev->b));
  return ms;
}

// The device half of the two batch entry points: plans[i] runs on images[i]; fills the timing of the call.
void run_batch(const std::vector<up::ImagePlan>& plans, const std::vector<undistort_image*>& images, int gpu_index) {
  bind_device(gpu_index);
  const auto t0 = std::chrono::steady_clock::now();
  Buffers d;
  Timer ev;
  double kernel_ms = 0.0;
  for (size_t i = 0; i < plans.size(); ++i) {
    images[i]->out_camera = plans[i].target;
    kernel_ms += run_image(plans[i], images[i]->data, images[i]->out, &d, &ev);
  }
  g_kernel_ms = kernel_ms;
  g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

UNDISTORT_API void undistort_options_init(undistort_options* o) { up::options_init(o); }

UNDISTORT_API int undistort_camera(const undistort_options* options, const undistort_cam* camera, undistort_cam* undistorted) {
  return Guard([&] {
    UD_CHECK(options && camera && undistorted, "null argument");
    up::undistort_camera_impl(*options, *camera, undistorted);
  });
}

UNDISTORT_API int undistort_cam_from_img(const undistort_cam* camera, const double* xy, int64_t n, double* uv) {
  return Guard([&] {
    UD_CHECK(camera && (n == 0 || (xy && uv)) && n >= 0, "null argument");
    up::cam_from_img(*camera, xy, n, uv);
  });
}

// Every entry point below plans first -- a Fail leaves the device unbound and nothing of the caller's written --, then binds
// the device, then runs its plans.
UNDISTORT_API int undistort_images(const undistort_options* options, int32_t num_images, undistort_image* images,
                                   int32_t gpu_index) {
  return Guard([&] {
    up::check_batch(options, num_images, images);
    std::vector<up::ImagePlan> plans;
    std::vector<undistort_image*> ims;
    for (int i = 0; i < num_images; ++i) {
      plans.push_back(up::plan_image(*options, images[i], i));
      ims.push_back(&images[i]);
    }
    run_batch(plans, ims, gpu_index);
  });
}

UNDISTORT_API int undistort_rectify_cameras(const undistort_cam* camera1, const undistort_cam* camera2, const double* R,
                                            const double* t, double* H1, double* H2, double* Q) {
  return Guard([&] {
    UD_CHECK(camera1 && camera2 && R && t && H1 && H2 && Q, "null argument");
    up::rectify_cameras_impl(*camera1, *camera2, R, t, H1, H2, Q);
  });
}

UNDISTORT_API int undistort_rectify_images(const undistort_options* options, int32_t num_pairs, undistort_stereo_pair* pairs,
                                           int32_t gpu_index) {
  return Guard([&] {
    up::check_batch(options, num_pairs, pairs);
    std::vector<up::PairPlan> pair_plans;
    std::vector<up::ImagePlan> plans;
    std::vector<undistort_image*> ims;
    for (int i = 0; i < num_pairs; ++i) {
      pair_plans.push_back(up::plan_pair(*options, pairs[i], i));
      undistort_image* im[2] = {&pairs[i].image1, &pairs[i].image2};
      for (int s = 0; s < 2; ++s) {
        plans.push_back(up::plan_pair_side(*options, pair_plans[i], *im[s], s));
        ims.push_back(im[s]);
      }
    }
    for (int i = 0; i < num_pairs; ++i) std::memcpy(pairs[i].Q, pair_plans[i].Q, sizeof(pairs[i].Q));  // all pairs planned
    run_batch(plans, ims, gpu_index);
  });
}

UNDISTORT_API int undistort_warp_homography(const undistort_options* options, const double* Hinv,
                                            const undistort_cam* target_camera, undistort_image* image, int32_t gpu_index) {
  return Guard([&] {
    const up::ImagePlan plan = up::plan_warp_homography(options, Hinv, target_camera, image);
    bind_device(gpu_index);
    Buffers d;
    run_image(plan, image->data, image->out, &d, nullptr);
    image->out_camera = plan.target;
  });
}

UNDISTORT_API int undistort_points(const undistort_cam* distorted, const undistort_cam* undistorted, double* xy, int64_t n,
                                   int32_t gpu_index) {
  return Guard([&] {
    UD_CHECK(distorted && undistorted && (n == 0 || xy) && n >= 0, "null argument");
    up::check_camera(*distorted);
    up::check_camera(*undistorted);
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
    const up::ImagePlan plan = up::plan_resize(src, src_width, src_height, channels, dst, dst_width, dst_height);
    bind_device(gpu_index);
    Buffers d;
    run_image(plan, src, dst, &d, nullptr);
  });
}

UNDISTORT_API void undistort_last_timing(double* kernel_ms, double* total_ms) {
  if (kernel_ms) *kernel_ms = g_kernel_ms;
  if (total_ms) *total_ms = g_total_ms;
}

UNDISTORT_API const char* undistort_last_error(void) { return g_error.c_str(); }

}  // extern "C"
