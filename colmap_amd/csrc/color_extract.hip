// color_extract.hip -- colour extraction of a sparse model on gfx950 behind include/colmap_amd_color.h.
//
// Three kernels:
//   color_sample_kernel<C>   one observation per lane: Bitmap::InterpolateBilinear(x - 1/2, y - 1/2) with exactly the range
//                            test and the arithmetic of sample<> in undistort.hip -- in double, narrowed to float, NOT cast
//                            to uint8 (Reconstruction::ExtractColorsForAllImages adds the floats,
//                            scene/reconstruction.cc:1148-1154) -- written with a valid byte to the observation's slot.
//                            An observation without a value leaves its slot as it is: invalid. The image is resident on
//                            the device for the launch (a 1024x768 RGB image is 2.4 MB, inside one XCD's 4 MiB L2), each
//                            lane gathers its four texels through the caches; nothing is staged in LDS.
//   color_point_kernel       one point per lane, for a point with up to color_plan::kSerialMax slots: adds its valid
//                            samples in double IN SLOT ORDER, counts them, divides, rounds half away from zero, casts to
//                            uint8 (:1175-1179); count 0 -> (0, 0, 0). Lanes of a wave own neighbouring points, whose slot
//                            ranges are neighbours in memory.
//   color_point_wave_kernel  one point per wave, for a longer range (color_plan::long_points): lane g adds the slots
//                            begin + g, begin + g + 64, ... in ascending order, then the 64 partial sums are combined by
//                            the butterfly 32, 16, 8, 4, 2, 1 (__shfl_xor). Addition commutes, so every lane ends with the
//                            same double, and the order is a function of the range's length alone.
// There is no atomic anywhere: a colour does not depend on scheduling.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_color.h"
#include "color_plan.h"

#define COLOR_API __attribute__((visibility("default")))

namespace {

thread_local std::string g_error;

using Fail = color_plan::Fail;
#define COLOR_HIP(call)                                                                  \
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

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

template <int C>
__global__ __launch_bounds__(kBlock) void color_sample_kernel(const uint8_t* __restrict__ img, int W, int H,
                                                               const double* __restrict__ xy,
                                                               const long long* __restrict__ slot, long long n,
                                                               float* __restrict__ rgb, uint8_t* __restrict__ valid) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // COLMAP assumes that the upper left pixel centre is (0.5, 0.5)
  const double x = xy[2 * i] - 0.5, y = xy[2 * i + 1] - 0.5;
  const double xf = floor(x), yf = floor(y);
  // x0 < 0 || x1 >= W || y0 < 0 || y1 >= H, written so that NaN and values beyond int fail too
  if (!(xf >= 0.0 && xf + 1.0 <= (double)(W - 1) && yf >= 0.0 && yf + 1.0 <= (double)(H - 1))) return;
  const int x0 = (int)xf, y0 = (int)yf;
  const double dx = x - xf, dy = y - yf, dx_1 = 1.0 - dx, dy_1 = 1.0 - dy;
  const int pitch = W * C;
  const uint8_t* line0 = img + (size_t)y0 * pitch + x0 * C;
  const uint8_t* line1 = line0 + pitch;
  const long long s = slot[i];
  float* out = rgb + 3 * s;
  if (C == 1) {  // grey replicated to RGB, as Bitmap::Read(as_rgb = true) does
    const double v0 = dx_1 * line0[0] + dx * line0[1];
    const double v1 = dx_1 * line1[0] + dx * line1[1];
    const float v = (float)(dy_1 * v0 + dy * v1);
    out[0] = v;
    out[1] = v;
    out[2] = v;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v0 = dx_1 * line0[c] + dx * line0[C + c];
      const double v1 = dx_1 * line1[c] + dx * line1[C + c];
      out[c] = (float)(dy_1 * v0 + dy * v1);
    }
  }
  valid[s] = 1;
}

// round (half away from zero) and cast of a mean of values in [0, 255]
__device__ __forceinline__ void store_colour(const double sum[3], int count, long long p, uint8_t* __restrict__ out_rgb,
                                             int* __restrict__ out_count) {
#pragma unroll
  for (int c = 0; c < 3; ++c) out_rgb[3 * p + c] = count > 0 ? (uint8_t)round(sum[c] / (double)count) : (uint8_t)0;
  if (out_count) out_count[p] = count;
}

__global__ __launch_bounds__(kBlock) void color_point_kernel(const long long* __restrict__ ptr, long long num_points,
                                                              const float* __restrict__ rgb,
                                                              const uint8_t* __restrict__ valid,
                                                              uint8_t* __restrict__ out_rgb, int* __restrict__ out_count) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= num_points) return;
  const long long begin = ptr[p], end = ptr[p + 1];
  if (end - begin > color_plan::kSerialMax) return;  // color_point_wave_kernel's
  double sum[3] = {0.0, 0.0, 0.0};
  int count = 0;
  for (long long s = begin; s < end; ++s) {
    if (!valid[s]) continue;
    sum[0] += (double)rgb[3 * s];
    sum[1] += (double)rgb[3 * s + 1];
    sum[2] += (double)rgb[3 * s + 2];
    ++count;
  }
  store_colour(sum, count, p, out_rgb, out_count);
}

__global__ __launch_bounds__(kBlock) void color_point_wave_kernel(const long long* __restrict__ ptr,
                                                                   const long long* __restrict__ long_points,
                                                                   long long num_long, const float* __restrict__ rgb,
                                                                   const uint8_t* __restrict__ valid,
                                                                   uint8_t* __restrict__ out_rgb,
                                                                   int* __restrict__ out_count) {
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / color_plan::kWave;
  const int lane = threadIdx.x % color_plan::kWave;
  if (wave >= num_long) return;  // the whole wave leaves: the shuffles below see all 64 lanes or none
  const long long p = long_points[wave];
  const long long begin = ptr[p], end = ptr[p + 1];
  double sum[3] = {0.0, 0.0, 0.0};
  int count = 0;
  for (long long s = begin + lane; s < end; s += color_plan::kWave) {
    if (!valid[s]) continue;
    sum[0] += (double)rgb[3 * s];
    sum[1] += (double)rgb[3 * s + 1];
    sum[2] += (double)rgb[3 * s + 2];
    ++count;
  }
#pragma unroll
  for (int m = color_plan::kWave / 2; m >= 1; m >>= 1) {
    sum[0] += __shfl_xor(sum[0], m);
    sum[1] += __shfl_xor(sum[1], m);
    sum[2] += __shfl_xor(sum[2], m);
    count += __shfl_xor(count, m);
  }
  if (lane == 0) store_colour(sum, count, p, out_rgb, out_count);
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

template <typename T>
struct DeviceBuffer {  // grows, never shrinks, freed with its owner
  T* p = nullptr;
  size_t cap = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    COLOR_HIP(hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
  }
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  void create() {
    COLOR_HIP(hipEventCreate(&a));
    COLOR_HIP(hipEventCreate(&b));
  }
  double stop() {  // records b, waits for it, -> ms since a
    COLOR_HIP(hipEventRecord(b, 0));
    COLOR_HIP(hipEventSynchronize(b));
    float ms = 0.0f;
    COLOR_HIP(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

}  // namespace

struct color_extractor {
  int gpu_index = 0;
  int64_t num_slots = 0;
  std::vector<uint8_t> taken;  // host: the slots given so far
  DeviceBuffer<float> d_rgb;
  DeviceBuffer<uint8_t> d_valid, d_img, d_out_rgb;
  DeviceBuffer<double> d_xy;
  DeviceBuffer<long long> d_slot, d_ptr, d_long;
  DeviceBuffer<int> d_out_count;
  Timer ev;
  double sample_ms = 0.0, point_ms = 0.0, total_ms = 0.0;
};

namespace {

struct WallClock {  // adds the life time of the object to *total
  double* total;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit WallClock(double* t) : total(t) {}
  ~WallClock() { *total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

void bind_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Fail("no HIP device available: colour extraction runs on the GPU (there is no CPU path)");
  if (!(gpu_index >= 0 && gpu_index < ndev)) throw Fail("gpu_index " + std::to_string(gpu_index) + " out of range");
  COLOR_HIP(hipSetDevice(gpu_index));
}

static_assert(sizeof(long long) == sizeof(int64_t), "slots and ptr are uploaded as they are");

}  // namespace

extern "C" {

COLOR_API color_extractor* color_create(int64_t num_observations, int32_t gpu_index) {
  color_extractor* e = nullptr;
  const int rc = Guard([&] {
    COLOR_CHECK(num_observations >= 0, "num_observations must not be negative");
    bind_device(gpu_index);
    e = new color_extractor;
    WallClock clock(&e->total_ms);
    e->gpu_index = gpu_index;
    e->num_slots = num_observations;
    e->taken.assign((size_t)num_observations, 0);
    e->ev.create();
    if (num_observations > 0) {
      e->d_rgb.reserve((size_t)3 * num_observations);
      e->d_valid.reserve((size_t)num_observations);
      COLOR_HIP(hipMemsetAsync(e->d_rgb.p, 0, (size_t)3 * num_observations * sizeof(float), 0));
      COLOR_HIP(hipMemsetAsync(e->d_valid.p, 0, (size_t)num_observations, 0));
      COLOR_HIP(hipStreamSynchronize(0));
    }
  });
  if (rc != 0) {
    delete e;
    return nullptr;
  }
  return e;
}

COLOR_API int color_add_image(color_extractor* e, const uint8_t* data, int32_t width, int32_t height, int32_t channels,
                              int64_t n, const double* xy, const int64_t* slot) {
  return Guard([&] {
    COLOR_CHECK(e != nullptr, "null extractor");
    WallClock clock(&e->total_ms);
    // everything the caller can get wrong is checked before the first byte moves
    color_plan::check_image(width, height, channels, data);
    COLOR_CHECK(n >= 0 && (n == 0 || xy != nullptr), "xy is null");
    color_plan::check_and_take_slots(&e->taken, n, slot);
    if (n == 0) return;
    bind_device(e->gpu_index);
    const size_t bytes = (size_t)width * height * channels;
    e->d_img.reserve(bytes);
    e->d_xy.reserve((size_t)2 * n);
    e->d_slot.reserve((size_t)n);
    COLOR_HIP(hipMemcpyAsync(e->d_img.p, data, bytes, hipMemcpyHostToDevice, 0));
    COLOR_HIP(hipMemcpyAsync(e->d_xy.p, xy, (size_t)2 * n * sizeof(double), hipMemcpyHostToDevice, 0));
    COLOR_HIP(hipMemcpyAsync(e->d_slot.p, slot, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, 0));
    COLOR_HIP(hipEventRecord(e->ev.a, 0));
    const dim3 grid(blocks_for((size_t)n)), block(kBlock);
    if (channels == 1)
      hipLaunchKernelGGL((color_sample_kernel<1>), grid, block, 0, 0, e->d_img.p, width, height, e->d_xy.p, e->d_slot.p,
                         (long long)n, e->d_rgb.p, e->d_valid.p);
    else
      hipLaunchKernelGGL((color_sample_kernel<3>), grid, block, 0, 0, e->d_img.p, width, height, e->d_xy.p, e->d_slot.p,
                         (long long)n, e->d_rgb.p, e->d_valid.p);
    COLOR_HIP(hipGetLastError());
    e->sample_ms += e->ev.stop();  // also: the staging buffers are free for the next image
  });
}

COLOR_API int color_finish(color_extractor* e, int64_t num_points, const int64_t* ptr, uint8_t* rgb, int32_t* count) {
  return Guard([&] {
    COLOR_CHECK(e != nullptr, "null extractor");
    WallClock clock(&e->total_ms);
    color_plan::check_ptr(e->num_slots, num_points, ptr);
    COLOR_CHECK(num_points == 0 || rgb != nullptr, "rgb is null");
    if (num_points == 0) return;
    const std::vector<int64_t> long_points = color_plan::long_points(num_points, ptr);
    bind_device(e->gpu_index);
    const size_t P = (size_t)num_points;
    e->d_ptr.reserve(P + 1);
    e->d_out_rgb.reserve(3 * P);
    e->d_out_count.reserve(P);
    COLOR_HIP(hipMemcpyAsync(e->d_ptr.p, ptr, (P + 1) * sizeof(long long), hipMemcpyHostToDevice, 0));
    if (!long_points.empty()) {
      e->d_long.reserve(long_points.size());
      COLOR_HIP(hipMemcpyAsync(e->d_long.p, long_points.data(), long_points.size() * sizeof(long long),
                               hipMemcpyHostToDevice, 0));
    }
    COLOR_HIP(hipEventRecord(e->ev.a, 0));
    hipLaunchKernelGGL(color_point_kernel, dim3(blocks_for(P)), dim3(kBlock), 0, 0, e->d_ptr.p, (long long)num_points,
                       e->d_rgb.p, e->d_valid.p, e->d_out_rgb.p, e->d_out_count.p);
    COLOR_HIP(hipGetLastError());
    if (!long_points.empty()) {
      hipLaunchKernelGGL(color_point_wave_kernel, dim3(blocks_for(long_points.size() * (size_t)color_plan::kWave)),
                         dim3(kBlock), 0, 0, e->d_ptr.p, e->d_long.p, (long long)long_points.size(), e->d_rgb.p,
                         e->d_valid.p, e->d_out_rgb.p, e->d_out_count.p);
      COLOR_HIP(hipGetLastError());
    }
    e->point_ms += e->ev.stop();
    COLOR_HIP(hipMemcpy(rgb, e->d_out_rgb.p, 3 * P, hipMemcpyDeviceToHost));
    if (count) COLOR_HIP(hipMemcpy(count, e->d_out_count.p, P * sizeof(int), hipMemcpyDeviceToHost));
  });
}

COLOR_API int color_samples(color_extractor* e, float* rgb, uint8_t* valid) {
  return Guard([&] {
    COLOR_CHECK(e != nullptr, "null extractor");
    WallClock clock(&e->total_ms);
    if (e->num_slots == 0) return;
    COLOR_CHECK(rgb != nullptr && valid != nullptr, "null output buffer");
    bind_device(e->gpu_index);
    COLOR_HIP(hipMemcpy(rgb, e->d_rgb.p, (size_t)3 * e->num_slots * sizeof(float), hipMemcpyDeviceToHost));
    COLOR_HIP(hipMemcpy(valid, e->d_valid.p, (size_t)e->num_slots, hipMemcpyDeviceToHost));
  });
}

COLOR_API void color_destroy(color_extractor* e) {
  if (!e) return;
  (void)hipSetDevice(e->gpu_index);
  delete e;
}

COLOR_API int color_slot_layout(int64_t num_observations, int64_t num_points, const int64_t* obs_point,
                                const int64_t* obs_image, const int64_t* obs_point2D, int64_t* ptr, int64_t* slot) {
  return Guard([&] { color_plan::slot_layout(num_observations, num_points, obs_point, obs_image, obs_point2D, ptr, slot); });
}

COLOR_API void color_timing(color_extractor* e, double* sample_kernel_ms, double* point_kernel_ms, double* total_ms) {
  if (sample_kernel_ms) *sample_kernel_ms = e ? e->sample_ms : 0.0;
  if (point_kernel_ms) *point_kernel_ms = e ? e->point_ms : 0.0;
  if (total_ms) *total_ms = e ? e->total_ms : 0.0;
}

COLOR_API const char* color_last_error(void) { return g_error.c_str(); }

}  // extern "C"
