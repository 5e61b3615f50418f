// sift.hip -- SIFT feature extraction on gfx950 behind include/colmap_amd_sift.h: the arithmetic of the reference's
// VLFeat route (SiftCPUFeatureExtractor::Extract over thirdparty/VLFeat/sift.c), one value per input. The host plan --
// options, scale-space geometry, Gaussian taps, exp(-x) table, order, result assembly -- is sift_plan.h; what a lane
// evaluates is sift_solvers.h; this file holds the kernels, the buffers of a handle and the walk over the octaves.
//
// Kernels (all sums are single accumulators in the order the C code fixes; no atomics except the candidate counter):
//   sift_to_float / sift_upsample2 / sift_decimate   the base level of an octave
//   sift_conv_cols / sift_conv_rows   the separable Gaussian with padding by continuity: a tile plus its halo and the
//                                     taps are staged in LDS, every output is ONE float accumulator over the taps in
//                                     ascending source index (vl_imconvcol_vf)
//   sift_dog / sift_extrema           DoG levels; 26-neighbour extrema of the interior, appended through one counter
//                                     (any order: the keys are sorted afterwards, an overflow is counted and rerun)
//   sift_refine                       one lane per sorted candidate (sifts::refine)
//   sift_gradient                     modulus / angle planes of levels s_min+1 .. s_max-2
//   sift_orientations                 one wave per detection: lanes evaluate 64 window samples at a time into LDS, then
//                                     lane b adds what fell into bin b, in raster order of the window
//   sift_descriptors                  one workgroup of 128 lanes per output row: lanes evaluate 128 samples at a time,
//                                     then lane b adds what fell into descriptor bin b, in raster order of the window
// The order per bin of both histograms is therefore the reference's own.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_sift.h"
#include "sift_plan.h"
#include "sift_solvers.h"

#define SIFT_API __attribute__((visibility("default")))

namespace {

namespace sp = sift_plan;

thread_local std::string g_error;
thread_local double g_event_ms = 0.0, g_total_ms = 0.0, g_stage_ms[SIFT_NUM_STAGES] = {0, 0, 0, 0};

using Fail = sp::Fail;
#define SIFT_HIP(call)                                                                   \
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

constexpr int kMaxTaps = 2 * sp::kHaloLimit + 1;
constexpr int kOriLanes = 64;
constexpr int kDescLanes = 128;

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void sift_to_float(const uint8_t* __restrict__ in, float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)in[i] / 255.0f;  // sift.cc:190
}

__device__ inline float sift_half_sum(float a, float b) { return (float)(0.5 * (a + b)); }  // copy_and_upsample_rows

// copy_and_upsample_rows applied along x, then along y (sift.c:739-758, 1019-1020): in[h][w] -> out[2h][2w]
__global__ __launch_bounds__(256) void sift_upsample2(const float* __restrict__ in, float* __restrict__ out, int w, int h) {
  const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
  if (X >= 2 * w || Y >= 2 * h) return;
  const int x = X >> 1, y = Y >> 1;
  const bool xmid = (X & 1) && x < w - 1, ymid = (Y & 1) && y < h - 1;
  const float* r0 = in + (size_t)y * w;
  const float u0 = xmid ? sift_half_sum(r0[x], r0[x + 1]) : r0[x];
  float v = u0;
  if (ymid) {
    const float* r1 = r0 + w;
    const float u1 = xmid ? sift_half_sum(r1[x], r1[x + 1]) : r1[x];
    v = sift_half_sum(u0, u1);
  }
  out[(size_t)Y * (2 * w) + X] = v;
}

// copy_and_downsample (sift.c:835-851): out[dh][dw] = in[y * step][x * step]
__global__ __launch_bounds__(256) void sift_decimate(const float* __restrict__ in, int in_w, float* __restrict__ out, int dw, int dh,
                                                     int step) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= dw || y >= dh) return;
  out[(size_t)y * dw + x] = in[(size_t)(y * step) * in_w + (size_t)x * step];
}

// Column pass: out[y][x] = sum_t in[clamp(y - W + t)][x] * taps[t], t ascending. A workgroup of 64 x 4 lanes owns a tile
// of kColTileX x kColTileY outputs and stages its kColTileY + 2 W source rows.
__global__ __launch_bounds__(256) void sift_conv_cols(const float* __restrict__ in, float* __restrict__ out, int w, int h,
                                                      const float* __restrict__ taps, int W) {
  __shared__ float tile[(sp::kColTileY + 2 * sp::kHaloLimit) * sp::kColTileX];
  __shared__ float ftaps[kMaxTaps];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x0 = blockIdx.x * sp::kColTileX, y0 = blockIdx.y * sp::kColTileY;
  const int ntaps = 2 * W + 1;
  const int lin = ty * 64 + tx;
  if (lin < ntaps) ftaps[lin] = taps[lin];
  const int xs = min(x0 + tx, w - 1);
  const int rows = sp::kColTileY + 2 * W;
  for (int r = ty; r < rows; r += 4) {
    const int ys = min(max(y0 - W + r, 0), h - 1);
    tile[r * sp::kColTileX + tx] = in[(size_t)ys * w + xs];
  }
  __syncthreads();
  const int x = x0 + tx;
  if (x >= w) return;
  for (int k = 0; k < sp::kColTileY / 4; ++k) {
    const int r = ty + 4 * k, y = y0 + r;
    if (y >= h) break;
    float acc = 0;
    for (int t = 0; t < ntaps; ++t) {
      const float v = tile[(r + t) * sp::kColTileX + tx];
      const float c = ftaps[t];
      acc += v * c;
    }
    out[(size_t)y * w + x] = acc;
  }
}

// Row pass: out[y][x] = sum_t in[y][clamp(x - W + t)] * taps[t]. A workgroup owns kRowTileX x kRowTileY outputs.
__global__ __launch_bounds__(256) void sift_conv_rows(const float* __restrict__ in, float* __restrict__ out, int w, int h,
                                                      const float* __restrict__ taps, int W) {
  constexpr int kPitch = sp::kRowTileX + 2 * sp::kHaloLimit;
  __shared__ float tile[sp::kRowTileY * kPitch];
  __shared__ float ftaps[kMaxTaps];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x0 = blockIdx.x * sp::kRowTileX, y0 = blockIdx.y * sp::kRowTileY;
  const int ntaps = 2 * W + 1;
  const int lin = ty * 64 + tx;
  if (lin < ntaps) ftaps[lin] = taps[lin];
  const int cols = sp::kRowTileX + 2 * W;
  for (int r = ty; r < sp::kRowTileY; r += 4) {
    const int ys = min(y0 + r, h - 1);
    for (int c = tx; c < cols; c += 64) {
      const int xs = min(max(x0 - W + c, 0), w - 1);
      tile[r * kPitch + c] = in[(size_t)ys * w + xs];
    }
  }
  __syncthreads();
  for (int r = ty; r < sp::kRowTileY; r += 4) {
    const int y = y0 + r;
    if (y >= h) break;
    for (int c = tx; c < sp::kRowTileX; c += 64) {
      const int x = x0 + c;
      if (x >= w) break;
      float acc = 0;
      for (int t = 0; t < ntaps; ++t) {
        const float v = tile[r * kPitch + c + t];
        const float cc = ftaps[t];
        acc += v * cc;
      }
      out[(size_t)y * w + x] = acc;
    }
  }
}

// dog[l] = level[l + 1] - level[l] over the whole stack (sift.c:1176-1185): n = num_dog * w * h, plane = w * h
__global__ __launch_bounds__(256) void sift_dog(const float* __restrict__ levels, float* __restrict__ dog, long long n, long long plane) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dog[i] = levels[i + plane] - levels[i];
}

// vl_sift_detect's search (sift.c:1194-1258): x in 1..w-2, y in 1..h-2, DoG index 1..S
__global__ __launch_bounds__(256) void sift_extrema(const float* __restrict__ dog, int w, int h, double tp, unsigned long long* __restrict__ keys,
                                                    int* __restrict__ counter, int capacity) {
  const int x = 1 + blockIdx.x * 64 + threadIdx.x, y = 1 + blockIdx.y * 4 + threadIdx.y, si = 1 + blockIdx.z;
  if (x >= w - 1 || y >= h - 1) return;
  const size_t plane = (size_t)w * h;
  const float* pt = dog + (size_t)si * plane + (size_t)y * w + x;
  const float v = *pt;
  const bool may_max = (double)v >= 0.8 * tp, may_min = (double)v <= -0.8 * tp;
  if (!may_max && !may_min) return;
  bool is_max = may_max, is_min = may_min;
  for (int ds = -1; ds <= 1; ++ds)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (ds == 0 && dy == 0 && dx == 0) continue;
        const float n = pt[(long)ds * (long)plane + (long)dy * w + dx];
        is_max = is_max && v > n;
        is_min = is_min && v < n;
      }
  if (is_max || is_min) {
    const int slot = atomicAdd(counter, 1);
    if (slot < capacity) keys[slot] = sp::candidate_key(x, y, si);
  }
}

__global__ __launch_bounds__(64) void sift_refine(const float* __restrict__ dog, int w, int h, int s_min, int s_max,
                                                  const unsigned long long* __restrict__ keys, int n, double tp, double te, double xper,
                                                  sifts::Refined* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int x, y, si;
  sp::candidate_unkey(keys[i], &x, &y, &si);
  out[i] = sifts::refine(dog, w, h, s_min, s_max, x, y, si + s_min, tp, te, xper);
}

// update_gradient (sift.c:1446-1531): one-sided differences at the borders. levels: the octave's Gaussian stack; plane p
// is level index p + 1. w, h >= 2.
__global__ __launch_bounds__(256) void sift_gradient(const float* __restrict__ levels, float* __restrict__ grad, int w, int h) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, p = blockIdx.z;
  if (x >= w || y >= h) return;
  const size_t plane = (size_t)w * h;
  const float* src = levels + (size_t)(p + 1) * plane + (size_t)y * w + x;
  float gx, gy;
  if (x == 0)
    gx = src[1] - src[0];
  else if (x == w - 1)
    gx = src[0] - src[-1];
  else
    gx = (float)(0.5 * (src[1] - src[-1]));
  if (y == 0)
    gy = src[w] - src[0];
  else if (y == h - 1)
    gy = src[0] - src[-w];
  else
    gy = (float)(0.5 * (src[w] - src[-w]));
  float mod, ang;
  sifts::gradient_polar(gx, gy, &mod, &ang);
  float* g = grad + 2 * ((size_t)p * plane + (size_t)y * w + x);
  g[0] = mod;
  g[1] = ang;
}

struct DeviceDetection {  // what the orientation and descriptor kernels read of a detection
  float x, y, sigma;
  int32_t is;
};

// vl_sift_calc_keypoint_orientations (sift.c:1559-1692), one wave per detection
__global__ __launch_bounds__(kOriLanes) void sift_orientations(const float* __restrict__ grad, int w, int h, int s_min, int s_max,
                                                               const DeviceDetection* __restrict__ dets, double xper,
                                                               const double* __restrict__ expn, int* __restrict__ counts,
                                                               double* __restrict__ angles) {
  __shared__ int sb0[kOriLanes], sb1[kOriLanes];
  __shared__ double sv0[kOriLanes], sv1[kOriLanes];
  __shared__ double hist[sifts::kOriBins];
  const int d = blockIdx.x, lane = threadIdx.x;
  const DeviceDetection k = dets[d];
  const double x = (double)k.x / xper, y = (double)k.y / xper, sigma = (double)k.sigma / xper;
  const int xi = (int)(x + 0.5), yi = (int)(y + 0.5), si = k.is;
  const double sigmaw = 1.5 * sigma;
  const int W = (int)fmax(floor(3.0 * sigmaw), 1.0);
  if (xi < 0 || xi > w - 1 || yi < 0 || yi > h - 1 || si < s_min + 1 || si > s_max - 2) {  // uniform over the wave
    if (lane == 0) counts[d] = 0;
    if (lane < 4) angles[4 * (size_t)d + lane] = 0.0;
    return;
  }
  const float* plane = grad + 2 * (size_t)(si - s_min - 1) * ((size_t)w * h);
  const int ys_lo = max(-W, -yi), ys_hi = min(W, h - 1 - yi), xs_lo = max(-W, -xi), xs_hi = min(W, w - 1 - xi);
  const int ncols = xs_hi - xs_lo + 1, total = ncols * (ys_hi - ys_lo + 1);
  double acc = 0.0;  // bin `lane` of the histogram (lanes 0..35)
  for (int base = 0; base < total; base += kOriLanes) {
    const int idx = base + lane;
    int b0 = -1, b1 = -1;
    double v0 = 0.0, v1 = 0.0;
    if (idx < total) {
      const int px = xi + xs_lo + idx % ncols, py = yi + ys_lo + idx / ncols;
      const float* g = plane + 2 * ((size_t)py * w + px);
      if (!sifts::orientation_sample(expn, x, y, sigmaw, W, px, py, g[0], g[1], &b0, &b1, &v0, &v1)) b0 = b1 = -1;
    }
    sb0[lane] = b0;
    sb1[lane] = b1;
    sv0[lane] = v0;
    sv1[lane] = v1;
    __syncthreads();
    if (lane < sifts::kOriBins) {
      const int m = min(kOriLanes, total - base);
      for (int j = 0; j < m; ++j) {
        if (sb0[j] == lane) acc += sv0[j];
        if (sb1[j] == lane) acc += sv1[j];
      }
    }
    __syncthreads();
  }
  if (lane < sifts::kOriBins) hist[lane] = acc;
  __syncthreads();
  if (lane != 0) return;
  constexpr int nbins = sifts::kOriBins;
  for (int iter = 0; iter < 6; ++iter) {
    double prev = hist[nbins - 1];
    const double first = hist[0];
    int i;
    for (i = 0; i < nbins - 1; i++) {
      const double newh = (prev + hist[i] + hist[(i + 1) % nbins]) / 3.0;
      prev = hist[i];
      hist[i] = newh;
    }
    hist[i] = (prev + hist[i] + first) / 3.0;
  }
  double maxh = 0;
  for (int i = 0; i < nbins; ++i) maxh = fmax(maxh, hist[i]);
  int nangles = 0;
  double* out = angles + 4 * (size_t)d;
  out[0] = out[1] = out[2] = out[3] = 0.0;
  for (int i = 0; i < nbins && nangles < 4; ++i) {
    const double h0 = hist[i];
    const double hm = hist[(i - 1 + nbins) % nbins];
    const double hp = hist[(i + 1 + nbins) % nbins];
    if (h0 > 0.8 * maxh && h0 > hm && h0 > hp) {
      const double di = -0.5 * (hp - hm) / (hp + hm - 2 * h0);
      const double th = 2 * sifts::kPi * (i + di + 0.5) / nbins;
      out[nangles++] = th;
    }
  }
  counts[d] = nangles;
}

struct DeviceRow {  // one output row: a detection and one of its angles, with the host's sin and cos of it
  int32_t det, pad;
  double angle0, st0, ct0;
};

// vl_sift_calc_keypoint_descriptor (sift.c:1923-2093), then L1_ROOT / L2 and the cast to bytes (feature/utils.cc:45-69),
// one workgroup per row. float_desc in VLFeat's bin order, bytes in UBC order.
__global__ __launch_bounds__(kDescLanes) void sift_descriptors(const float* __restrict__ grad, int w, int h, int s_min, int s_max,
                                                               const DeviceDetection* __restrict__ dets,
                                                               const DeviceRow* __restrict__ rows, double xper,
                                                               const double* __restrict__ expn, int normalization,
                                                               float* __restrict__ float_desc, uint8_t* __restrict__ bytes) {
  __shared__ sifts::DescSample samples[kDescLanes];
  __shared__ float descr[sifts::kDescDim];
  const int row = blockIdx.x, lane = threadIdx.x;
  const DeviceRow R = rows[row];
  const DeviceDetection k = dets[R.det];
  const double x = (double)k.x / xper, y = (double)k.y / xper, sigma = (double)k.sigma / xper;
  const int xi = (int)(x + 0.5), yi = (int)(y + 0.5), si = k.is;
  const double SBP = 3.0 * sigma + sifts::kEpsD;
  const int W = (int)floor(1.4142135623730951 * SBP * (sifts::kNBP + 1) / 2.0 + 0.5);
  float* fout = float_desc + (size_t)row * sifts::kDescDim;
  uint8_t* bout = bytes + (size_t)row * sifts::kDescDim;
  if (xi < 0 || xi >= w || yi < 0 || yi >= h - 1 || si < s_min + 1 || si > s_max - 2) {  // uniform over the workgroup
    fout[lane] = 0.0f;
    bout[lane] = 0;
    return;
  }
  const float* plane = grad + 2 * (size_t)(si - s_min - 1) * ((size_t)w * h);
  const int dy_lo = max(-W, 1 - yi), dy_hi = min(W, h - yi - 2), dx_lo = max(-W, 1 - xi), dx_hi = min(W, w - xi - 2);
  const int ncols = max(dx_hi - dx_lo + 1, 0), nrows = max(dy_hi - dy_lo + 1, 0), total = ncols * nrows;
  const int bt = lane & 7, bx = ((lane >> 3) & 3) - sifts::kNBP / 2, by = (lane >> 5) - sifts::kNBP / 2;  // this lane's bin
  float acc = 0.0f;
  for (int base = 0; base < total; base += kDescLanes) {
    const int idx = base + lane;
    if (idx < total) {
      const int px = xi + dx_lo + idx % ncols, py = yi + dy_lo + idx / ncols;
      const float* g = plane + 2 * ((size_t)py * w + px);
      samples[lane] = sifts::descriptor_sample(expn, x, y, R.angle0, R.st0, R.ct0, SBP, px, py, g[0], g[1]);
    }
    __syncthreads();
    const int m = min(kDescLanes, total - base);
    for (int j = 0; j < m; ++j) {
      const int ddx = bx - samples[j].binx, ddy = by - samples[j].biny;
      if (ddx < 0 || ddx > 1 || ddy < 0 || ddy > 1) continue;
      const int bint = samples[j].bint;
      const int ddt = (bint % sifts::kNBO == bt) ? 0 : ((bint + 1) % sifts::kNBO == bt) ? 1 : -1;
      if (ddt < 0) continue;
      acc += samples[j].wgt[ddx * 4 + ddy * 2 + ddt];
    }
    __syncthreads();
  }
  descr[lane] = acc;
  __syncthreads();
  if (lane == 0) {  // normalize_histogram, the clamp at 0.2, again; then the reference's own normalisation: all sequential sums
    for (int pass = 0; pass < 2; ++pass) {
      float norm = 0.0f;
      for (int i = 0; i < sifts::kDescDim; ++i) norm += descr[i] * descr[i];
      norm = sifts::fast_sqrt_f(norm) + sifts::kEpsF;
      for (int i = 0; i < sifts::kDescDim; ++i) descr[i] /= norm;
      if (pass == 0)
        for (int i = 0; i < sifts::kDescDim; ++i)
          if ((double)descr[i] > 0.2) descr[i] = (float)0.2;
    }
  }
  __syncthreads();
  const float v = descr[lane];
  fout[lane] = v;
  __syncthreads();
  if (lane == 0) {
    if (normalization == SIFT_NORMALIZATION_L2) {  // rowwise().normalize()
      float z = 0.0f;
      for (int i = 0; i < sifts::kDescDim; ++i) z += descr[i] * descr[i];
      if (z > 0.0f) {
        const float n = sqrtf(z);
        for (int i = 0; i < sifts::kDescDim; ++i) descr[i] /= n;
      }
    } else {  // row *= 1 / lpNorm<1>(); row = sqrt(row)
      float l1 = 0.0f;
      for (int i = 0; i < sifts::kDescDim; ++i) l1 += fabsf(descr[i]);
      const float inv = 1 / l1;
      for (int i = 0; i < sifts::kDescDim; ++i) descr[i] = sqrtf(descr[i] * inv);
    }
  }
  __syncthreads();
  const float scaled = roundf(512.0f * descr[lane]);
  const float clamped = fminf(255.0f, fmaxf(0.0f, scaled));  // TruncateCast<float, uint8_t>
  bout[sp::ubc_index(lane)] = (uint8_t)clamped;
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    if (p) SIFT_HIP(hipFree(p));
    p = nullptr;
    cap = 0;
    SIFT_HIP(hipMalloc(&p, bytes));
    cap = bytes;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

struct Octave {
  int w = 0, h = 0, o = 0;
  DevBuf levels, dog, grad;
  int64_t num_candidates = 0;
  std::vector<sift_detection> detections;
  std::vector<int32_t> ori_counts;
  std::vector<double> ori_angles;
};

}  // namespace

struct sift_handle {
  int gpu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[SIFT_NUM_STAGES + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  DevBuf grey, image, temp, taps, expn, keys, keys_sorted, sort_tmp, counter, refined, dets, ori_counts, ori_angles,
      rows, fdesc, bdesc;
  std::vector<Octave> octaves;
  int num_octaves = 0;
  sp::Geometry geom;
  int forced_capacity = 0;
  int64_t reruns = 0;
  // the last result
  std::vector<float> keypoints, float_desc;
  std::vector<uint8_t> desc;
};

namespace {

dim3 Grid2(int w, int h, int z = 1) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)z); }

void Smooth(sift_handle* H, const float* in, float* out, int w, int h, const float* taps, int W) {
  float* temp = H->temp.as<float>();
  hipLaunchKernelGGL(sift_conv_cols, dim3((w + sp::kColTileX - 1) / sp::kColTileX, (h + sp::kColTileY - 1) / sp::kColTileY), dim3(64, 4), 0,
                     H->stream, in, temp, w, h, taps, W);
  hipLaunchKernelGGL(sift_conv_rows, dim3((w + sp::kRowTileX - 1) / sp::kRowTileX, (h + sp::kRowTileY - 1) / sp::kRowTileY), dim3(64, 4), 0,
                     H->stream, (const float*)temp, out, w, h, taps, W);
}

sp::Options PlanOptions(const sift_options& o) {
  sp::Options p;
  p.max_num_features = o.max_num_features;
  p.first_octave = o.first_octave;
  p.num_octaves = o.num_octaves;
  p.octave_resolution = o.octave_resolution;
  p.peak_threshold = o.peak_threshold;
  p.edge_threshold = o.edge_threshold;
  p.max_num_orientations = o.max_num_orientations;
  p.upright = o.upright;
  p.normalization = o.normalization;
  return p;
}

void Extract(sift_handle* H, const uint8_t* grey, int width, int height, const sift_options& copt) {
  const sp::Options opt = PlanOptions(copt);
  const std::string bad = sp::check(opt);
  if (!bad.empty()) throw Fail("sift_extract: " + bad);
  if (!grey || width < 1 || height < 1) throw Fail("sift_extract: an image of at least 1 x 1 pixels is needed");
  const sp::Geometry g = sp::geometry(width, height, opt);
  const int n_oct = sp::num_octaves_run(g);
  if (g.octave_width(g.o_min) >= sp::kMaxOctaveDim || g.octave_height(g.o_min) >= sp::kMaxOctaveDim)
    throw Fail("sift_extract: the first octave is larger than 2^20 pixels along one side");
  SIFT_HIP(hipSetDevice(H->gpu));
  H->geom = g;
  H->num_octaves = 0;
  H->keypoints.clear();
  H->float_desc.clear();
  H->desc.clear();
  if ((int)H->octaves.size() < n_oct) H->octaves.resize(n_oct);

  // every filter of the extraction, made on the host: [0] first base smoothing, [1] later base smoothing, [2 + i] level
  // s_min + 1 + i
  const int L = g.num_levels();
  std::vector<sp::Smoothing> sm(2 + (L - 1));
  sm[0] = sp::base_smoothing(g, true);
  sm[1] = sp::base_smoothing(g, false);
  for (int i = 0; i < L - 1; ++i) sm[2 + i] = sp::Smoothing{true, sp::level_sigma(g, g.s_min + 1 + i)};
  std::vector<float> taps_host((size_t)sm.size() * kMaxTaps, 0.0f);
  std::vector<int> half(sm.size(), 0);
  for (size_t i = 0; i < sm.size(); ++i) {
    if (!sm[i].apply) continue;
    half[i] = sp::gaussian_half_width(sm[i].sigma);
    if (half[i] > sp::kHaloLimit)
      throw Fail("sift_extract: a smoothing of sigma " + std::to_string(sm[i].sigma) + " needs a half-width of " + std::to_string(half[i]) +
                 " taps, above the " + std::to_string(sp::kHaloLimit) + " the convolution kernels stage (octave_resolution too small)");
    const std::vector<float> f = sp::gaussian_taps(sm[i].sigma);
    std::memcpy(&taps_host[i * kMaxTaps], f.data(), f.size() * sizeof(float));
  }
  H->taps.ensure(taps_host.size() * sizeof(float));
  SIFT_HIP(hipMemcpy(H->taps.p, taps_host.data(), taps_host.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!H->expn.p) {
    const std::vector<double> t = sp::expn_table();
    H->expn.ensure(t.size() * sizeof(double));
    SIFT_HIP(hipMemcpy(H->expn.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  const float* taps = H->taps.as<float>();
  const double* expn = H->expn.as<double>();

  const size_t npix = (size_t)width * height;
  H->grey.ensure(npix);
  H->image.ensure(npix * sizeof(float));
  SIFT_HIP(hipMemcpyAsync(H->grey.p, grey, npix, hipMemcpyHostToDevice, H->stream));
  H->counter.ensure(sizeof(int));
  const size_t plane0 = (size_t)g.octave_width(g.o_min) * g.octave_height(g.o_min);
  H->temp.ensure(plane0 * sizeof(float));

  // levels of output rows, over all octaves (sift.cc:212-291)
  std::vector<int> level_num_features, level_num_rows;
  std::vector<float> all_kp, all_fdesc;
  std::vector<uint8_t> all_desc;
  double stage_ms[SIFT_NUM_STAGES] = {0, 0, 0, 0};

  for (int k = 0; k < n_oct; ++k) {
    Octave& oc = H->octaves[k];
    const int o = g.o_min + k, w = g.octave_width(o), h = g.octave_height(o);
    const size_t plane = (size_t)w * h;
    oc.w = w;
    oc.h = h;
    oc.o = o;
    oc.num_candidates = 0;
    oc.detections.clear();
    oc.ori_counts.clear();
    oc.ori_angles.clear();
    oc.levels.ensure(plane * L * sizeof(float));
    oc.dog.ensure(plane * g.num_dog() * sizeof(float));
    oc.grad.ensure(plane * g.num_grad() * 2 * sizeof(float));
    float* levels = oc.levels.as<float>();
    float* dog = oc.dog.as<float>();
    float* grad = oc.grad.as<float>();
    const double xper = pow(2.0, (double)o);

    // ---- pyramid (the events mark the borders of the stages: an interval holds the stage's launches AND the host
    // synchronisations, copies and gaps between them)
    SIFT_HIP(hipEventRecord(H->ev[0], H->stream));
    if (k == 0) {
      hipLaunchKernelGGL(sift_to_float, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, H->stream, H->grey.as<uint8_t>(),
                         H->image.as<float>(), (long long)npix);
      if (g.o_min < 0)
        hipLaunchKernelGGL(sift_upsample2, Grid2(w, h), dim3(64, 4), 0, H->stream, (const float*)H->image.as<float>(), levels, width, height);
      else
        hipLaunchKernelGGL(sift_decimate, Grid2(w, h), dim3(64, 4), 0, H->stream, (const float*)H->image.as<float>(), width, levels, w, h,
                           1 << g.o_min);
    } else {
      const Octave& prev = H->octaves[k - 1];
      const float* seed = prev.levels.as<float>() + (size_t)(sp::seed_level(g) - g.s_min) * prev.w * prev.h;
      hipLaunchKernelGGL(sift_decimate, Grid2(w, h), dim3(64, 4), 0, H->stream, seed, prev.w, levels, w, h, 2);
    }
    const int base = k == 0 ? 0 : 1;
    if (sm[base].apply) Smooth(H, levels, levels, w, h, taps + (size_t)base * kMaxTaps, half[base]);
    for (int i = 0; i < L - 1; ++i)
      Smooth(H, levels + (size_t)i * plane, levels + (size_t)(i + 1) * plane, w, h, taps + (size_t)(2 + i) * kMaxTaps, half[2 + i]);

    // ---- detection
    SIFT_HIP(hipEventRecord(H->ev[1], H->stream));
    const long long ndog = (long long)plane * g.num_dog();
    hipLaunchKernelGGL(sift_dog, dim3((unsigned)((ndog + 255) / 256)), dim3(256), 0, H->stream, (const float*)levels, dog, ndog, (long long)plane);
    int count = 0;
    if (w >= 3 && h >= 3) {
      int capacity = H->forced_capacity > 0 ? H->forced_capacity : sp::candidate_capacity(w, h, g.S);
      for (;;) {
        H->keys.ensure((size_t)capacity * sizeof(unsigned long long));
        SIFT_HIP(hipMemsetAsync(H->counter.p, 0, sizeof(int), H->stream));
        hipLaunchKernelGGL(sift_extrema, Grid2(w - 2, h - 2, g.S), dim3(64, 4), 0, H->stream, (const float*)dog, w, h, opt.peak_threshold,
                           H->keys.as<unsigned long long>(), H->counter.as<int>(), capacity);
        SIFT_HIP(hipMemcpyAsync(&count, H->counter.p, sizeof(int), hipMemcpyDeviceToHost, H->stream));
        SIFT_HIP(hipStreamSynchronize(H->stream));
        if (count <= capacity) break;
        capacity = sp::grown_capacity(count);  // never truncate: rerun with room for all of them
        ++H->reruns;
      }
    }
    oc.num_candidates = count;
    std::vector<sifts::Refined> refined(count);
    if (count > 0) {
      H->keys_sorted.ensure((size_t)count * sizeof(unsigned long long));
      size_t tmp_bytes = 0;
      SIFT_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, H->keys.as<unsigned long long>(), H->keys_sorted.as<unsigned long long>(),
                                                 count, 0, 64, H->stream));
      H->sort_tmp.ensure(tmp_bytes);
      SIFT_HIP(hipcub::DeviceRadixSort::SortKeys(H->sort_tmp.p, tmp_bytes, H->keys.as<unsigned long long>(),
                                                 H->keys_sorted.as<unsigned long long>(), count, 0, 64, H->stream));
      H->refined.ensure((size_t)count * sizeof(sifts::Refined));
      hipLaunchKernelGGL(sift_refine, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, H->stream, (const float*)dog, w, h, g.s_min, g.s_max,
                         (const unsigned long long*)H->keys_sorted.as<unsigned long long>(), count, opt.peak_threshold, opt.edge_threshold, xper,
                         H->refined.as<sifts::Refined>());
      SIFT_HIP(hipMemcpyAsync(refined.data(), H->refined.p, (size_t)count * sizeof(sifts::Refined), hipMemcpyDeviceToHost, H->stream));
    }
    SIFT_HIP(hipEventRecord(H->ev[2], H->stream));
    SIFT_HIP(hipStreamSynchronize(H->stream));
    std::vector<DeviceDetection> dets;
    for (const sifts::Refined& r : refined) {
      if (!r.good) continue;
      sift_detection d;
      d.o = o;
      d.ix = r.ix;
      d.iy = r.iy;
      d.is = r.is;
      d.x = r.x;
      d.y = r.y;
      d.s = r.s;
      d.sigma = sp::keypoint_sigma(g, r.sn, o);
      oc.detections.push_back(d);
      dets.push_back(DeviceDetection{d.x, d.y, d.sigma, d.is});
    }
    const int nd = (int)dets.size();
    float ms = 0;
    if (nd == 0) {
      SIFT_HIP(hipEventElapsedTime(&ms, H->ev[0], H->ev[1]));
      stage_ms[SIFT_STAGE_PYRAMID] += ms;
      SIFT_HIP(hipEventElapsedTime(&ms, H->ev[1], H->ev[2]));
      stage_ms[SIFT_STAGE_DETECTION] += ms;
      continue;
    }

    // ---- orientation (the gradient planes are made once per octave, on the first use: update_gradient)
    hipLaunchKernelGGL(sift_gradient, Grid2(w, h, g.num_grad()), dim3(64, 4), 0, H->stream, (const float*)levels, grad, w, h);
    H->dets.ensure((size_t)nd * sizeof(DeviceDetection));
    SIFT_HIP(hipMemcpyAsync(H->dets.p, dets.data(), (size_t)nd * sizeof(DeviceDetection), hipMemcpyHostToDevice, H->stream));
    oc.ori_counts.assign(nd, 1);
    oc.ori_angles.assign((size_t)nd * 4, 0.0);
    if (!opt.upright) {
      H->ori_counts.ensure((size_t)nd * sizeof(int));
      H->ori_angles.ensure((size_t)nd * 4 * sizeof(double));
      hipLaunchKernelGGL(sift_orientations, dim3((unsigned)nd), dim3(kOriLanes), 0, H->stream, (const float*)grad, w, h, g.s_min, g.s_max,
                         (const DeviceDetection*)H->dets.as<DeviceDetection>(), xper, expn, H->ori_counts.as<int>(),
                         H->ori_angles.as<double>());
      SIFT_HIP(hipMemcpyAsync(oc.ori_counts.data(), H->ori_counts.p, (size_t)nd * sizeof(int), hipMemcpyDeviceToHost, H->stream));
      SIFT_HIP(hipMemcpyAsync(oc.ori_angles.data(), H->ori_angles.p, (size_t)nd * 4 * sizeof(double), hipMemcpyDeviceToHost, H->stream));
    }
    SIFT_HIP(hipEventRecord(H->ev[3], H->stream));
    SIFT_HIP(hipStreamSynchronize(H->stream));

    // ---- rows and descriptors: the first max_num_orientations angles of every detection (sift.cc:253-257), with the C
    // library's sin and cos of each
    std::vector<DeviceRow> rows;
    int prev_level = -1;
    for (int i = 0; i < nd; ++i) {
      if (oc.detections[i].is != prev_level) {
        level_num_features.push_back(0);
        level_num_rows.push_back(0);
      }
      level_num_features.back() += 1;
      prev_level = oc.detections[i].is;
      const int used = std::min(oc.ori_counts[i], opt.max_num_orientations);
      for (int a = 0; a < used; ++a) {
        const double angle0 = oc.ori_angles[(size_t)i * 4 + a];
        rows.push_back(DeviceRow{i, 0, angle0, sin(angle0), cos(angle0)});
        level_num_rows.back() += 1;
      }
    }
    const int nr = (int)rows.size();
    if (nr > 0) {
      H->rows.ensure((size_t)nr * sizeof(DeviceRow));
      H->fdesc.ensure((size_t)nr * 128 * sizeof(float));
      H->bdesc.ensure((size_t)nr * 128);
      SIFT_HIP(hipMemcpyAsync(H->rows.p, rows.data(), (size_t)nr * sizeof(DeviceRow), hipMemcpyHostToDevice, H->stream));
      hipLaunchKernelGGL(sift_descriptors, dim3((unsigned)nr), dim3(kDescLanes), 0, H->stream, (const float*)grad, w, h, g.s_min, g.s_max,
                         (const DeviceDetection*)H->dets.as<DeviceDetection>(), (const DeviceRow*)H->rows.as<DeviceRow>(), xper, expn,
                         opt.normalization, H->fdesc.as<float>(), H->bdesc.as<uint8_t>());
      const size_t at = all_desc.size();
      all_desc.resize(at + (size_t)nr * 128);
      all_fdesc.resize(at + (size_t)nr * 128);
      SIFT_HIP(hipMemcpyAsync(all_fdesc.data() + at, H->fdesc.p, (size_t)nr * 128 * sizeof(float), hipMemcpyDeviceToHost, H->stream));
      SIFT_HIP(hipMemcpyAsync(all_desc.data() + at, H->bdesc.p, (size_t)nr * 128, hipMemcpyDeviceToHost, H->stream));
      for (const DeviceRow& r : rows) {
        const sift_detection& d = oc.detections[r.det];
        all_kp.push_back(d.x + 0.5f);
        all_kp.push_back(d.y + 0.5f);
        all_kp.push_back(d.sigma);
        all_kp.push_back((float)r.angle0);
      }
    }
    SIFT_HIP(hipEventRecord(H->ev[4], H->stream));
    SIFT_HIP(hipStreamSynchronize(H->stream));
    for (int s = 0; s < SIFT_NUM_STAGES; ++s) {
      SIFT_HIP(hipEventElapsedTime(&ms, H->ev[s], H->ev[s + 1]));
      stage_ms[s] += ms;
    }
  }
  H->num_octaves = n_oct;

  // ---- the cut to max_num_features (sift.cc:294-333): whole levels from the coarsest down
  const sp::Cut cut = sp::cut_levels(level_num_features, level_num_rows, opt.max_num_features);
  size_t skip = 0;
  for (int i = 0; i < cut.first_level; ++i) skip += (size_t)level_num_rows[i];
  const size_t n_out = (size_t)cut.num_out;
  H->keypoints.assign(all_kp.begin() + skip * 4, all_kp.begin() + (skip + n_out) * 4);
  H->float_desc.assign(all_fdesc.begin() + skip * 128, all_fdesc.begin() + (skip + n_out) * 128);
  H->desc.assign(all_desc.begin() + skip * 128, all_desc.begin() + (skip + n_out) * 128);
  g_event_ms = 0.0;
  for (int s = 0; s < SIFT_NUM_STAGES; ++s) {
    g_stage_ms[s] = stage_ms[s];
    g_event_ms += stage_ms[s];
  }
}

Octave& OctaveOf(sift_handle* H, int k) {
  if (!H) throw Fail("sift: null handle");
  if (k < 0 || k >= H->num_octaves) throw Fail("sift: octave " + std::to_string(k) + " of " + std::to_string(H->num_octaves));
  return H->octaves[k];
}

}  // namespace

extern "C" {

SIFT_API void sift_options_init(sift_options* o) {
  const sp::Options d;
  o->max_num_features = d.max_num_features;
  o->first_octave = d.first_octave;
  o->num_octaves = d.num_octaves;
  o->octave_resolution = d.octave_resolution;
  o->peak_threshold = d.peak_threshold;
  o->edge_threshold = d.edge_threshold;
  o->max_num_orientations = d.max_num_orientations;
  o->upright = d.upright;
  o->normalization = d.normalization;
  o->reserved = 0;
}

SIFT_API const char* sift_options_check(const sift_options* o) {
  thread_local std::string msg;
  msg = sp::check(PlanOptions(*o));
  return msg.c_str();
}

SIFT_API int sift_create(int32_t gpu_index, sift_handle** handle) {
  return Guard([&] {
    if (!handle) throw Fail("sift_create: null handle pointer");
    *handle = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
      throw Fail("no HIP device available: SIFT extraction runs on the GPU (there is no CPU path)");
    if (gpu_index < 0) gpu_index = 0;
    if (gpu_index >= n) throw Fail("sift_create: gpu_index " + std::to_string(gpu_index) + " out of range (" + std::to_string(n) + " devices)");
    SIFT_HIP(hipSetDevice(gpu_index));
    sift_handle* H = new sift_handle();
    H->gpu = gpu_index;
    try {
      SIFT_HIP(hipStreamCreateWithFlags(&H->stream, hipStreamNonBlocking));
      for (auto& e : H->ev) SIFT_HIP(hipEventCreate(&e));
    } catch (...) {
      sift_destroy(H);
      throw;
    }
    *handle = H;
  });
}

SIFT_API void sift_destroy(sift_handle* H) {
  if (!H) return;
  (void)hipSetDevice(H->gpu);
  if (H->stream) (void)hipStreamSynchronize(H->stream);
  for (DevBuf* b : {&H->grey, &H->image, &H->temp, &H->taps, &H->expn, &H->keys, &H->keys_sorted, &H->sort_tmp,
                    &H->counter, &H->refined, &H->dets, &H->ori_counts, &H->ori_angles, &H->rows, &H->fdesc, &H->bdesc})
    b->release();
  for (Octave& o : H->octaves) {
    o.levels.release();
    o.dog.release();
    o.grad.release();
  }
  for (auto& e : H->ev)
    if (e) (void)hipEventDestroy(e);
  if (H->stream) (void)hipStreamDestroy(H->stream);
  delete H;
}

SIFT_API int sift_extract(sift_handle* H, const uint8_t* grey, int32_t width, int32_t height, const sift_options* options) {
  return Guard([&] {
    if (!H || !options) throw Fail("sift_extract: null handle or options");
    const auto t0 = std::chrono::steady_clock::now();
    H->num_octaves = 0;  // a failed call leaves no result behind
    H->keypoints.clear();
    H->float_desc.clear();
    H->desc.clear();
    Extract(H, grey, width, height, *options);
    g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
}

SIFT_API int64_t sift_num_features(sift_handle* H) { return H ? (int64_t)(H->keypoints.size() / 4) : 0; }

SIFT_API int sift_copy_keypoints(sift_handle* H, float* out, int64_t capacity_rows) {
  return Guard([&] {
    if (!H || (!out && !H->keypoints.empty())) throw Fail("sift_copy_keypoints: null argument");
    if (capacity_rows < sift_num_features(H)) throw Fail("sift_copy_keypoints: capacity below sift_num_features");
    if (!H->keypoints.empty()) std::memcpy(out, H->keypoints.data(), H->keypoints.size() * sizeof(float));
  });
}

SIFT_API int sift_copy_descriptors(sift_handle* H, uint8_t* out, int64_t capacity_rows) {
  return Guard([&] {
    if (!H || (!out && !H->desc.empty())) throw Fail("sift_copy_descriptors: null argument");
    if (capacity_rows < sift_num_features(H)) throw Fail("sift_copy_descriptors: capacity below sift_num_features");
    if (!H->desc.empty()) std::memcpy(out, H->desc.data(), H->desc.size());
  });
}

SIFT_API int sift_copy_float_descriptors(sift_handle* H, float* out, int64_t capacity_rows) {
  return Guard([&] {
    if (!H || (!out && !H->float_desc.empty())) throw Fail("sift_copy_float_descriptors: null argument");
    if (capacity_rows < sift_num_features(H)) throw Fail("sift_copy_float_descriptors: capacity below sift_num_features");
    if (!H->float_desc.empty()) std::memcpy(out, H->float_desc.data(), H->float_desc.size() * sizeof(float));
  });
}

SIFT_API int32_t sift_num_octaves(sift_handle* H) { return H ? H->num_octaves : 0; }

SIFT_API int sift_octave_info(sift_handle* H, int32_t k, int32_t* width, int32_t* height, int32_t* o) {
  return Guard([&] {
    const Octave& oc = OctaveOf(H, k);
    if (width) *width = oc.w;
    if (height) *height = oc.h;
    if (o) *o = oc.o;
  });
}

SIFT_API int sift_copy_level(sift_handle* H, int32_t k, int32_t level, float* out) {
  return Guard([&] {
    const Octave& oc = OctaveOf(H, k);
    if (level < 0 || level >= H->geom.num_levels() || !out) throw Fail("sift_copy_level: level out of range or null output");
    const size_t plane = (size_t)oc.w * oc.h;
    SIFT_HIP(hipSetDevice(H->gpu));
    SIFT_HIP(hipMemcpy(out, oc.levels.as<float>() + plane * level, plane * sizeof(float), hipMemcpyDeviceToHost));
  });
}

SIFT_API int sift_copy_dog(sift_handle* H, int32_t k, int32_t level, float* out) {
  return Guard([&] {
    const Octave& oc = OctaveOf(H, k);
    if (level < 0 || level >= H->geom.num_dog() || !out) throw Fail("sift_copy_dog: level out of range or null output");
    const size_t plane = (size_t)oc.w * oc.h;
    SIFT_HIP(hipSetDevice(H->gpu));
    SIFT_HIP(hipMemcpy(out, oc.dog.as<float>() + plane * level, plane * sizeof(float), hipMemcpyDeviceToHost));
  });
}

SIFT_API int sift_copy_gradient(sift_handle* H, int32_t k, int32_t p, float* out) {
  return Guard([&] {
    const Octave& oc = OctaveOf(H, k);
    if (p < 0 || p >= H->geom.num_grad() || !out) throw Fail("sift_copy_gradient: plane out of range or null output");
    if (oc.detections.empty()) throw Fail("sift_copy_gradient: the planes of an octave without a detection are not made");
    const size_t plane = (size_t)oc.w * oc.h * 2;
    SIFT_HIP(hipSetDevice(H->gpu));
    SIFT_HIP(hipMemcpy(out, oc.grad.as<float>() + plane * p, plane * sizeof(float), hipMemcpyDeviceToHost));
  });
}

SIFT_API int64_t sift_num_candidates(sift_handle* H, int32_t k) { return (H && k >= 0 && k < H->num_octaves) ? H->octaves[k].num_candidates : -1; }

SIFT_API int64_t sift_num_detections(sift_handle* H, int32_t k) {
  return (H && k >= 0 && k < H->num_octaves) ? (int64_t)H->octaves[k].detections.size() : -1;
}

SIFT_API int sift_copy_detections(sift_handle* H, int32_t k, sift_detection* out, int64_t capacity) {
  return Guard([&] {
    const Octave& oc = OctaveOf(H, k);
    if (capacity < (int64_t)oc.detections.size() || (!out && !oc.detections.empty())) throw Fail("sift_copy_detections: capacity too small");
    if (!oc.detections.empty()) std::memcpy(out, oc.detections.data(), oc.detections.size() * sizeof(sift_detection));
  });
}

SIFT_API int sift_copy_orientations(sift_handle* H, int32_t k, int32_t* counts, double* angles, int64_t capacity) {
  return Guard([&] {
    const Octave& oc = OctaveOf(H, k);
    if (capacity < (int64_t)oc.ori_counts.size() || ((!counts || !angles) && !oc.ori_counts.empty()))
      throw Fail("sift_copy_orientations: capacity too small");
    if (!oc.ori_counts.empty()) {
      std::memcpy(counts, oc.ori_counts.data(), oc.ori_counts.size() * sizeof(int32_t));
      std::memcpy(angles, oc.ori_angles.data(), oc.ori_angles.size() * sizeof(double));
    }
  });
}

SIFT_API void sift_conv_tile(int32_t pass, int32_t* tile_x, int32_t* tile_y) {
  *tile_x = pass == 0 ? sp::kColTileX : sp::kRowTileX;
  *tile_y = pass == 0 ? sp::kColTileY : sp::kRowTileY;
}

SIFT_API int32_t sift_halo_limit(void) { return sp::kHaloLimit; }
SIFT_API int32_t sift_candidate_capacity(int32_t w, int32_t h, int32_t S) { return sp::candidate_capacity(w, h, S); }
SIFT_API int32_t sift_grown_capacity(int32_t count) { return sp::grown_capacity(count); }
SIFT_API void sift_set_candidate_capacity(sift_handle* H, int32_t capacity) {
  if (H) H->forced_capacity = capacity > 0 ? capacity : 0;
}
SIFT_API int64_t sift_num_reruns(sift_handle* H) { return H ? H->reruns : 0; }

SIFT_API void sift_last_timing(double* event_ms, double* total_ms, double* stage_ms) {
  if (event_ms) *event_ms = g_event_ms;
  if (total_ms) *total_ms = g_total_ms;
  if (stage_ms)
    for (int s = 0; s < SIFT_NUM_STAGES; ++s) stage_ms[s] = g_stage_ms[s];
}

SIFT_API const char* sift_last_error(void) { return g_error.c_str(); }

}  // extern "C"
