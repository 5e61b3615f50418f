// model_stats.hip -- the statistics of a dense-stage model on gfx950 behind include/colmap_amd_model.h: depth ranges,
// shared-point counts, percentile triangulation angles and the overlap lists made of them (reference mvs/model.cc:120-277).
//
// Passes (the host decisions -- checks, orders, classes, limits -- are model_plan.h):
//   model_image_kernel        one lane per image: projection centre C = -R^T T in float, widened to double
//                             (ComputeProjectionCenter, mvs/image.cc:137-142; model.cc:239-245).
//   model_depth_kernel        one lane per observation, in the plan's by-image order: depth = R.row(2) . X + T[2] in float
//                             (model.cc:184-186), written as its bit pattern into the image's segment; a depth that is not
//                             > 0 is written as kNoDepth, which orders after every float.
//   model_pair_kernel<G, 0>   one point per group of G lanes (1, 16 or 64 by track length): every pair of track positions
//                             i > j with different images does one integer atomicAdd on its cell (min, max) of the dense
//                             upper-triangular count table.
//   model_scan_*              exclusive scan of the cells in 64 bits: where the angles of a cell begin.
//   model_pair_kernel<G, 1>   the same walk: CalculateTriangulationAngle (geometry/triangulation.cc:217-249) in double,
//                             narrowed to float, stored at offset[cell] + atomicAdd(cursor[cell], 1). The arrival order
//                             inside a cell differs from run to run; nothing below depends on it.
//   model_select_*_kernel     order statistics of a segment -- the positive depths of an image, the angles of a cell.
//                             Non-negative floats order like their bit patterns. Up to 64 values: one wave, one value per
//                             lane, rank = number of smaller values, equal bits broken by position. More: one workgroup, a
//                             most-significant-byte-first radix select over 256-bin LDS histograms (integer atomics).
//                             Either way the result is the bit pattern of the k-th smallest value, a function of the
//                             multiset alone. Depth ranges take the elements (size_t)(n * 0.01f) and (size_t)(n * 0.99f)
//                             and stretch them by 0.75f / 1.25f; angles take colmap::Percentile (math/math.h:205-224).
//   model_overlap_kernel      one workgroup per image: the row's cells with a count and a percentile angle >= the
//                             threshold, ranked by (count descending, image index ascending) -- the key is unique, so the
//                             candidate of rank r < K writes slot r, no atomic.
// Every count is an integer and no float is added atomically: the outputs are the same bytes on every run.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_model.h"
#include "model_plan.h"

#define MODEL_API __attribute__((visibility("default")))

struct model_pairs {
  int32_t num_images = 0;
  std::vector<int64_t> row_offsets;
  std::vector<int32_t> other, count;
  std::vector<float> angle;
};

namespace {

namespace mp = model_plan;

thread_local std::string g_error;
thread_local double g_kernel_ms = 0.0, g_total_ms = 0.0;

using Fail = mp::Fail;
#define MODEL_HIP(call)                                                                  \
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
constexpr int kScanItems = 8;                                 // cells per lane of a scan workgroup
constexpr unsigned kNoDepth = 0xFFFFFFFFu;                    // orders after the bits of every float
constexpr double kPi = 3.14159265358979323846;
constexpr double kDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;  // DegToRad, math/math.h
enum Kind : int { KIND_DEPTH = 0, KIND_PERCENTILE = 1 };

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void model_image_kernel(const float* __restrict__ R, const float* __restrict__ T,
                                                              int num_images, double* __restrict__ centres) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_images) return;
  const float* r = R + (size_t)9 * i;
  const float* t = T + (size_t)3 * i;
  for (int k = 0; k < 3; ++k) {
    const float c = -((r[k] * t[0] + r[3 + k] * t[1]) + r[6 + k] * t[2]);
    centres[(size_t)3 * i + k] = (double)c;
  }
}

__global__ __launch_bounds__(kBlock) void model_depth_kernel(const float* __restrict__ R, const float* __restrict__ T,
                                                              const float* __restrict__ points,
                                                              const int* __restrict__ track_image,
                                                              const int* __restrict__ obs_order,
                                                              const int* __restrict__ obs_point, int num_obs,
                                                              unsigned* __restrict__ depth_bits) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= num_obs) return;
  const int o = obs_order[t];
  const int img = track_image[o];
  const float* r = R + (size_t)9 * img;
  const float* X = points + (size_t)3 * obs_point[o];
  const float depth = ((r[6] * X[0] + r[7] * X[1]) + r[8] * X[2]) + T[(size_t)3 * img + 2];
  depth_bits[t] = depth > 0.0f ? __float_as_uint(depth) : kNoDepth;
}

// CalculateTriangulationAngle (geometry/triangulation.cc:217-249) of the rays X - c1, X - c2
__device__ __forceinline__ double triangulation_angle(const double v1[3], const double v2[3]) {
  const double n1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
  const double n2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  double angle = 0.0;
  if (!(n1 == 0.0 || n2 == 0.0)) {
    const double c = (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) / sqrt(n1 * n2);
    angle = acos(fmin(fmax(c, -1.0), 1.0));
  }
  return fmin(angle, kPi - angle);
}

struct PairArgs {
  const long long* track_offsets;
  const int* track_image;
  const float* points;
  const double* centres;
  int* counts;                      // [cells] pass 0 adds to it
  const long long* cell_offsets;    // [cells + 1] pass 1: where a cell's angles begin
  int* cursor;                      // [cells] pass 1: zero on entry
  unsigned* angles;                 // pass 1: float bit patterns
  int num_images;
};

template <int G, int ANGLE>
__global__ __launch_bounds__(kBlock) void model_pair_kernel(PairArgs a, const int* __restrict__ class_points,
                                                             int num_class_points) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long group = tid / G;
  const int gl = (int)(tid % G);
  if (group >= num_class_points) return;  // no cross-lane operation below
  const int p = class_points[group];
  const long long begin = a.track_offsets[p];
  const int L = (int)(a.track_offsets[p + 1] - begin);
  const long long I = a.num_images;
  double X[3] = {0.0, 0.0, 0.0};
  if (ANGLE) {
    X[0] = (double)a.points[(size_t)3 * p];
    X[1] = (double)a.points[(size_t)3 * p + 1];
    X[2] = (double)a.points[(size_t)3 * p + 2];
  }
  for (int i = gl; i < L; i += G) {
    const int im1 = a.track_image[begin + i];
    double v1[3] = {0.0, 0.0, 0.0};
    if (ANGLE) {
      const double* c1 = a.centres + (size_t)3 * im1;
      v1[0] = X[0] - c1[0]; v1[1] = X[1] - c1[1]; v1[2] = X[2] - c1[2];
    }
    for (int j = 0; j < i; ++j) {
      const int im2 = a.track_image[begin + j];
      if (im1 == im2) continue;
      const long long lo = im1 < im2 ? im1 : im2, hi = im1 < im2 ? im2 : im1;
      const long long cell = lo * (2 * I - lo - 1) / 2 + (hi - lo - 1);  // model_plan::cell_index
      if (!ANGLE) {
        atomicAdd(&a.counts[cell], 1);
      } else {
        const double* c2 = a.centres + (size_t)3 * im2;
        const double v2[3] = {X[0] - c2[0], X[1] - c2[1], X[2] - c2[2]};
        const float angle = (float)triangulation_angle(v1, v2);
        const int slot = atomicAdd(&a.cursor[cell], 1);  // < counts[cell]: the count pass made the same walk
        a.angles[a.cell_offsets[cell] + slot] = __float_as_uint(angle);
      }
    }
  }
}

// Exclusive scan of one value per lane over the workgroup (every lane calls it); *total is the workgroup's sum.
__device__ __forceinline__ long long block_exclusive_scan(long long v, long long* s, long long* total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    const long long t = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  const long long inclusive = s[tid];
  *total = s[kBlock - 1];
  __syncthreads();  // s may be written again
  return inclusive - v;
}

// a workgroup covers kBlock * kScanItems consecutive cells: its sum
__global__ __launch_bounds__(kBlock) void model_scan_sums_kernel(const int* __restrict__ counts, long long num_cells,
                                                                  long long* __restrict__ block_sums) {
  __shared__ long long s[kBlock];
  const long long first = ((long long)blockIdx.x * kBlock + threadIdx.x) * kScanItems;
  long long v = 0;
  for (int k = 0; k < kScanItems; ++k)
    if (first + k < num_cells) v += counts[first + k];
  long long total;
  block_exclusive_scan(v, s, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: the sums of all workgroups, in place, to their exclusive scan; block_sums[num_blocks] = the total
__global__ __launch_bounds__(kBlock) void model_scan_blocks_kernel(long long* __restrict__ block_sums, int num_blocks) {
  __shared__ long long s[kBlock];
  long long carry = 0;
  for (int base = 0; base < num_blocks; base += kBlock) {
    const int b = base + threadIdx.x;
    const long long v = b < num_blocks ? block_sums[b] : 0;
    long long total;
    const long long ex = block_exclusive_scan(v, s, &total);
    if (b < num_blocks) block_sums[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) block_sums[num_blocks] = carry;
}

__global__ __launch_bounds__(kBlock) void model_scan_apply_kernel(const int* __restrict__ counts, long long num_cells,
                                                                   const long long* __restrict__ block_sums,
                                                                   long long* __restrict__ cell_offsets) {
  __shared__ long long s[kBlock];
  const long long first = ((long long)blockIdx.x * kBlock + threadIdx.x) * kScanItems;
  long long v = 0;
  for (int k = 0; k < kScanItems; ++k)
    if (first + k < num_cells) v += counts[first + k];
  long long total;
  long long run = block_sums[blockIdx.x] + block_exclusive_scan(v, s, &total);
  for (int k = 0; k < kScanItems; ++k)
    if (first + k < num_cells) {
      cell_offsets[first + k] = run;
      run += counts[first + k];
      if (first + k == num_cells - 1) cell_offsets[num_cells] = run;
    }
}

// The order statistics a segment of n values needs (left <= right), and what becomes of them.
__device__ __forceinline__ void select_picks(int kind, int n, double percentile, int* left, int* right) {
  if (n <= 0) {
    *left = *right = 0;
  } else if (kind == KIND_DEPTH) {  // image_depths[size * 0.01f], image_depths[size * 0.99f] (model.cc:207-210)
    *left = (int)(size_t)((float)n * 0.01f);
    *right = (int)(size_t)((float)n * 0.99f);
  } else {  // Percentile (math/math.h:209-213)
    const double idx = percentile / 100. * (double)(n - 1);
    *left = (int)floor(idx);
    *right = (int)ceil(idx);
  }
}

__device__ __forceinline__ void select_finish(int kind, int id, int n, double percentile, unsigned left, unsigned right,
                                              float* __restrict__ out) {
  if (kind == KIND_DEPTH) {
    if (n <= 0) {
      out[(size_t)2 * id] = -1.0f;
      out[(size_t)2 * id + 1] = -1.0f;
    } else {  // stretched by kStretchRatio (model.cc:212-214)
      out[(size_t)2 * id] = __uint_as_float(left) * 0.75f;
      out[(size_t)2 * id + 1] = __uint_as_float(right) * 1.25f;
    }
    return;
  }
  const double idx = percentile / 100. * (double)(n - 1);
  const double l = floor(idx), r = ceil(idx);
  double result = (double)__uint_as_float(right);
  if (l != r) result = (r - idx) * (double)__uint_as_float(left) + (idx - l) * result;
  out[id] = (float)result;
}

// Segments of up to 64 values, one wave each: lane l holds value l and counts the values that come before it.
__global__ __launch_bounds__(kBlock) void model_select_wave_kernel(const unsigned* __restrict__ values,
                                                                    const long long* __restrict__ offsets,
                                                                    const int* __restrict__ ids, int num_ids, int kind,
                                                                    double percentile, float* __restrict__ out) {
  const int seg = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / 64);
  const int lane = threadIdx.x & 63;
  if (seg >= num_ids) return;  // the whole wave leaves
  const int id = ids[seg];
  const long long begin = offsets[id];
  const int len = (int)(offsets[id + 1] - begin);  // <= 64 (model_plan::select_class)
  const unsigned* v = values + begin;
  const bool has = lane < len;
  const unsigned e = has ? v[lane] : kNoDepth;
  int rank = 0;
  for (int j = 0; j < len; ++j) {
    const unsigned u = v[j];
    rank += (u < e || (u == e && j < lane)) ? 1 : 0;
  }
  const int n = kind == KIND_DEPTH ? __popcll(__ballot(has && e != kNoDepth ? 1 : 0)) : len;
  int kl, kr;
  select_picks(kind, n, percentile, &kl, &kr);
  const unsigned long long bl = __ballot(has && rank == kl ? 1 : 0), br = __ballot(has && rank == kr ? 1 : 0);
  const unsigned left = (unsigned)__shfl((int)e, bl ? __ffsll((long long)bl) - 1 : 0);
  const unsigned right = (unsigned)__shfl((int)e, br ? __ffsll((long long)br) - 1 : 0);
  if (lane == 0) select_finish(kind, id, n, percentile, left, right, out);
}

// The k-th smallest (k < n) of v[0 .. n) by a radix select, most significant byte first; every lane of the workgroup
// calls it and gets the value. hist: 256 words of LDS, pick: 2.
__device__ __forceinline__ unsigned radix_select(const unsigned* __restrict__ v, int n, int k, unsigned* hist, unsigned* pick) {
  const int tid = threadIdx.x;
  unsigned prefix = 0u, mask = 0u, rest = (unsigned)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;  // kBlock == 256 bins
    __syncthreads();
    for (int i = tid; i < n; i += kBlock) {
      const unsigned u = v[i];
      if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned below = 0u, digit = 255u;
      for (unsigned b = 0; b < 256u; ++b) {
        if (rest < below + hist[b]) {
          digit = b;
          break;
        }
        below += hist[b];
      }
      pick[0] = digit;
      pick[1] = rest - below;
    }
    __syncthreads();
    prefix |= pick[0] << shift;
    mask |= 255u << shift;
    rest = pick[1];
  }
  __syncthreads();  // pick and hist may be written again
  return prefix;
}

__global__ __launch_bounds__(kBlock) void model_select_block_kernel(const unsigned* __restrict__ values,
                                                                     const long long* __restrict__ offsets,
                                                                     const int* __restrict__ ids, int kind,
                                                                     double percentile, float* __restrict__ out) {
  __shared__ unsigned hist[256];
  __shared__ unsigned pick[2];
  __shared__ int positive;
  const int id = ids[blockIdx.x];
  const long long begin = offsets[id];
  const int len = (int)(offsets[id + 1] - begin);
  const unsigned* v = values + begin;
  int n = len;
  if (kind == KIND_DEPTH) {
    if (threadIdx.x == 0) positive = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < len; i += kBlock) mine += v[i] != kNoDepth ? 1 : 0;
    if (mine) atomicAdd(&positive, mine);
    __syncthreads();
    n = positive;
  }
  int kl, kr;
  select_picks(kind, n, percentile, &kl, &kr);
  const unsigned right = radix_select(v, len, kr, hist, pick);
  const unsigned left = kl == kr ? right : radix_select(v, len, kl, hist, pick);
  if (threadIdx.x == 0) select_finish(kind, id, n, percentile, left, right, out);
}

__global__ __launch_bounds__(kBlock) void model_overlap_kernel(const int* __restrict__ counts,
                                                                const float* __restrict__ cell_angle, int num_images,
                                                                float min_rad, int K, int* __restrict__ rows,
                                                                int* __restrict__ row_count) {
  __shared__ unsigned shared_count[mp::kMaxImages];  // of the row's candidates, 0 for every other image
  __shared__ int candidates;
  const int i = blockIdx.x;
  const long long I = num_images;
  if (threadIdx.x == 0) candidates = 0;
  __syncthreads();
  int mine = 0;
  for (int j = threadIdx.x; j < num_images; j += kBlock) {
    unsigned c = 0u;
    if (j != i) {
      const long long lo = j < i ? j : i, hi = j < i ? i : j;
      const long long cell = lo * (2 * I - lo - 1) / 2 + (hi - lo - 1);
      const int n = counts[cell];
      if (n > 0 && cell_angle[cell] >= min_rad) {
        c = (unsigned)n;
        ++mine;
      }
    }
    shared_count[j] = c;
  }
  if (mine) atomicAdd(&candidates, mine);
  __syncthreads();
  for (int j = threadIdx.x; j < num_images; j += kBlock) {
    const unsigned c = shared_count[j];
    if (c == 0u) continue;
    int rank = 0;
    for (int b = 0; b < num_images; ++b) {
      const unsigned u = shared_count[b];
      rank += (u > c || (u == c && b < j)) ? 1 : 0;
    }
    if (rank < K) rows[(size_t)i * K + rank] = j;
  }
  if (threadIdx.x == 0) row_count[i] = candidates < K ? candidates : K;
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

void bind_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Fail("no HIP device available: the model statistics run on the GPU (there is no CPU path)");
  if (!(gpu_index >= 0 && gpu_index < ndev)) throw Fail("gpu_index " + std::to_string(gpu_index) + " out of range");
  MODEL_HIP(hipSetDevice(gpu_index));
}

int64_t free_device_bytes() {
  size_t free_bytes = 0, total = 0;
  MODEL_HIP(hipMemGetInfo(&free_bytes, &total));
  return (int64_t)free_bytes;
}

template <typename T>
struct DeviceBuffer {
  T* p = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  void alloc(size_t n) {
    if (n == 0) return;
    MODEL_HIP(hipMalloc((void**)&p, n * sizeof(T)));
  }
  void zero(size_t n) {
    alloc(n);
    if (n) MODEL_HIP(hipMemset(p, 0, n * sizeof(T)));
  }
  void upload(const T* host, size_t n) {
    alloc(n);
    if (n) MODEL_HIP(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
  }
  void download(T* host, size_t n) const {
    if (n && host) MODEL_HIP(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost));
  }
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};

// the kernels between start() and stop(), added up over the intervals of a call
struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  double ms = 0.0;
  Timer() {
    MODEL_HIP(hipEventCreate(&a));
    MODEL_HIP(hipEventCreate(&b));
  }
  void start() { MODEL_HIP(hipEventRecord(a, 0)); }
  void stop() {
    MODEL_HIP(hipEventRecord(b, 0));
    MODEL_HIP(hipEventSynchronize(b));
    float t = 0.0f;
    MODEL_HIP(hipEventElapsedTime(&t, a, b));
    ms += t;
  }
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

// both selection kernels over the segments `offsets` delimits in `values`
void launch_select(const unsigned* values, const long long* offsets, const std::vector<int32_t> ids[2],
                   DeviceBuffer<int> d_ids[2], int kind, double percentile, float* out) {
  for (int k = 0; k < 2; ++k) {
    const size_t n = ids[k].size();
    if (n == 0) continue;
    if (k == 0)
      hipLaunchKernelGGL(model_select_wave_kernel, dim3(blocks_for(n * 64)), dim3(kBlock), 0, 0, values, offsets,
                         d_ids[k].p, (int)n, kind, percentile, out);
    else
      hipLaunchKernelGGL(model_select_block_kernel, dim3((unsigned)n), dim3(kBlock), 0, 0, values, offsets, d_ids[k].p, kind,
                         percentile, out);
    MODEL_HIP(hipGetLastError());
  }
}

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

void depth_ranges(const model_flat* model, float* ranges, int gpu_index) {
  if (!model) throw Fail("null argument");
  mp::validate(*model);
  const model_flat& m = *model;
  MODEL_CHECK(m.num_images == 0 || ranges, "ranges is null (it has 2 * num_images entries)");
  bind_device(gpu_index);
  const Clock clock;
  const size_t I = (size_t)m.num_images, P = (size_t)m.num_points, O = (size_t)m.num_observations;
  g_kernel_ms = 0.0;
  if (I == 0) {
    g_total_ms = clock.ms();
    return;
  }
  const mp::DepthPlan plan = mp::make_depth_plan(m);
  mp::check_device_memory(mp::device_bytes_depth(m), free_device_bytes());

  DeviceBuffer<float> d_R, d_T, d_points, d_ranges;
  DeviceBuffer<int> d_track_image, d_order, d_obs_point, d_ids[2];
  DeviceBuffer<long long> d_image_offsets;
  DeviceBuffer<unsigned> d_bits;
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are uploaded as they are");
  d_R.upload(m.R, 9 * I);
  d_T.upload(m.T, 3 * I);
  d_points.upload(m.points, 3 * P);
  d_track_image.upload(m.track_image, O);
  d_order.upload(plan.obs_order.data(), O);
  d_obs_point.upload(plan.obs_point.data(), O);
  d_image_offsets.upload((const long long*)plan.image_offsets.data(), I + 1);
  for (int k = 0; k < 2; ++k) d_ids[k].upload(plan.select_ids[k].data(), plan.select_ids[k].size());
  d_bits.alloc(O);
  d_ranges.alloc(2 * I);

  Timer timer;
  timer.start();
  if (O > 0) {
    hipLaunchKernelGGL(model_depth_kernel, dim3(blocks_for(O)), dim3(kBlock), 0, 0, d_R.p, d_T.p, d_points.p,
                       d_track_image.p, d_order.p, d_obs_point.p, (int)O, d_bits.p);
    MODEL_HIP(hipGetLastError());
  }
  launch_select(d_bits.p, d_image_offsets.p, plan.select_ids, d_ids, KIND_DEPTH, 0.0, d_ranges.p);
  timer.stop();
  d_ranges.download(ranges, 2 * I);
  g_kernel_ms = timer.ms;
  g_total_ms = clock.ms();
}

// the pair table of a model: counts and percentile angles per cell, on the host and (for the overlap pass) the device
struct PairTables {
  int64_t num_cells = 0;
  std::vector<int32_t> counts;
  std::vector<float> angles;
  DeviceBuffer<int> d_counts;
  DeviceBuffer<float> d_cell_angle;
};

// of a validated model, on the bound device
void pair_tables(const model_flat& m, double percentile, bool want_host_angles, PairTables* t, Timer* timer) {
  const mp::PairPlan plan = mp::make_pair_plan(m);
  const size_t I = (size_t)m.num_images, P = (size_t)m.num_points, O = (size_t)m.num_observations;
  const size_t cells = (size_t)plan.num_cells;
  t->num_cells = plan.num_cells;
  if (cells == 0) return;
  mp::check_device_memory(mp::device_bytes_pairs(m, plan, 0), free_device_bytes());

  DeviceBuffer<float> d_R, d_T, d_points;
  DeviceBuffer<double> d_centres;
  DeviceBuffer<long long> d_track_offsets, d_cell_offsets, d_block_sums;
  DeviceBuffer<int> d_track_image, d_class[mp::kNumClasses], d_cursor, d_ids[2];
  DeviceBuffer<unsigned> d_angles;
  d_R.upload(m.R, 9 * I);
  d_T.upload(m.T, 3 * I);
  d_points.upload(m.points, 3 * P);
  d_track_offsets.upload((const long long*)m.track_offsets, P + 1);
  d_track_image.upload(m.track_image, O);
  for (int k = 0; k < mp::kNumClasses; ++k) d_class[k].upload(plan.class_points[k].data(), plan.class_points[k].size());
  d_centres.alloc(3 * I);
  t->d_counts.zero(cells);
  t->d_cell_angle.alloc(cells);
  d_cell_offsets.alloc(cells + 1);
  const unsigned scan_blocks = blocks_for((cells + kScanItems - 1) / kScanItems);
  d_block_sums.alloc((size_t)scan_blocks + 1);

  PairArgs a;
  a.track_offsets = d_track_offsets.p;
  a.track_image = d_track_image.p;
  a.points = d_points.p;
  a.centres = d_centres.p;
  a.counts = t->d_counts.p;
  a.cell_offsets = d_cell_offsets.p;
  a.cursor = nullptr;
  a.angles = nullptr;
  a.num_images = (int)I;
  auto launch_pairs = [&](int angle_pass) {
    for (int k = 0; k < mp::kNumClasses; ++k) {
      const size_t n = plan.class_points[k].size();
      if (n == 0) continue;
      const dim3 grid(blocks_for(n * (size_t)mp::kClassWidth[k])), block(kBlock);
      if (k == 0 && !angle_pass) hipLaunchKernelGGL((model_pair_kernel<1, 0>), grid, block, 0, 0, a, d_class[k].p, (int)n);
      else if (k == 1 && !angle_pass) hipLaunchKernelGGL((model_pair_kernel<16, 0>), grid, block, 0, 0, a, d_class[k].p, (int)n);
      else if (!angle_pass) hipLaunchKernelGGL((model_pair_kernel<64, 0>), grid, block, 0, 0, a, d_class[k].p, (int)n);
      else if (k == 0) hipLaunchKernelGGL((model_pair_kernel<1, 1>), grid, block, 0, 0, a, d_class[k].p, (int)n);
      else if (k == 1) hipLaunchKernelGGL((model_pair_kernel<16, 1>), grid, block, 0, 0, a, d_class[k].p, (int)n);
      else hipLaunchKernelGGL((model_pair_kernel<64, 1>), grid, block, 0, 0, a, d_class[k].p, (int)n);
      MODEL_HIP(hipGetLastError());
    }
  };

  timer->start();
  hipLaunchKernelGGL(model_image_kernel, dim3(blocks_for(I)), dim3(kBlock), 0, 0, d_R.p, d_T.p, (int)I, d_centres.p);
  MODEL_HIP(hipGetLastError());
  launch_pairs(0);
  hipLaunchKernelGGL(model_scan_sums_kernel, dim3(scan_blocks), dim3(kBlock), 0, 0, t->d_counts.p, (long long)cells, d_block_sums.p);
  MODEL_HIP(hipGetLastError());
  hipLaunchKernelGGL(model_scan_blocks_kernel, dim3(1), dim3(kBlock), 0, 0, d_block_sums.p, (int)scan_blocks);
  MODEL_HIP(hipGetLastError());
  hipLaunchKernelGGL(model_scan_apply_kernel, dim3(scan_blocks), dim3(kBlock), 0, 0, t->d_counts.p, (long long)cells,
                     d_block_sums.p, d_cell_offsets.p);
  MODEL_HIP(hipGetLastError());
  timer->stop();

  // the counts are part of the result, and they say which cells hold a segment and of which selection class
  t->counts.resize(cells);
  t->d_counts.download(t->counts.data(), cells);
  const mp::CellSegments segments = mp::make_cell_segments(t->counts.data(), plan.num_cells);
  if (segments.pairs > 0) {
    mp::check_device_memory(segments.pairs * 4 + (int64_t)cells * 4, free_device_bytes());
    d_angles.alloc((size_t)segments.pairs);
    d_cursor.zero(cells);
    for (int k = 0; k < 2; ++k) d_ids[k].upload(segments.select_ids[k].data(), segments.select_ids[k].size());
    a.cursor = d_cursor.p;
    a.angles = d_angles.p;
    timer->start();
    launch_pairs(1);
    launch_select(d_angles.p, d_cell_offsets.p, segments.select_ids, d_ids, KIND_PERCENTILE, percentile, t->d_cell_angle.p);
    timer->stop();
  }
  if (want_host_angles) {
    t->angles.resize(cells);
    t->d_cell_angle.download(t->angles.data(), cells);  // the empty cells hold no value and are never read
  }
}

void pair_statistics(const model_flat* model, double percentile, model_pairs** out, int gpu_index) {
  if (!model || !out) throw Fail("null argument");
  *out = nullptr;
  mp::validate(*model);
  mp::validate_percentile(percentile);
  bind_device(gpu_index);
  const Clock clock;
  Timer timer;
  PairTables t;
  pair_tables(*model, percentile, true, &t, &timer);
  model_pairs* r = new model_pairs();
  r->num_images = model->num_images;
  mp::make_rows(t.counts.data(), t.angles.data(), model->num_images, &r->row_offsets, &r->other, &r->count, &r->angle);
  *out = r;
  g_kernel_ms = timer.ms;
  g_total_ms = clock.ms();
}

void max_overlapping_images(const model_flat* model, int64_t wanted, double min_angle_deg, int64_t* ptr, int32_t* idx,
                            size_t* total, int gpu_index) {
  if (!model || !total) throw Fail("null argument");
  mp::validate(*model);
  MODEL_CHECK(wanted >= 0, "num_images_wanted must not be negative");
  MODEL_CHECK((ptr == nullptr) == (idx == nullptr), "ptr and idx are given together, or both null to query the total");
  bind_device(gpu_index);
  const Clock clock;
  Timer timer;
  const size_t I = (size_t)model->num_images;
  const float min_rad = (float)(min_angle_deg * kDegToRad);  // const float ... = DegToRad(double) (model.cc:124)
  PairTables t;
  pair_tables(*model, 75.0, false, &t, &timer);  // kTriangulationAnglePercentile (model.cc:128)
  const int K = (int)(wanted < (int64_t)I ? wanted : (int64_t)I);  // a row has at most num_images - 1 candidates
  std::vector<int> rows(I * (size_t)K), row_count(I, 0);
  if (t.num_cells > 0) {
    mp::check_device_memory((int64_t)(I * (size_t)K + I) * 4, free_device_bytes());
    DeviceBuffer<int> d_rows, d_row_count;
    d_rows.alloc(I * (size_t)K);
    d_row_count.alloc(I);
    timer.start();
    hipLaunchKernelGGL(model_overlap_kernel, dim3((unsigned)I), dim3(kBlock), 0, 0, t.d_counts.p, t.d_cell_angle.p, (int)I,
                       min_rad, K, d_rows.p, d_row_count.p);
    MODEL_HIP(hipGetLastError());
    timer.stop();
    d_rows.download(rows.data(), rows.size());
    d_row_count.download(row_count.data(), I);
  }
  size_t sum = 0;
  for (size_t i = 0; i < I; ++i) sum += (size_t)row_count[i];
  *total = sum;
  if (ptr) {
    ptr[0] = 0;
    for (size_t i = 0; i < I; ++i) {
      for (int r = 0; r < row_count[i]; ++r) idx[ptr[i] + r] = rows[i * (size_t)K + (size_t)r];
      ptr[i + 1] = ptr[i] + row_count[i];
    }
  }
  g_kernel_ms = timer.ms;
  g_total_ms = clock.ms();
}

}  // namespace

extern "C" {

MODEL_API int model_compute_depth_ranges(const model_flat* model, float* ranges, int32_t gpu_index) {
  return Guard([&] { depth_ranges(model, ranges, gpu_index); });
}

MODEL_API int model_compute_pair_statistics(const model_flat* model, double percentile, model_pairs** out,
                                            int32_t gpu_index) {
  return Guard([&] { pair_statistics(model, percentile, out, gpu_index); });
}

MODEL_API void model_pairs_size(const model_pairs* pairs, int32_t* num_images, size_t* num_entries) {
  if (num_images) *num_images = pairs ? pairs->num_images : 0;
  if (num_entries) *num_entries = pairs ? pairs->other.size() : 0;
}

MODEL_API void model_pairs_get(const model_pairs* pairs, int64_t* row_offsets, int32_t* other, int32_t* count,
                               float* angle) {
  if (!pairs) return;
  const size_t n = pairs->other.size();
  if (row_offsets) std::memcpy(row_offsets, pairs->row_offsets.data(), pairs->row_offsets.size() * sizeof(int64_t));
  if (other && n) std::memcpy(other, pairs->other.data(), n * sizeof(int32_t));
  if (count && n) std::memcpy(count, pairs->count.data(), n * sizeof(int32_t));
  if (angle && n) std::memcpy(angle, pairs->angle.data(), n * sizeof(float));
}

MODEL_API void model_pairs_free(model_pairs* pairs) { delete pairs; }

MODEL_API int model_get_max_overlapping_images(const model_flat* model, int64_t num_images_wanted,
                                               double min_triangulation_angle_deg, int64_t* ptr, int32_t* idx,
                                               size_t* total, int32_t gpu_index) {
  return Guard([&] { max_overlapping_images(model, num_images_wanted, min_triangulation_angle_deg, ptr, idx, total, gpu_index); });
}

MODEL_API void model_last_timing(double* kernel_ms, double* total_ms) {
  if (kernel_ms) *kernel_ms = g_kernel_ms;
  if (total_ms) *total_ms = g_total_ms;
}

MODEL_API const char* model_last_error(void) { return g_error.c_str(); }

}  // extern "C"
