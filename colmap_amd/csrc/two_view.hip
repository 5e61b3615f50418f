// two_view.hip -- two-view geometry estimation on gfx950 behind include/colmap_amd_tvg.h: minimal solvers for batches of
// samples and the scoring of batches of models against the matches of their point sets. The host side of the search --
// checks, layout, router, the LORANSAC walk, local estimators, decisions -- is two_view_plan.h; this file uploads,
// launches and hands that walk its Backend. What a lane evaluates is two_view_solvers.h.
//
// A handle holds a batch of point sets: x1, y1, x2, y2 in double, SoA, every set's segment padded to whole waves.
//
// Kernels:
//   tvg_hypothesize_kernel<KIND>  one lane per trial, 64 lanes per workgroup. The lane finds its item by bisection of the
//                                 items' trial prefix, draws its sample from (seed, stream id of the set, kind, trial),
//                                 gathers the 7 / 4 / 1 matches and solves. The 7 x 9 / 8 x 9 working matrix is indexed by
//                                 run-time pivots: it lives in LDS, lane-minor (element k of lane l at work[64 k + l], so
//                                 a wave's accesses to one element fall in distinct banks), never in a private array,
//                                 which would go to scratch. Writes num_models[trial], models[trial][3][9] and the set of
//                                 every model slot (-1 for a slot without a model), which is what the scorer reads.
//   tvg_score_kernel<KIND>        a workgroup of 64 lanes owns one set x a tile of 64 model slots, one model per lane: 9
//                                 coefficients, a count and a sum in registers. The set's matches are staged through
//                                 LDS in tiles of 256 and read as broadcasts. Summation order of residual_sum: ONE
//                                 accumulator per model adds the inlier residuals in match order. It depends on the
//                                 set alone: not on the number of models in the launch, not on the model's position.
// No atomics of any kind. The scorer of a search round is the same kernel, reading the models the first kernel left in
// device memory: one host synchronisation per round.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_tvg.h"
#include "two_view_plan.h"
#include "two_view_solvers.h"

#define TVG_API __attribute__((visibility("default")))

namespace {

namespace tp = two_view_plan;

thread_local std::string g_error;
thread_local double g_kernel_ms = 0.0, g_total_ms = 0.0;

using Fail = tp::Fail;
#define TVG_HIP(call)                                                                    \
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

constexpr int kLanes = 64;        // lanes of a workgroup of either kernel: one wave
constexpr int kModelTile = 64;    // model slots of one workgroup of the scorer, one per lane
constexpr int kMatchTile = 256;   // matches of one LDS tile of the scorer
constexpr int kMatchesPerLane = kMatchTile / kLanes;
constexpr int kSlots = tvs::kMaxModels;

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

struct LdsWork {  // element k of this lane's working storage
  double* p;
  __device__ double& operator()(int k) const { return p[kLanes * k]; }
};

template <int KIND>
__global__ __launch_bounds__(kLanes) void tvg_hypothesize_kernel(
    const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2, const double* __restrict__ y2,
    const int* __restrict__ set_begin, const int* __restrict__ set_count, const unsigned long long* __restrict__ set_stream,
    const int* __restrict__ item_set, const long long* __restrict__ item_first_trial, const long long* __restrict__ item_trial_begin,
    int num_items, long long num_trials, int random_seed, int* __restrict__ num_models, double* __restrict__ models,
    int* __restrict__ slot_set, unsigned* __restrict__ samples) {
  __shared__ double work[tvs::kWorkDoubles * kLanes];
  const long long g = (long long)blockIdx.x * kLanes + threadIdx.x;
  if (g >= num_trials) return;
  int lo = 0, hi = num_items - 1;  // the item with item_trial_begin[item] <= g < item_trial_begin[item + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (item_trial_begin[mid] <= g)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int set = item_set[lo];
  const unsigned long long trial = (unsigned long long)(item_first_trial[lo] + (g - item_trial_begin[lo]));
  const int begin = set_begin[set], n = set_count[set];
  constexpr int K = KIND == tvs::KIND_F ? 7 : KIND == tvs::KIND_H ? 4 : 1;
  uint32_t idx[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  tvs::draw_sample(random_seed, set_stream[set], KIND, trial, (uint32_t)n, idx);  // n >= K: checked by the host
  double a1[K], b1[K], a2[K], b2[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int row = begin + (int)idx[k];
    a1[k] = x1[row];
    b1[k] = y1[row];
    a2[k] = x2[row];
    b2[k] = y2[row];
  }
  // the models go straight to device memory: the cubic's root count is a run-time index, and a private [3][9] array
  // under it would live in scratch
  double (*out)[9] = reinterpret_cast<double (*)[9]>(models + 9 * (kSlots * g));
  int nm;
  LdsWork W{work + threadIdx.x};
  if constexpr (KIND == tvs::KIND_F) {
    nm = tvs::solve_f7(W, a1, b1, a2, b2, out);
  } else if constexpr (KIND == tvs::KIND_H) {
    nm = tvs::solve_h4(W, a1, b1, a2, b2, out[0]);
  } else {
    tvs::solve_t1(a1[0], b1[0], a2[0], b2[0], out[0]);
    nm = 1;
  }
  num_models[g] = nm;
  for (int m = 0; m < kSlots; ++m) {
    slot_set[kSlots * g + m] = m < nm ? set : -1;
    if (m >= nm)
      for (int k = 0; k < 9; ++k) out[m][k] = 0.0;
  }
  if (samples) {
#pragma unroll
    for (int k = 0; k < 7; ++k) samples[7 * g + k] = k < K ? idx[k] : 0u;
  }
}

// tile t: the model slots [tile_first[t], tile_first[t] + tile_count[t]) against set tile_set[t]
template <int KIND>
__global__ __launch_bounds__(kLanes) void tvg_score_kernel(
    const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2, const double* __restrict__ y2,
    const int* __restrict__ set_begin, const int* __restrict__ set_count, const int* __restrict__ tile_set,
    const long long* __restrict__ tile_first, const int* __restrict__ tile_count, const int* __restrict__ slot_set,
    const double* __restrict__ models, double max_residual, long long* __restrict__ num_inliers,
    double* __restrict__ residual_sum, const long long* __restrict__ mask_offset, unsigned char* __restrict__ mask) {
  __shared__ double s1x[kMatchTile], s1y[kMatchTile], s2x[kMatchTile], s2y[kMatchTile];
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int set = tile_set[tile];
  const int begin = set_begin[set], n = set_count[set];
  const long long slot = tile_first[tile] + lane;
  const bool valid = lane < tile_count[tile] && slot_set[slot] >= 0;
  double M[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = valid ? models[9 * slot + k] : 0.0;
  unsigned char* const my_mask = (mask && valid) ? mask + mask_offset[slot] : nullptr;
  long long count = 0;
  double sum = 0.0;
  for (int base = 0; base < n; base += kMatchTile) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < kMatchesPerLane; ++j) {
      const int i = kLanes * j + lane;
      const bool in = base + i < n;
      s1x[i] = in ? x1[begin + base + i] : 0.0;
      s1y[i] = in ? y1[begin + base + i] : 0.0;
      s2x[i] = in ? x2[begin + base + i] : 0.0;
      s2y[i] = in ? y2[begin + base + i] : 0.0;
    }
    __syncthreads();
    if (valid) {
      const int m = n - base < kMatchTile ? n - base : kMatchTile;
      for (int i = 0; i < m; ++i) {
        const double r = tvs::residual(KIND, M, s1x[i], s1y[i], s2x[i], s2y[i]);
        const bool inlier = r <= max_residual;
        if (inlier) {
          ++count;
          sum += r;
        }
        if (my_mask) my_mask[base + i] = inlier ? 1 : 0;
      }
    }
  }
  if (lane < tile_count[tile]) {
    num_inliers[slot] = count;
    residual_sum[slot] = sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

void bind_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Fail("no HIP device available: two-view geometry estimation runs on the GPU (there is no CPU path)");
  if (!(gpu_index >= 0 && gpu_index < ndev)) throw Fail("gpu_index " + std::to_string(gpu_index) + " out of range");
  TVG_HIP(hipSetDevice(gpu_index));
}

template <typename T>
struct DeviceBuffer {
  T* p = nullptr;
  size_t n = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  void alloc(size_t count) {
    release();
    if (count == 0) return;
    TVG_HIP(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
  }
  void reserve(size_t count) {  // scratch: contents are not kept
    if (count > n) alloc(count + count / 2);
  }
  void put(const T* host, size_t count) {
    reserve(count);
    if (count) TVG_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
  }
  void get(T* host, size_t count) const {
    if (count && host) TVG_HIP(hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DeviceBuffer() { release(); }
};

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  Timer() {
    TVG_HIP(hipEventCreate(&a));
    TVG_HIP(hipEventCreate(&b));
  }
  Timer(const Timer&) = delete;
  Timer& operator=(const Timer&) = delete;
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void start() { TVG_HIP(hipEventRecord(a, 0)); }
  double stop() {
    TVG_HIP(hipEventRecord(b, 0));
    TVG_HIP(hipEventSynchronize(b));
    float ms = 0.0f;
    TVG_HIP(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
};

struct Tiles {  // the scorer's work list
  std::vector<int> set, count;
  std::vector<long long> first;
  void add(int s, long long first_slot, long long num_slots) {
    for (long long o = 0; o < num_slots; o += kModelTile) {
      set.push_back(s);
      first.push_back(first_slot + o);
      count.push_back((int)std::min<long long>(kModelTile, num_slots - o));
    }
  }
};

}  // namespace

struct tvg_handle : tp::Backend {
  int gpu_index = 0;
  std::unique_ptr<Timer> timer;
  double kernel_ms = 0.0;  // of the running call
  // the batch
  tp::SetLayout layout;
  std::vector<int64_t> offsets{0};
  std::vector<double> points;  // host copy [.][4]: the local estimators' input
  int num_sets = 0;
  DeviceBuffer<double> d_xy;  // x1 | y1 | x2 | y2, num_rows each
  DeviceBuffer<int> d_set_begin, d_set_count;
  DeviceBuffer<unsigned long long> d_set_stream;
  // a launch
  DeviceBuffer<int> d_item_set, d_num_models, d_slot_set, d_tile_set, d_tile_count;
  DeviceBuffer<long long> d_item_first, d_item_begin, d_tile_first, d_num_inliers, d_mask_offset;
  DeviceBuffer<double> d_models, d_residual_sum;
  DeviceBuffer<unsigned> d_samples;
  DeviceBuffer<unsigned char> d_mask;

  const double* dx(int c) const { return d_xy.p + (size_t)c * (size_t)layout.num_rows; }

  void upload(const std::vector<int64_t>& offs, const std::vector<double>& pts, const std::vector<uint64_t>& streams) override {
    TVG_HIP(hipSetDevice(gpu_index));
    const int32_t S = (int32_t)offs.size() - 1;
    layout = tp::make_layout(S, offs.data());
    offsets = offs;
    points = pts;
    num_sets = S;
    const size_t rows = (size_t)layout.num_rows;
    std::vector<double> soa(4 * rows, 0.0);
    for (int32_t s = 0; s < S; ++s)
      for (int64_t i = 0; i < layout.count[(size_t)s]; ++i)
        for (int c = 0; c < 4; ++c)
          soa[(size_t)c * rows + (size_t)layout.begin[(size_t)s] + (size_t)i] = pts[4 * (size_t)(offs[(size_t)s] + i) + (size_t)c];
    d_xy.put(soa.data(), soa.size());
    d_set_begin.put(layout.begin.data(), (size_t)S);
    d_set_count.put(layout.count.data(), (size_t)S);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "stream ids are uploaded as they are");
    d_set_stream.put((const unsigned long long*)streams.data(), (size_t)S);
  }

  // launches the solver for the items' trials; returns the number of trials. The models stay on the device.
  size_t hypothesize(int kind, int32_t seed, const std::vector<tp::Item>& items, bool want_samples) {
    std::vector<int> set(items.size());
    std::vector<long long> first(items.size()), begin(items.size() + 1, 0);
    for (size_t i = 0; i < items.size(); ++i) {
      const tp::Item& it = items[i];
      TVG_CHECK(it.set >= 0 && it.set < num_sets, "item " + std::to_string(i) + ": set out of range");
      TVG_CHECK(it.first_trial >= 0 && it.num_trials >= 0, "item " + std::to_string(i) + ": negative trial");
      TVG_CHECK(it.num_trials == 0 || layout.count[(size_t)it.set] >= tvs::min_samples(kind),
                "item " + std::to_string(i) + ": its set holds fewer matches than a minimal sample");
      set[i] = it.set;
      first[i] = it.first_trial;
      begin[i + 1] = begin[i] + it.num_trials;
    }
    const size_t total = (size_t)begin[items.size()];
    TVG_CHECK(total * kSlots * 9 < ((size_t)1 << 31), "the trials of one launch must stay below 2^31 / 27");
    if (total == 0) return 0;
    d_item_set.put(set.data(), set.size());
    d_item_first.put(first.data(), first.size());
    d_item_begin.put(begin.data(), begin.size());
    d_num_models.reserve(total);
    d_models.reserve(total * kSlots * 9);
    d_slot_set.reserve(total * kSlots);
    if (want_samples) d_samples.reserve(total * 7);
    const dim3 grid((unsigned)((total + kLanes - 1) / kLanes));
#define TVG_LAUNCH_HYP(K)                                                                                                  \
  hipLaunchKernelGGL(tvg_hypothesize_kernel<K>, grid, dim3(kLanes), 0, 0, dx(0), dx(1), dx(2), dx(3), d_set_begin.p,        \
                     d_set_count.p, d_set_stream.p, d_item_set.p, d_item_first.p, d_item_begin.p, (int)items.size(),       \
                     (long long)total, (int)seed, d_num_models.p, d_models.p, d_slot_set.p, want_samples ? d_samples.p : nullptr)
    if (kind == tvs::KIND_F)
      TVG_LAUNCH_HYP(tvs::KIND_F);
    else if (kind == tvs::KIND_H)
      TVG_LAUNCH_HYP(tvs::KIND_H);
    else
      TVG_LAUNCH_HYP(tvs::KIND_T);
#undef TVG_LAUNCH_HYP
    TVG_HIP(hipGetLastError());
    return total;
  }

  // launches the scorer over the tiles for the slots d_slot_set / d_models hold
  void launch_score(int kind, double max_error, const Tiles& tiles, size_t num_slots, bool want_mask) {
    if (tiles.set.empty()) return;
    d_tile_set.put(tiles.set.data(), tiles.set.size());
    d_tile_first.put(tiles.first.data(), tiles.first.size());
    d_tile_count.put(tiles.count.data(), tiles.count.size());
    d_num_inliers.reserve(num_slots);
    d_residual_sum.reserve(num_slots);
    const dim3 grid((unsigned)tiles.set.size());
    const double max_residual = max_error * max_error;
#define TVG_LAUNCH_SCORE(K)                                                                                                \
  hipLaunchKernelGGL(tvg_score_kernel<K>, grid, dim3(kLanes), 0, 0, dx(0), dx(1), dx(2), dx(3), d_set_begin.p, d_set_count.p, \
                     d_tile_set.p, d_tile_first.p, d_tile_count.p, d_slot_set.p, d_models.p, max_residual, d_num_inliers.p, \
                     d_residual_sum.p, want_mask ? d_mask_offset.p : nullptr, want_mask ? d_mask.p : nullptr)
    if (kind == tvs::KIND_F)
      TVG_LAUNCH_SCORE(tvs::KIND_F);
    else if (kind == tvs::KIND_H)
      TVG_LAUNCH_SCORE(tvs::KIND_H);
    else
      TVG_LAUNCH_SCORE(tvs::KIND_T);
#undef TVG_LAUNCH_SCORE
    TVG_HIP(hipGetLastError());
  }

  void round(int kind, double max_error, int32_t seed, const std::vector<tp::Item>& items, tp::RoundResult* out) override {
    TVG_HIP(hipSetDevice(gpu_index));
    timer->start();
    const size_t total = hypothesize(kind, seed, items, false);
    Tiles tiles;
    long long slot = 0;
    for (const tp::Item& it : items) {
      tiles.add(it.set, slot, (long long)kSlots * it.num_trials);
      slot += (long long)kSlots * it.num_trials;
    }
    launch_score(kind, max_error, tiles, total * kSlots, false);
    kernel_ms += timer->stop();
    out->num_models.resize(total);
    out->models.resize(total * kSlots * 9);
    out->supports.resize(total * kSlots);
    d_num_models.get(out->num_models.data(), total);
    d_models.get(out->models.data(), total * kSlots * 9);
    std::vector<long long> n(total * kSlots);
    std::vector<double> sum(total * kSlots);
    d_num_inliers.get(n.data(), n.size());
    d_residual_sum.get(sum.data(), sum.size());
    for (size_t k = 0; k < n.size(); ++k) {
      out->supports[k].num_inliers = (uint64_t)n[k];
      out->supports[k].residual_sum = sum[k];
    }
  }

  // models: [num][9]; masks (nullable): one after the other, each as long as its set
  void score_arrays(int kind, double max_error, size_t num, const int32_t* model_set, const double* models, int64_t* num_inliers,
                    double* residual_sum, uint8_t* masks) {
    if (num == 0) return;
    TVG_HIP(hipSetDevice(gpu_index));
    std::vector<long long> mask_offset(num + 1, 0);
    Tiles tiles;
    size_t run = 0;
    for (size_t m = 0; m < num; ++m) {
      TVG_CHECK(model_set[m] >= 0 && model_set[m] < num_sets, "model " + std::to_string(m) + ": set out of range");
      mask_offset[m + 1] = mask_offset[m] + layout.count[(size_t)model_set[m]];
      if (m + 1 == num || model_set[m + 1] != model_set[m]) {  // a run of models of one set shares its tiles
        tiles.add(model_set[m], (long long)run, (long long)(m + 1 - run));
        run = m + 1;
      }
    }
    static_assert(sizeof(int) == sizeof(int32_t), "sets are uploaded as they are");
    d_slot_set.put((const int*)model_set, num);
    d_models.put(models, 9 * num);
    if (masks) {
      d_mask_offset.put(mask_offset.data(), num);
      d_mask.reserve((size_t)mask_offset[num]);
    }
    timer->start();
    launch_score(kind, max_error, tiles, num, masks != nullptr);
    kernel_ms += timer->stop();
    static_assert(sizeof(long long) == sizeof(int64_t), "counts are downloaded as they are");
    d_num_inliers.get((long long*)num_inliers, num);
    d_residual_sum.get(residual_sum, num);
    if (masks) d_mask.get(masks, (size_t)mask_offset[num]);
  }

  void score(int kind, double max_error, const std::vector<tp::ScoreJob>& jobs, std::vector<tp::Support>* supports,
             std::vector<std::vector<uint8_t>>* masks) override {
    const size_t J = jobs.size();
    std::vector<int32_t> set(J);
    std::vector<double> models(9 * J);
    size_t bytes = 0;
    for (size_t k = 0; k < J; ++k) {
      set[k] = jobs[k].set;
      for (int c = 0; c < 9; ++c) models[9 * k + (size_t)c] = jobs[k].model[(size_t)c];
      bytes += (size_t)layout.count[(size_t)jobs[k].set];
    }
    std::vector<int64_t> n(J);
    std::vector<double> sum(J);
    std::vector<uint8_t> flat(masks ? bytes : 0);
    score_arrays(kind, max_error, J, set.data(), models.data(), n.data(), sum.data(), masks ? flat.data() : nullptr);
    supports->resize(J);
    if (masks) masks->resize(J);
    size_t at = 0;
    for (size_t k = 0; k < J; ++k) {
      (*supports)[k].num_inliers = (uint64_t)n[k];
      (*supports)[k].residual_sum = sum[k];
      if (masks) {
        const size_t len = (size_t)layout.count[(size_t)jobs[k].set];
        (*masks)[k].assign(flat.begin() + (long)at, flat.begin() + (long)(at + len));
        at += len;
      }
    }
  }
};

namespace {

struct CallClock {  // kernel and total time of one ABI call
  tvg_handle* H;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit CallClock(tvg_handle* h) : H(h) { H->kernel_ms = 0.0; }
  void done() {
    g_kernel_ms = H->kernel_ms;
    g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
};

void check_models(const double* models, size_t num) {
  TVG_CHECK(num == 0 || models, "the models are null (9 doubles each)");
}

}  // namespace

extern "C" {

TVG_API void tvg_ransac_options_init(tvg_ransac_options* o) {
  o->max_error = 4.0;
  o->min_inlier_ratio = 0.25;
  o->confidence = 0.999;
  o->dyn_num_trials_multiplier = 3.0;
  o->min_num_trials = 100;
  o->max_num_trials = 10000;
  o->random_seed = -1;
  o->trials_per_round = 0;
}

TVG_API void tvg_options_init(tvg_options* o) {
  tvg_ransac_options_init(&o->ransac);
  o->min_num_inliers = 15;
  o->detect_watermark = 1;
  o->multiple_ignore_watermark = 1;
  o->filter_stationary_matches = 0;
  o->force_H_use = 0;
  o->multiple_models = 0;
  o->max_H_inlier_ratio = 0.8;
  o->watermark_min_inlier_ratio = 0.7;
  o->watermark_border_size = 0.1;
  o->watermark_detection_max_error = 4.0;
  o->stationary_matches_max_error = 4.0;
}

TVG_API int tvg_create(int32_t gpu_index, tvg_handle** handle) {
  return Guard([&] {
    if (!handle) throw Fail("null argument");
    *handle = nullptr;
    bind_device(gpu_index);
    std::unique_ptr<tvg_handle> H(new tvg_handle);
    H->gpu_index = gpu_index;
    H->timer.reset(new Timer);
    *handle = H.release();
  });
}

TVG_API void tvg_destroy(tvg_handle* handle) { delete handle; }

TVG_API int tvg_set_points(tvg_handle* handle, int32_t num_sets, const int64_t* set_offsets, const double* points,
                           const uint64_t* stream_ids) {
  return Guard([&] {
    if (!handle) throw Fail("null handle");
    tp::validate_offsets(num_sets, set_offsets, points, "sets");
    TVG_CHECK(num_sets == 0 || stream_ids, "the stream ids are null");
    CallClock clock(handle);
    const size_t total = (size_t)set_offsets[num_sets];
    handle->upload(std::vector<int64_t>(set_offsets, set_offsets + num_sets + 1), std::vector<double>(points, points + 4 * total),
                   std::vector<uint64_t>(stream_ids, stream_ids + num_sets));
    clock.done();
  });
}

TVG_API int tvg_hypothesize(tvg_handle* handle, int32_t kind, int32_t random_seed, int32_t num_items, const int32_t* item_set,
                            const int64_t* item_first_trial, const int32_t* item_num_trials, int32_t* num_models, double* models,
                            uint32_t* samples) {
  return Guard([&] {
    if (!handle) throw Fail("null handle");
    tp::check_kind(kind);
    TVG_CHECK(num_items >= 0, "num_items must not be negative");
    TVG_CHECK(random_seed >= -1, "random_seed must be -1 or larger");
    TVG_CHECK(num_items == 0 || (item_set && item_first_trial && item_num_trials), "the items are null");
    CallClock clock(handle);
    std::vector<tp::Item> items((size_t)num_items);
    for (int32_t i = 0; i < num_items; ++i) items[(size_t)i] = {item_set[i], item_first_trial[i], item_num_trials[i]};
    TVG_HIP(hipSetDevice(handle->gpu_index));
    handle->timer->start();
    const size_t total = handle->hypothesize(kind, random_seed, items, samples != nullptr);
    handle->kernel_ms += handle->timer->stop();
    TVG_CHECK(total == 0 || (num_models && models), "num_models and models are null");
    static_assert(sizeof(int) == sizeof(int32_t) && sizeof(unsigned) == sizeof(uint32_t), "downloaded as they are");
    handle->d_num_models.get((int*)num_models, total);
    handle->d_models.get(models, total * kSlots * 9);
    if (samples) handle->d_samples.get((unsigned*)samples, total * 7);
    clock.done();
  });
}

TVG_API int tvg_score(tvg_handle* handle, int32_t kind, double max_error, int32_t num_models, const int32_t* model_set,
                      const double* models, int64_t* num_inliers, double* residual_sum, uint8_t* inlier_masks) {
  return Guard([&] {
    if (!handle) throw Fail("null handle");
    tp::check_kind(kind);
    TVG_CHECK(num_models >= 0, "num_models must not be negative");
    TVG_CHECK(max_error >= 0.0, "max_error must not be negative");
    check_models(models, (size_t)num_models);
    TVG_CHECK(num_models == 0 || (model_set && num_inliers && residual_sum), "model_set, num_inliers or residual_sum is null");
    CallClock clock(handle);
    handle->score_arrays(kind, max_error, (size_t)num_models, model_set, models, num_inliers, residual_sum, inlier_masks);
    clock.done();
  });
}

TVG_API int tvg_estimate(tvg_handle* handle, int32_t kind, const tvg_ransac_options* options, const double* min_inlier_ratios,
                         tvg_report* reports) {
  return Guard([&] {
    if (!handle || !options) throw Fail("null argument");
    TVG_CHECK(handle->num_sets == 0 || reports, "the reports are null");
    CallClock clock(handle);
    const std::vector<tp::Report> R =
        tp::estimate(*handle, kind, *options, handle->offsets, handle->points, min_inlier_ratios, nullptr);
    for (size_t s = 0; s < R.size(); ++s) {
      tvg_report& o = reports[s];
      o.success = R[s].success ? 1 : 0;
      o.has_model = R[s].has_model ? 1 : 0;
      o.num_trials = (int64_t)R[s].num_trials;
      o.num_inliers = (int64_t)R[s].support.num_inliers;
      o.residual_sum = R[s].support.residual_sum;
      for (int k = 0; k < 9; ++k) o.model[k] = R[s].model[(size_t)k];
      if (o.inlier_mask) {
        const size_t n = (size_t)(handle->offsets[s + 1] - handle->offsets[s]);
        if (R[s].inlier_mask.size() == n && n)
          std::memcpy(o.inlier_mask, R[s].inlier_mask.data(), n);
        else if (n)
          std::memset(o.inlier_mask, 0, n);
      }
      o.num_scored = (int64_t)R[s].num_scored;
      o.num_launches = (int64_t)R[s].num_launches;
    }
    clock.done();
  });
}

TVG_API int tvg_verify_pairs(tvg_handle* handle, const tvg_options* options, int32_t num_pairs, const tvg_camera* cameras1,
                             const tvg_camera* cameras2, const int64_t* match_offsets, const double* points,
                             const uint64_t* stream_ids, int32_t* route, int32_t* config, int32_t* has_F, double* F,
                             int32_t* has_H, double* H, uint8_t* inlier_mask, int64_t* stats) {
  return Guard([&] {
    if (!handle || !options) throw Fail("null argument");
    TVG_CHECK(num_pairs >= 0, "num_pairs must not be negative");
    TVG_CHECK(num_pairs == 0 || (route && config && has_F && F && has_H && H), "an output array is null");
    CallClock clock(handle);
    tp::VerifyStats vs;
    const std::vector<tp::PairResult> R =
        tp::verify_pairs(*handle, *options, num_pairs, cameras1, cameras2, match_offsets, points, stream_ids, &vs);
    TVG_CHECK(num_pairs == 0 || match_offsets[num_pairs] == 0 || inlier_mask, "inlier_mask is null");
    for (size_t p = 0; p < R.size(); ++p) {
      const tp::Geometry& g = R[p].geometry;
      route[p] = R[p].route;
      config[p] = g.config;
      has_F[p] = g.has_F ? 1 : 0;
      has_H[p] = g.has_H ? 1 : 0;
      for (int k = 0; k < 9; ++k) {
        F[9 * p + (size_t)k] = g.has_F ? g.F[(size_t)k] : 0.0;
        H[9 * p + (size_t)k] = g.has_H ? g.H[(size_t)k] : 0.0;
      }
      if (!g.inlier_mask.empty()) std::memcpy(inlier_mask + match_offsets[p], g.inlier_mask.data(), g.inlier_mask.size());
    }
    if (stats) {
      stats[0] = (int64_t)vs.num_scored;
      stats[1] = (int64_t)vs.num_launches;
    }
    clock.done();
  });
}

TVG_API int tvg_route(const tvg_camera* camera1, const tvg_camera* camera2, const tvg_options* options) {
  if (!camera1 || !camera2 || !options) return -1;
  return tp::route(*camera1, *camera2, *options);
}

TVG_API const char* tvg_route_name(int32_t route) { return tp::route_name(route); }

TVG_API int tvg_route_is_built(int32_t route) { return tp::route_is_built(route) ? 1 : 0; }

TVG_API int tvg_draw_sample(int32_t random_seed, uint64_t stream_id, int32_t kind, uint64_t trial, uint32_t num_points,
                            uint32_t sample[7]) {
  return Guard([&] {
    tp::check_kind(kind);
    TVG_CHECK(sample != nullptr, "sample is null");
    TVG_CHECK(num_points >= (uint32_t)tvs::min_samples(kind), "fewer points than a minimal sample");
    for (int k = 0; k < 7; ++k) sample[k] = 0u;
    tvs::draw_sample(random_seed, stream_id, kind, trial, num_points, sample);
  });
}

TVG_API int tvg_model_tile(void) { return kModelTile; }
TVG_API int tvg_match_tile(void) { return kMatchTile; }
TVG_API int tvg_trial_round(void) { return tp::kDefaultTrialRound; }

TVG_API void tvg_last_timing(double* kernel_ms, double* total_ms) {
  if (kernel_ms) *kernel_ms = g_kernel_ms;
  if (total_ms) *total_ms = g_total_ms;
}

TVG_API const char* tvg_last_error(void) { return g_error.c_str(); }

}  // extern "C"
