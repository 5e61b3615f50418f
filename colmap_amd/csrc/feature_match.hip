// feature_match.hip -- SIFT descriptor matching on gfx950 (include/colmap_amd_match.h): one launch computes, for a list
// of image pairs and both directions of each, the first best column, the best and the second best dot product of every
// descriptor against the other image's set (reference feature/sift.cc:772-864, 967-1004, 1346-1473). The host plan, the
// device image of a set and the finish are in match_plan.h; DESIGN.md section 2.4e has the numbers.
//
// Work split. A workgroup (4 waves) owns 256 query rows of one direction of one pair (a row of the host's tile table);
// each wave keeps ITS 64 rows as 4 x 2 operand fragments of v_mfma_i32_16x16x64_i8 in registers for the whole kernel
// (K = 128 is two k-steps). The other set streams past in chunks of 64 rows that the workgroup stages in LDS once, in
// fragment order, and every wave reads. The matrix instruction takes the streamed rows as A and the query rows as B, so
// that by the C/D map (col = lane & 15, row = 4 (lane >> 4) + reg) a LANE owns one query per tile and its 4 registers
// are 4 streamed rows: the running top-2 of a query is plain per-lane arithmetic; the 4 lanes that share a query merge
// once at the end. The column direction is the same kernel with the sets swapped: no cross-workgroup merge, no
// atomics, one possible value per output.
//
// Unsigned inputs. The instruction is signed; a set is stored as x - 128 with corr[row] = 128 * sum(row) - 2 097 152
// (match_plan.h: build_device_image). corr of the streamed rows is the C input, so a register after the two k-steps
// holds v = dot - 128 * sum(query), exact in int32 over the full 0..255; 128 * sum(query) is constant per lane and
// does not change the order, it is added back when the result is written. Padding rows of the streamed set are zero
// descriptors whose corr is match_plan::kAbsent, below every real v: such a column is absent, it can neither win nor
// raise `second`, and a row that saw only absent columns reports (-1, 0, 0).
//
// Operand map. Both operands are loaded the same way: lane l takes, for k-step s, bytes 64 s + 16 (l >> 4) .. + 15 of
// row (l & 15) of its 16-row fragment. Whatever k each of a lane's 16 bytes stands for inside the instruction, the A and
// the B fragment of one lane group pair the SAME 16 bytes of their rows element by element, and the four lane groups
// cover the 64 bytes of the step, so the result cannot depend on the k order inside a fragment.
//
// Selection. v (24 bits and a sign) is packed with 255 - (column inside a window of 256 streamed rows) into one int32
// key: a larger dot wins, on equal dots the smaller column. Then best' = max(best, key) and
// second' = max(second, min(best, key)) keep the two largest keys; equal dots at different columns are different keys,
// so `second == best` comes out for a doubled maximum. Every 4 chunks the window's two keys are unpacked and merged
// into the lane's running (best, idx, second) by the order-free rule of match_plan.h.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_match.h"
#include "match_plan.h"

#define MATCH_API __attribute__((visibility("default")))

namespace {

namespace mp = match_plan;

thread_local std::string g_error;
thread_local double g_kernel_ms = 0.0, g_total_ms = 0.0;

using Fail = mp::Fail;
#define MATCH_HIP(call)                                                                  \
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
constexpr int kQueryTiles = mp::kWaveRows / 16;  // MFMA tiles of a wave's query rows
constexpr int kChunkSteps = mp::kChunkRows / 16;  // 16-row fragments of a streamed chunk
constexpr int kWindowChunks = 4;                  // 256 streamed rows share the 8 index bits of a key
static_assert(kBlock / 64 * mp::kWaveRows == mp::kTileRows, "a workgroup's waves cover one tile of the plan");
static_assert(kWindowChunks * mp::kChunkRows == 256, "the key has 8 bits of column");
static_assert(mp::kChunkRows * mp::kDim / 16 == 2 * kBlock, "every thread stages two 16-byte pieces of a chunk");

typedef int v4i __attribute__((ext_vector_type(4)));

struct DevSet {
  const v4i* desc;     // [rows_pad][8] pieces of 16 bytes: the rows as int8 (x - 128)
  const int* corr;     // [rows_pad]
  int rows, rows_pad;  // rows_pad: multiple of match_plan::kChunkRows
};

__global__ __launch_bounds__(kBlock) void match_top2_kernel(const DevSet* __restrict__ sets,
                                                            const mp::Tile* __restrict__ tiles, int* __restrict__ out) {
  // [16-row fragment][k-step][lane]: a wave reads one fragment as 1 KiB of consecutive 16-byte pieces
  __shared__ v4i s_frag[kChunkSteps][2][64];
  __shared__ int s_corr[mp::kChunkRows] __attribute__((aligned(16)));  // read 4 at a time

  const mp::Tile T = tiles[blockIdx.x];
  const DevSet Q = sets[T.query_set], S = sets[T.stream_set];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int q_base = T.query_row0 + wave * mp::kWaveRows;
  // wave-uniform. rows_pad is a multiple of the 64 rows of a wave, so an active wave's 64 rows are all allocated.
  const bool active = q_base < Q.rows;

  v4i qf[kQueryTiles][2];
  for (int t = 0; t < kQueryTiles; ++t)
    for (int s = 0; s < 2; ++s) {
      qf[t][s] = v4i{0, 0, 0, 0};
      if (active) qf[t][s] = Q.desc[(size_t)(q_base + 16 * t + c) * 8 + 4 * s + g];
    }

  int rb[kQueryTiles], ri[kQueryTiles], rs[kQueryTiles];  // running best, its column, second (biased values)
  int bk[kQueryTiles], sk[kQueryTiles];                   // the window's two largest keys
  for (int t = 0; t < kQueryTiles; ++t) {
    rb[t] = rs[t] = mp::kAbsent;
    ri[t] = -1;
    bk[t] = sk[t] = INT32_MIN;
  }

  // staging: piece p of a chunk is 16 bytes of row p >> 3; a thread moves pieces tid and tid + 256
  const int num_chunks = S.rows_pad / mp::kChunkRows;
  v4i stage[2];
  int stage_corr = 0;
  auto fetch = [&](int chunk) {
    const v4i* src = S.desc + (size_t)chunk * (mp::kChunkRows * 8);
    stage[0] = src[tid];
    stage[1] = src[tid + kBlock];
    if (tid < mp::kChunkRows) stage_corr = S.corr[chunk * mp::kChunkRows + tid];
  };
  if (num_chunks > 0) fetch(0);

  for (int chunk = 0; chunk < num_chunks; ++chunk) {
    __syncthreads();  // the previous chunk has been read by every wave
    for (int u = 0; u < 2; ++u) {
      const int p = tid + u * kBlock, row = p >> 3, piece = p & 7;
      s_frag[row >> 4][piece >> 2][(piece & 3) * 16 + (row & 15)] = stage[u];
    }
    if (tid < mp::kChunkRows) s_corr[tid] = stage_corr;
    __syncthreads();
    if (chunk + 1 < num_chunks) fetch(chunk + 1);  // in flight while this chunk is multiplied

    if (active) {
      const int window_pos = (chunk % kWindowChunks) * mp::kChunkRows;
      for (int step = 0; step < kChunkSteps; ++step) {
        const v4i a0 = s_frag[step][0][lane], a1 = s_frag[step][1][lane];
        const v4i cin = *reinterpret_cast<const v4i*>(&s_corr[step * 16 + 4 * g]);
        const int code = 255 - (window_pos + step * 16 + 4 * g);  // of register 0; register r is column + r
        for (int t = 0; t < kQueryTiles; ++t) {
          v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, qf[t][0], cin, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, qf[t][1], acc, 0, 0, 0);
          for (int r = 0; r < 4; ++r) {
            const int key = (int)(((unsigned)acc[r] << 8) | (unsigned)(code - r));
            sk[t] = max(sk[t], min(bk[t], key));
            bk[t] = max(bk[t], key);
          }
        }
      }
      if (chunk % kWindowChunks == kWindowChunks - 1 || chunk + 1 == num_chunks) {
        const int window_row0 = (chunk / kWindowChunks) * (kWindowChunks * mp::kChunkRows);
        for (int t = 0; t < kQueryTiles; ++t) {
          const int b2 = bk[t] >> 8, s2 = sk[t] >> 8;  // arithmetic shifts: an unused key gives kAbsent
          const int i2 = window_row0 + 255 - (bk[t] & 255);
          rs[t] = max(max(min(rb[t], b2), rs[t]), s2);
          if (b2 > rb[t]) {  // windows ascend: on equal values the earlier column stays
            rb[t] = b2;
            ri[t] = i2;
          }
          bk[t] = sk[t] = INT32_MIN;
        }
      }
    }
  }

  if (!active) return;
  // the 4 lanes of a query (lane groups g = 0..3) hold disjoint columns: merge, smaller column on equal best
  for (int t = 0; t < kQueryTiles; ++t)
    for (int m = 16; m <= 32; m <<= 1) {
      const int ob = __shfl_xor(rb[t], m), oi = __shfl_xor(ri[t], m), os = __shfl_xor(rs[t], m);
      rs[t] = max(max(min(rb[t], ob), rs[t]), os);
      if (ob > rb[t] || (ob == rb[t] && oi < ri[t])) {
        rb[t] = ob;
        ri[t] = oi;
      }
    }
  // every lane now holds its query's result for all 4 tiles; lane group g writes tile g
  for (int t = 0; t < kQueryTiles; ++t) {
    if (t != g) continue;
    const int row = q_base + 16 * t + c;
    if (row >= Q.rows) continue;
    const int back = Q.corr[row] + mp::kRowBias;  // 128 * sum(query row)
    int idx = -1, best = 0, second = 0;           // the reference's start values: only a dot > 0 counts
    if (rb[t] != mp::kAbsent && rb[t] + back > 0) {
      idx = ri[t];
      best = rb[t] + back;
      second = rs[t] != mp::kAbsent ? rs[t] + back : 0;
    }
    int* o = out + (size_t)(T.out_row0 + row) * 3;
    o[0] = idx;
    o[1] = best;
    o[2] = second;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

void bind_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Fail("no HIP device available: descriptor matching runs on the GPU (there is no CPU path)");
  if (!(gpu_index >= 0 && gpu_index < ndev)) throw Fail("gpu_index " + std::to_string(gpu_index) + " out of range");
  MATCH_HIP(hipSetDevice(gpu_index));
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
    MATCH_HIP(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
  }
  void reserve(size_t count) {  // scratch: contents are not kept
    if (count > n) alloc(count);
  }
  void upload(const T* host, size_t count) {
    reserve(count);
    if (count) MATCH_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
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
    MATCH_HIP(hipEventCreate(&a));
    MATCH_HIP(hipEventCreate(&b));
  }
  Timer(const Timer&) = delete;
  Timer& operator=(const Timer&) = delete;
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void start() { MATCH_HIP(hipEventRecord(a, 0)); }
  double stop() {
    MATCH_HIP(hipEventRecord(b, 0));
    MATCH_HIP(hipEventSynchronize(b));
    float ms = 0.0f;
    MATCH_HIP(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
};

struct CachedSet {
  DeviceBuffer<int8_t> desc;
  DeviceBuffer<int32_t> corr;
  int rows = 0;
  size_t bytes = 0;
  uint64_t last_use = 0;
};

struct PairResult {
  int64_t rows[2] = {0, 0};
  int64_t out_row0[2] = {0, 0};
  std::vector<uint32_t> matches;
};

}  // namespace

struct match_handle {
  int gpu_index = 0;
  int max_num_matches = 0;
  size_t cache_bytes = 0, resident_bytes = 0;
  int64_t evictions = 0;
  uint64_t clock = 0;
  std::map<uint32_t, std::unique_ptr<CachedSet>> sets;
  DeviceBuffer<DevSet> d_sets;
  DeviceBuffer<mp::Tile> d_tiles;
  DeviceBuffer<int32_t> d_out;
  std::vector<int32_t> out;  // [out_rows][3] of the last call
  std::vector<PairResult> results;
  std::unique_ptr<Timer> timer;
};

namespace {

void evict_to_budget(match_handle& H, uint32_t keep) {
  while (H.resident_bytes > H.cache_bytes) {
    auto victim = H.sets.end();
    for (auto it = H.sets.begin(); it != H.sets.end(); ++it)
      if (it->first != keep && (victim == H.sets.end() || it->second->last_use < victim->second->last_use)) victim = it;
    if (victim == H.sets.end()) break;
    H.resident_bytes -= victim->second->bytes;
    H.sets.erase(victim);
    ++H.evictions;
  }
}

void set_descriptors(match_handle& H, uint32_t image_id, int rows, int cols, const uint8_t* data) {
  bool truncated = false;
  const int used = mp::check_descriptors(rows, cols, data, H.max_num_matches, &truncated);
  if (truncated)
    std::fprintf(stderr, "W image %u has %d descriptors: only the first %d take part (max_num_matches)\n", image_id, rows,
                 used);
  bind_device(H.gpu_index);
  std::vector<int8_t> desc;
  std::vector<int32_t> corr;
  mp::build_device_image(data, used, &desc, &corr);
  auto fresh = std::make_unique<CachedSet>();
  fresh->desc.upload(desc.data(), desc.size());
  fresh->corr.upload(corr.data(), corr.size());
  fresh->rows = used;
  fresh->bytes = mp::device_bytes(used);
  fresh->last_use = ++H.clock;
  auto old = H.sets.find(image_id);
  if (old != H.sets.end()) {
    H.resident_bytes -= old->second->bytes;
    H.sets.erase(old);
  }
  H.resident_bytes += fresh->bytes;
  H.sets[image_id] = std::move(fresh);
  evict_to_budget(H, image_id);
}

void match_pairs_impl(match_handle& H, const match_pair* pairs, int n, const match_options* options) {
  const auto t0 = std::chrono::steady_clock::now();
  g_kernel_ms = 0.0;
  mp::check_options(options);
  MATCH_CHECK(n >= 0, "number of pairs must not be negative");
  MATCH_CHECK(n == 0 || pairs != nullptr, "pairs is null");
  bind_device(H.gpu_index);
  H.results.clear();
  H.out.clear();

  // the launch's set table: the distinct images of the batch
  std::map<uint32_t, int32_t> slot_of;
  std::vector<DevSet> dev_sets;
  std::vector<int32_t> set_rows;
  std::vector<mp::PairSlots> slots(n);
  auto slot = [&](uint32_t image_id) {
    auto known = slot_of.find(image_id);
    if (known != slot_of.end()) return known->second;
    auto it = H.sets.find(image_id);
    if (it == H.sets.end())
      throw Fail("image " + std::to_string(image_id) + " has no descriptors on the device: match_set_descriptors first");
    CachedSet& s = *it->second;
    s.last_use = ++H.clock;
    dev_sets.push_back(DevSet{reinterpret_cast<const v4i*>(s.desc.p), s.corr.p, s.rows, mp::padded_rows(s.rows)});
    set_rows.push_back(s.rows);
    return slot_of[image_id] = (int32_t)dev_sets.size() - 1;
  };
  for (int p = 0; p < n; ++p) slots[p] = mp::PairSlots{slot(pairs[p].image_id1), slot(pairs[p].image_id2)};

  const mp::Launch L = mp::build_launch(set_rows, slots.data(), n);
  H.out.assign((size_t)L.out_rows * 3, 0);
  if (!L.tiles.empty()) {
    H.d_sets.upload(dev_sets.data(), dev_sets.size());
    H.d_tiles.upload(L.tiles.data(), L.tiles.size());
    H.d_out.reserve(H.out.size());
    if (!H.timer) H.timer = std::make_unique<Timer>();
    H.timer->start();
    hipLaunchKernelGGL(match_top2_kernel, dim3((unsigned)L.tiles.size()), dim3(kBlock), 0, 0, H.d_sets.p, H.d_tiles.p,
                       H.d_out.p);
    MATCH_HIP(hipGetLastError());
    g_kernel_ms = H.timer->stop();
    MATCH_HIP(hipMemcpy(H.out.data(), H.d_out.p, H.out.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }

  H.results.resize(n);
  for (int p = 0; p < n; ++p) {
    PairResult& R = H.results[p];
    for (int d = 0; d < 2; ++d) {
      R.rows[d] = set_rows[d == 0 ? slots[p].set1 : slots[p].set2];
      R.out_row0[d] = L.out_row0[2 * (size_t)p + d];
    }
    mp::finish(H.out.data() + 3 * R.out_row0[0], R.rows[0], H.out.data() + 3 * R.out_row0[1], R.rows[1], *options,
               &R.matches);
  }
  g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

PairResult& result_of(match_handle* handle, int k) {
  MATCH_CHECK(handle != nullptr, "handle is null");
  MATCH_CHECK(k >= 0 && k < (int)handle->results.size(), "pair index " + std::to_string(k) + " out of range");
  return handle->results[k];
}

}  // namespace

extern "C" {

MATCH_API void match_options_init(match_options* options) {
  if (options) mp::options_init(options);
}

MATCH_API int match_create(int32_t gpu_index, int32_t max_num_matches, size_t cache_bytes, match_handle** handle) {
  return Guard([&] {
    MATCH_CHECK(handle != nullptr, "handle is null");
    *handle = nullptr;
    const int limit = mp::effective_max_num_matches(max_num_matches);
    bind_device(gpu_index);
    auto H = std::make_unique<match_handle>();
    H->gpu_index = gpu_index;
    H->max_num_matches = limit;
    H->cache_bytes = mp::effective_cache_bytes(cache_bytes, limit);
    *handle = H.release();
  });
}

MATCH_API int match_set_descriptors(match_handle* handle, uint32_t image_id, int32_t rows, int32_t cols,
                                    const uint8_t* data) {
  return Guard([&] {
    MATCH_CHECK(handle != nullptr, "handle is null");
    set_descriptors(*handle, image_id, rows, cols, data);
  });
}

MATCH_API int match_has_descriptors(match_handle* handle, uint32_t image_id) {
  if (!handle) return 0;
  auto it = handle->sets.find(image_id);
  if (it == handle->sets.end()) return 0;
  it->second->last_use = ++handle->clock;
  return 1;
}

MATCH_API int match_pairs(match_handle* handle, const match_pair* pairs, int32_t n, const match_options* options) {
  return Guard([&] {
    MATCH_CHECK(handle != nullptr, "handle is null");
    match_pairs_impl(*handle, pairs, n, options);
  });
}

MATCH_API int match_num_matches(match_handle* handle, int32_t k, int64_t* count) {
  return Guard([&] {
    MATCH_CHECK(count != nullptr, "count is null");
    *count = (int64_t)result_of(handle, k).matches.size() / 2;
  });
}

MATCH_API int match_copy_matches(match_handle* handle, int32_t k, uint32_t* matches, int64_t capacity) {
  return Guard([&] {
    const PairResult& R = result_of(handle, k);
    const int64_t count = (int64_t)R.matches.size() / 2;
    MATCH_CHECK(capacity >= count, "capacity is smaller than the number of matches");
    MATCH_CHECK(count == 0 || matches != nullptr, "matches is null");
    if (count) std::memcpy(matches, R.matches.data(), R.matches.size() * sizeof(uint32_t));
  });
}

MATCH_API int match_num_rows(match_handle* handle, int32_t k, int32_t direction, int64_t* rows) {
  return Guard([&] {
    MATCH_CHECK(rows != nullptr, "rows is null");
    MATCH_CHECK(direction == 0 || direction == 1, "direction must be 0 or 1");
    *rows = result_of(handle, k).rows[direction];
  });
}

MATCH_API int match_copy_selection(match_handle* handle, int32_t k, int32_t direction, int32_t* out, int64_t capacity) {
  return Guard([&] {
    MATCH_CHECK(direction == 0 || direction == 1, "direction must be 0 or 1");
    const PairResult& R = result_of(handle, k);
    MATCH_CHECK(capacity >= R.rows[direction], "capacity is smaller than the number of rows");
    MATCH_CHECK(R.rows[direction] == 0 || out != nullptr, "out is null");
    if (R.rows[direction])
      std::memcpy(out, handle->out.data() + 3 * R.out_row0[direction], (size_t)R.rows[direction] * 3 * sizeof(int32_t));
  });
}

MATCH_API void match_cache_stats(match_handle* handle, int64_t* entries, int64_t* bytes, int64_t* evictions) {
  if (entries) *entries = handle ? (int64_t)handle->sets.size() : 0;
  if (bytes) *bytes = handle ? (int64_t)handle->resident_bytes : 0;
  if (evictions) *evictions = handle ? handle->evictions : 0;
}

MATCH_API int match_tile_rows(void) { return mp::kTileRows; }

MATCH_API void match_last_timing(double* kernel_ms, double* total_ms) {
  if (kernel_ms) *kernel_ms = g_kernel_ms;
  if (total_ms) *total_ms = g_total_ms;
}

MATCH_API void match_destroy(match_handle* handle) { delete handle; }

MATCH_API const char* match_last_error(void) { return g_error.c_str(); }

}  // extern "C"
