// pm_api.cpp -- host side of the PatchMatch C ABI (include/colmap_amd_pm.h).
//
// Mirrors the host half of the reference's PatchMatchCuda
// (src/colmap/mvs/patch_match_cuda.cu:1290-1939) in two parts. What is decided -- option/problem validation, pose
// tables for the four sweep directions, the shape of a run, the sweep schedule and its parameter blocks -- is plain
// C++ in pm_host_plan.h (namespace pm_host). This file owns the device side of it: memory pools, the image cache,
// uploads, streams, launches, the coalescing of concurrent runs; Create and RunBatchAsync build a plan, then do the
// device work the plan states. Which kernels a run launches is decided by pm_plan_run (pm_kernels.hip), where the
// device half lives. Compiled with hipcc; no CPU fallback: every entry point fails with an error if there is no
// usable HIP device.
#include "../../include/colmap_amd_pm.h"
#include "pm_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <stdexcept>
#include <string>
#include <vector>

using namespace colmap_amd;

namespace {

thread_local std::string g_last_error;

using PmError = pm_host::Fail;  // what PM_CHECK (pm_host_plan.h) throws

#define HIP_CALL(expr)                                                                  \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      throw PmError(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); \
  } while (0)

// Device buffers of destroyed handles are kept for the next handle of the same shape (a controller or a
// benchmark creates and destroys ~10 buffers of up to 1.3 GB per reference image: hipMalloc / hipFree
// would map, clear and unmap those pages every time and hipFree synchronises the device). Exact-size
// free lists per device; bounded by 64 GB unless pm_set_cached_memory_limit says otherwise; pm_release_cached_memory()
// returns everything to the driver. A buffer only comes back here after pm_destroy synchronised the
// handle's own stream AND the stream its last (batched) run was enqueued on, so the next user cannot
// race with the previous one. The cap is additionally bounded by a quarter of the device's memory,
// and a failed hipMalloc releases the pool and retries once (cached memory must never cause an OOM).
class DevPool {
 public:
  static DevPool& Get() {
    static DevPool* pool = new DevPool();  // never destroyed: no hipFree after the runtime is gone
    return *pool;
  }
  void* Take(int dev, size_t bytes) {
    std::lock_guard<std::mutex> lock(mu_);
    auto it = free_.find({dev, bytes});
    if (it == free_.end() || it->second.empty()) return nullptr;
    void* p = it->second.back();
    it->second.pop_back();
    pooled_ -= bytes;
    return p;
  }
  void Give(int dev, size_t bytes, void* p) {
    {
      std::lock_guard<std::mutex> lock(mu_);
      if (pooled_ + bytes <= cap_) {
        free_[{dev, bytes}].push_back(p);
        pooled_ += bytes;
        return;
      }
    }
    (void)hipFree(p);
  }
  // pm_set_cached_memory_limit: bytes the free lists may hold from now on (what is pooled beyond it goes back at once)
  void SetCap(size_t bytes) {
    bool shrink;
    {
      std::lock_guard<std::mutex> lock(mu_);
      cap_ = bytes;
      shrink = pooled_ > cap_;
    }
    if (shrink) Release();
  }
  void Release() {
    std::lock_guard<std::mutex> lock(mu_);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& kv : free_) {
      (void)hipSetDevice(kv.first.first);
      for (void* p : kv.second) (void)hipFree(p);
    }
    (void)hipSetDevice(cur);
    free_.clear();
    pooled_ = 0;
  }

 private:
  DevPool() {
    cap_ = 64ull << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) cap_ = std::min(cap_, total_b / 4);
  }
  std::mutex mu_;
  std::map<std::pair<int, size_t>, std::vector<void*>> free_;
  size_t pooled_ = 0, cap_ = 0;
};

template <typename T>
struct DevBuf {
  T* ptr = nullptr;
  size_t count = 0;
  int dev = -1;
  void alloc(size_t n) {
    free();
    if (n == 0) return;
    HIP_CALL(hipGetDevice(&dev));
    void* p = DevPool::Get().Take(dev, n * sizeof(T));
    if (!p) {
      hipError_t e = hipMalloc(&p, n * sizeof(T));
      if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        DevPool::Get().Release();
        e = hipMalloc(&p, n * sizeof(T));
      }
      HIP_CALL(e);
    }
    ptr = static_cast<T*>(p);
    count = n;
  }
  void free() {
    if (ptr) DevPool::Get().Give(dev, count * sizeof(T), ptr);
    ptr = nullptr;
    count = 0;
  }
  ~DevBuf() { free(); }
};

}  // namespace

// Packed source images come out of slabs of equally sized slots (one hipMalloc per slab, at most 3.5 GB):
// the images of a problem are then neighbours in the address space, which is what lets the 11 x 11 sweep kernels
// address all of them through ONE buffer resource (pm_kernels.hip: fp_resource -- every image must end within 4 GB
// of the lowest one). A problem whose sources straddle two slabs that lie further apart takes the explicit-index
// build of the kernels instead; nothing else depends on the slabs. Slots return to their slab when the last
// problem (or the image cache) drops the image; pm_release_cached_memory() frees the slabs that are empty.
// Test hook (pm_debug_set_image_slab_limits): slab size and the span one buffer resource may cover. The defaults are the
// hardware's (3.5 GB slabs, 32-bit buffer offsets); the tests shrink both to exercise the re-homing of shared images
// with a few small images instead of > 4 GB of them.
static size_t g_fp_slab_slots = 0;                 // 0: by image size (below)
static std::atomic<unsigned long long> g_fp_rehomed{0};

class FpSlabPool {
 public:
  static FpSlabPool& Get() {
    static FpSlabPool* pool = new FpSlabPool();  // leaked on purpose, like DevPool
    return *pool;
  }
  uint32_t* Take(size_t bytes) {
    int dev = 0;
    HIP_CALL(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu_);
    for (auto it = slabs_.rbegin(); it != slabs_.rend(); ++it)
      if (it->dev == dev && it->slot_bytes == bytes && !it->free_slots.empty()) {
        const int k = it->free_slots.back();
        it->free_slots.pop_back();
        return reinterpret_cast<uint32_t*>(it->base + (size_t)k * bytes);
      }
    Slab sl;
    sl.dev = dev;
    sl.slot_bytes = bytes;
    // slab size: 3.5 GB for full-size images (178 slots at 2560 x 1920), 256 MB for small ones
    const size_t target = bytes >= (4u << 20) ? (size_t)(3.5 * (1ull << 30)) : (256u << 20);
    int n = (int)std::max<size_t>(1, std::min<size_t>(4096, target / bytes));
    // test mode: n slots per slab and as much unused memory behind them, so that two slabs never fit one span
    const size_t pad = g_fp_slab_slots ? 2 : 1;
    if (g_fp_slab_slots) n = (int)g_fp_slab_slots;
    void* p = nullptr;
    hipError_t e = hipErrorOutOfMemory;
    for (; n >= 1; n /= 2) {  // a slab that does not fit any more shrinks down to a single slot
      e = hipMalloc(&p, pad * n * bytes);
      if (e == hipSuccess) break;
      (void)hipGetLastError();
      if (n == 1) break;
    }
    if (e == hipErrorOutOfMemory) {
      DevPool::Get().Release();
      n = 1;
      e = hipMalloc(&p, bytes);
    }
    HIP_CALL(e);
    sl.base = static_cast<char*>(p);
    sl.nslots = n;
    for (int k = n - 1; k >= 1; --k) sl.free_slots.push_back(k);
    slabs_.push_back(sl);
    return reinterpret_cast<uint32_t*>(sl.base);
  }
  // The slab (identified by its base address) that holds `ptr`; null for a pointer the pool does not own.
  const char* SlabOf(const uint32_t* ptr) {
    std::lock_guard<std::mutex> lock(mu_);
    const char* c = reinterpret_cast<const char*>(ptr);
    for (auto& sl : slabs_)
      if (c >= sl.base && c < sl.base + (size_t)sl.nslots * sl.slot_bytes) return sl.base;
    return nullptr;
  }
  // A free slot of the given slab, or null when it has none (or its slots have another size).
  uint32_t* TakeFrom(const char* slab, size_t bytes) {
    std::lock_guard<std::mutex> lock(mu_);
    for (auto& sl : slabs_)
      if (sl.base == slab && sl.slot_bytes == bytes && !sl.free_slots.empty()) {
        const int k = sl.free_slots.back();
        sl.free_slots.pop_back();
        return reinterpret_cast<uint32_t*>(sl.base + (size_t)k * bytes);
      }
    return nullptr;
  }
  // Free slots of the newest slab of this size on the current device (0: none).
  int FreeInNewest(size_t bytes, const char** slab) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu_);
    for (auto it = slabs_.rbegin(); it != slabs_.rend(); ++it)
      if (it->dev == dev && it->slot_bytes == bytes) {
        *slab = it->base;
        return (int)it->free_slots.size();
      }
    return 0;
  }
  void Give(uint32_t* ptr) {
    std::lock_guard<std::mutex> lock(mu_);
    char* c = reinterpret_cast<char*>(ptr);
    for (auto& sl : slabs_)
      if (c >= sl.base && c < sl.base + (size_t)sl.nslots * sl.slot_bytes) {
        sl.free_slots.push_back((int)((c - sl.base) / sl.slot_bytes));
        return;
      }
  }
  void Release() {  // frees the slabs none of whose slots is in use
    std::lock_guard<std::mutex> lock(mu_);
    int cur = 0;
    (void)hipGetDevice(&cur);
    size_t keep = 0;
    for (size_t i = 0; i < slabs_.size(); ++i) {
      if ((int)slabs_[i].free_slots.size() == slabs_[i].nslots) {
        (void)hipSetDevice(slabs_[i].dev);
        (void)hipFree(slabs_[i].base);
      } else {
        if (keep != i) slabs_[keep] = std::move(slabs_[i]);
        ++keep;
      }
    }
    slabs_.resize(keep);
    (void)hipSetDevice(cur);
  }

 private:
  struct Slab {
    char* base = nullptr;
    size_t slot_bytes = 0;
    int nslots = 0, dev = 0;
    std::vector<int> free_slots;
  };
  std::mutex mu_;
  std::vector<Slab> slabs_;
};

struct FpBuf {
  uint32_t* ptr = nullptr;
  size_t count = 0;
  void alloc(size_t n) {
    ptr = FpSlabPool::Get().Take(n * sizeof(uint32_t));
    count = n;
  }
  void adopt(uint32_t* p, size_t n) {  // a slot taken from the pool by the caller
    ptr = p;
    count = n;
  }
  ~FpBuf() {
    if (ptr) FpSlabPool::Get().Give(ptr);
  }
};

// A packed source image (2x2 footprints + zero ring) in HBM. Shared between problems through
// pm_image_cache: neighbouring reference images use mostly the same sources (28 distinct images
// for 8 consecutive references with S = 20), so a batch gathers from one copy instead of eight.
struct FpEntry {
  FpBuf data;
};

struct pm_image_cache {
  int device = 0;
  std::mutex mu;
  // key: (caller's bitmap pointer, image width, image height, slot width, slot height)
  using Key = std::tuple<const void*, int, int, int, int>;
  std::map<Key, std::shared_ptr<FpEntry>> entries;
  std::vector<Key> order;  // insertion order, for eviction
  size_t hits = 0, misses = 0;
  size_t bytes = 0, capacity = ~(size_t)0;

  // Drops the oldest entries no live problem references until the cache fits its capacity.
  void Trim() {
    size_t keep = 0;
    for (size_t i = 0; i < order.size(); ++i) {
      auto it = entries.find(order[i]);
      if (bytes > capacity && it != entries.end() && it->second.use_count() == 1) {
        bytes -= it->second->data.count * sizeof(uint32_t);
        entries.erase(it);
      } else {
        order[keep++] = order[i];
      }
    }
    order.resize(keep);
  }
};

// Problems alive per device (created, not yet destroyed): what a launch can expect to share the GPU with
// (RunBatchAsync: columns per wave by occupancy).
static std::atomic<int> g_live_handles[16];

struct pm_handle {
  pm_options opt;
  int device = 0;
  hipStream_t stream = nullptr;
  int W = 0, H = 0, S = 0, src_w = 0, src_h = 0;
  std::vector<int> src_idxs;
  pm_host::PoseTables tables;  // host pose tables
  // device buffers
  DevBuf<float> rec;
  std::vector<std::shared_ptr<FpEntry>> src_fp;  // per source image (possibly shared)
  DevBuf<const uint32_t*> src_fp_tab;
  DevBuf<float> src_depth;
  DevBuf<uint8_t> ref_img;
  DevBuf<float> ref_sum, ref_sqsum;
  DevBuf<uint32_t> rng;
  DevBuf<float> draws;  // the random numbers of one sweep per pixel (pm_draw_kernel), shapes served by the 11 x 11 kernel
  DevBuf<uint8_t> mask;
  DevBuf<float> poses;  // [4][S][43]
  DevBuf<float> out_depth, out_normal, out_sel, out_cost;
  DevBuf<unsigned long long> prof;
  DevBuf<unsigned long long> trace;  // progress trace of the last sweep launch (debug)
  DevBuf<uint32_t> src_fp_off;       // [S] the packed source images as slots of the problem's buffer resource
  const uint32_t* fp_base = nullptr; // its base (lowest address among them); null: the images lie too far apart
  const char* sweep_kernel = "";     // kernel of the last sweep launch (pm_get_sweep_kernel_name)
  DevBuf<unsigned long long> evals;  // [4] last run: NCC evaluations of the sweep launches; of them answered without taps;
                                     // evaluations of the initial cost answered without taps; sweep evaluations
                                     // pruned (PmParams::answered)
  DevBuf<PmParams> plan;  // per-launch parameter blocks of the last (batched) run
  hipStream_t run_stream = nullptr;  // stream the last run was enqueued on
  PmParams base;
  int threads = 64;
  int sweeps_done = 0;
  int final_sel_off = 0;
  bool ran = false;
  std::vector<hipEvent_t> ev;
  double sweep_ms = 0.0;
  int sweep_launches = 0;
  int launch_images = 1;       // reference images per sweep launch of the last run (its sub-batch)
  int launch_concurrency = 1;  // sub-batches of that run in flight together (RunBatchSplitAsync)

  bool counted = false;  // in g_live_handles
  ~pm_handle() {
    if (counted) --g_live_handles[device & 15];
    for (auto e : ev) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

PmParams ParamsForSweep(const pm_handle* h, int rot) {
  return pm_host::ParamsForSweep(h->base, h->tables, h->poses.ptr, rot);
}

pm_host::RunKey RunKeyOf(const pm_handle* h) { return pm_host::MakeRunKey(h->device, h->base, h->opt); }

int DeviceCUs(int device) {
  static std::atomic<int> cus[16];
  int ncu = cus[device & 15].load();
  if (ncu == 0) {
    HIP_CALL(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    ncu = std::max(ncu, 1);
    cus[device & 15] = ncu;
  }
  return ncu;
}

// Whether the packed images of `tab` can be read through one buffer resource, and as which slots of it.
pm_host::FpSpan SpanOf(const std::vector<const uint32_t*>& tab, size_t fp_count) {
  std::vector<uint64_t> addrs(tab.size());
  for (size_t s = 0; s < tab.size(); ++s) addrs[s] = (uint64_t)(uintptr_t)tab[s];
  return pm_host::PlanFpSpan(addrs.data(), (int)addrs.size(), fp_count,
                             pm_host::FpSpanLimit(g_fp_slab_slots, fp_count * sizeof(uint32_t)));
}

void RehomeSourceImages(pm_handle* h, pm_image_cache* cache, const pm_problem& prob, size_t fp_count,
                        std::vector<const uint32_t*>* tab) {
  FpSlabPool& pool = FpSlabPool::Get();
  const size_t bytes = fp_count * sizeof(uint32_t);
  const int S = h->S;
  std::vector<const char*> slab(S);
  for (int s = 0; s < S; ++s) slab[s] = pool.SlabOf((*tab)[s]);
  const char* newest = nullptr;
  if (pool.FreeInNewest(bytes, &newest) <= 0) newest = nullptr;
  auto try_slab = [&](const char* target) -> bool {
    std::vector<std::pair<int, uint32_t*>> moved;
    for (int s = 0; s < S; ++s) {
      if (slab[s] == target) continue;
      uint32_t* p = pool.TakeFrom(target, bytes);
      if (!p) {  // not enough room in this slab: hand the slots back
        for (auto& m : moved) pool.Give(m.second);
        return false;
      }
      moved.push_back({s, p});
    }
    // all copies first, one synchronisation, THEN the new entries become visible (to this handle and, through the
    // cache, to other threads' Create calls, which launch on their own streams): nobody can pick up a half-written
    // image. If a copy fails the taken slots go back to the pool and nothing has changed.
    try {
      for (auto& m : moved)
        HIP_CALL(hipMemcpyAsync(m.second, (*tab)[m.first], bytes, hipMemcpyDeviceToDevice, h->stream));
      HIP_CALL(hipStreamSynchronize(h->stream));
    } catch (...) {
      for (auto& m : moved) pool.Give(m.second);
      throw;
    }
    for (auto& m : moved) {
      const int s = m.first;
      auto e = std::make_shared<FpEntry>();
      e->data.adopt(m.second, fp_count);
      if (cache) {
        const pm_image& im = prob.images[h->src_idxs[s]];
        const auto key = std::make_tuple((const void*)im.gray, im.width, im.height, h->src_w, h->src_h);
        std::lock_guard<std::mutex> lock(cache->mu);
        auto it = cache->entries.find(key);
        if (it != cache->entries.end() && it->second == h->src_fp[s]) it->second = e;
      }
      h->src_fp[s] = e;   // (the old copy is released here at the earliest: the copies above are complete)
      (*tab)[s] = m.second;
      ++g_fp_rehomed;
    }
    return true;
  };
  for (const char* c : pm_host::RehomeCandidates(slab, newest))
    if (try_slab(c)) return;
  // every slab the problem touches is full: a fresh one (Take opens it when no slab has a free slot)
  uint32_t* probe = pool.Take(bytes);
  const char* fresh = pool.SlabOf(probe);
  pool.Give(probe);
  if (fresh && try_slab(fresh)) return;
  // no slab has room for all of them: the problem takes the explicit-index build of the kernels
}

void Create(const pm_options& opt_in, const pm_problem& prob, pm_image_cache* cache, pm_handle* h) {
  pm_host::CheckOptions(opt_in);
  pm_host::CheckProblem(opt_in, prob);
  h->opt = opt_in;
  const pm_options& opt = h->opt;

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    throw PmError("no HIP device available: the MI355X PatchMatch path has no CPU fallback");
  if (opt.gpu_index >= 0) {
    PM_CHECK(opt.gpu_index < ndev, "gpu_index < device count");
    h->device = opt.gpu_index;
  } else {
    HIP_CALL(hipGetDevice(&h->device));
  }
  HIP_CALL(hipSetDevice(h->device));
  if (cache) {
    // a cache holds device pointers of one GPU: bind it on first use, refuse another device later
    std::lock_guard<std::mutex> lock(cache->mu);
    if (cache->device < 0) cache->device = h->device;
    PM_CHECK(cache->device == h->device, "image cache and problem are on the same GPU");
  }
  HIP_CALL(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  ++g_live_handles[h->device & 15];
  h->counted = true;

  const pm_image& ref = prob.images[prob.ref_image_idx];
  h->W = ref.width;
  h->H = ref.height;
  h->S = prob.num_src_images;
  h->src_idxs.assign(prob.src_image_idxs, prob.src_image_idxs + prob.num_src_images);
  const int W = h->W, H = h->H, S = h->S;
  const hipMemcpyKind in_kind = opt.inputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;

  // ---- InitSourceImages (reference patch_match_cuda.cu:1595-1692) ------------------
  for (int s = 0; s < S; ++s) {
    const pm_image& im = prob.images[h->src_idxs[s]];
    h->src_w = std::max(h->src_w, im.width);
    h->src_h = std::max(h->src_h, im.height);
  }
  const size_t slot = (size_t)h->src_w * h->src_h;
  {
    DevBuf<uint8_t> staging;
    const size_t fp_count = pm_fp_entries(h->src_w, h->src_h);
    std::vector<const uint32_t*> tab(S);
    h->src_fp.resize(S);
    for (int s = 0; s < S; ++s) {
      const pm_image& im = prob.images[h->src_idxs[s]];
      std::shared_ptr<FpEntry> e;
      const auto key = std::make_tuple((const void*)im.gray, im.width, im.height, h->src_w, h->src_h);
      if (cache) {
        std::lock_guard<std::mutex> lock(cache->mu);
        auto it = cache->entries.find(key);
        if (it != cache->entries.end()) {
          e = it->second;
          ++cache->hits;
        }
      }
      if (!e) {
        e = std::make_shared<FpEntry>();
        e->data.alloc(fp_count);
        if (!staging.ptr) staging.alloc(slot);
        HIP_CALL(hipMemsetAsync(staging.ptr, 0, slot, h->stream));
        // contiguous copy into the max-size slot without re-pitching, exactly as the
        // reference's memcpy (patch_match_cuda.cu:1617-1622)
        HIP_CALL(hipMemcpyAsync(staging.ptr, im.gray, (size_t)im.width * im.height, in_kind, h->stream));
        pm_launch_build_footprint(staging.ptr, e->data.ptr, 1, h->src_w, h->src_h, h->stream);
        HIP_CALL(hipStreamSynchronize(h->stream));
        if (cache) {
          std::lock_guard<std::mutex> lock(cache->mu);
          // two threads may miss the same key at once: only the first insertion is accounted for, the
          // second adopts the entry that is already there
          const auto ins = cache->entries.emplace(key, e);
          ++cache->misses;
          if (ins.second) {
            cache->order.push_back(key);
            cache->bytes += fp_count * sizeof(uint32_t);
            cache->Trim();
          } else {
            e = ins.first->second;
          }
        }
      }
      h->src_fp[s] = e;
      tab[s] = e->data.ptr;
    }
    // One buffer resource per problem (pm_host::PlanFpSpan) needs the S images within 4 GB of each other. Images shared
    // through the cache may sit in slabs that lie further apart (a long run packs more images than one slab holds):
    // those of them outside the slab that holds most of the problem's images are then re-homed -- copied device to
    // device into a free slot of that slab, the cache handed the new copy; problems that still use the old one keep it
    // alive. Problems whose images still lie too far apart afterwards (separate allocations, shared through the image
    // cache) take the explicit-index build of the kernels (fp_base = null).
    pm_host::FpSpan span = SpanOf(tab, fp_count);
    if (!span.fits) {
      RehomeSourceImages(h, cache, prob, fp_count, &tab);
      span = SpanOf(tab, fp_count);
    }
    h->fp_base = span.fits ? reinterpret_cast<const uint32_t*>((uintptr_t)span.base) : nullptr;
    h->src_fp_tab.alloc(S);
    HIP_CALL(hipMemcpyAsync(h->src_fp_tab.ptr, tab.data(), S * sizeof(const uint32_t*), hipMemcpyHostToDevice,
                            h->stream));
    h->src_fp_off.alloc(S);
    HIP_CALL(hipMemcpyAsync(h->src_fp_off.ptr, span.offs.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice,
                            h->stream));
    HIP_CALL(hipStreamSynchronize(h->stream));  // `tab` and `span` die with this scope
  }
  if (opt.geom_consistency) {
    h->src_depth.alloc(slot * S);
    HIP_CALL(hipMemsetAsync(h->src_depth.ptr, 0, slot * S * sizeof(float), h->stream));
    for (int s = 0; s < S; ++s) {
      const pm_image& im = prob.images[h->src_idxs[s]];
      // row copy into the padded slot (patch_match_cuda.cu:1668-1673)
      HIP_CALL(hipMemcpy2DAsync(h->src_depth.ptr + slot * s, (size_t)h->src_w * sizeof(float),
                                im.depth_map, (size_t)im.width * sizeof(float),
                                (size_t)im.width * sizeof(float), im.height, in_kind, h->stream));
    }
  }

  // ---- InitRefImage (reference :1578-1593) ---------------------------------------
  h->ref_img.alloc((size_t)W * H);
  h->ref_sum.alloc((size_t)W * H);
  h->ref_sqsum.alloc((size_t)W * H);
  {
    DevBuf<uint8_t> gray;
    gray.alloc((size_t)W * H);
    HIP_CALL(hipMemcpyAsync(gray.ptr, ref.gray, (size_t)W * H, in_kind, h->stream));
    pm_launch_filter_ref(gray.ptr, W, H, opt.window_radius, opt.window_step, (float)opt.sigma_spatial,
                         (float)opt.sigma_color, h->ref_img.ptr, h->ref_sum.ptr, h->ref_sqsum.ptr,
                         h->stream);
    HIP_CALL(hipStreamSynchronize(h->stream));
  }

  // ---- InitTransforms -------------------------------------------------------------
  h->tables = pm_host::BuildPoseTables(prob, W, H, h->src_idxs);
  h->poses.alloc(h->tables.poses.size());
  HIP_CALL(hipMemcpyAsync(h->poses.ptr, h->tables.poses.data(), h->tables.poses.size() * sizeof(float),
                          hipMemcpyHostToDevice, h->stream));

  // ---- InitWorkspaceMemory (reference :1810-1857) ---------------------------------
  PmParams& b = h->base;
  b = pm_host::ShapeParams(opt, W, H, S, h->src_w, h->src_h);
  b.C = pm_pick_columns(S, b.ntaps, b.num_samples, opt.geom_consistency != 0, b.radius,
                        opt.columns_per_group);
  h->threads = pm_host::SweepThreads(opt.threads_per_group);

  h->rec.alloc((size_t)W * H * b.rec_stride);
  h->rng.alloc((size_t)W * H * kRngWords);
  b.rec = h->rec.ptr;
  b.src_fp_tab = h->src_fp_tab.ptr;
  b.fp_base = h->fp_base;
  b.src_fp_off = h->src_fp_off.ptr;
  b.src_depth = h->src_depth.ptr;
  b.ref_img = h->ref_img.ptr;
  b.ref_sum = h->ref_sum.ptr;
  b.ref_sqsum = h->ref_sqsum.ptr;
  b.rng = h->rng.ptr;
  b.mask = nullptr;
  b.draws = nullptr;
  // the 11 x 11 kernels read the sweep's random numbers from a per-pixel table (one column per wave is the
  // shape RunBatchAsync may lower to; if that fits the workgroup's LDS budget the table is needed)
  if (PmRunPlan::wave_kernels_fit(b, 1, opt.geom_consistency != 0)) {
    h->draws.alloc((size_t)W * H * pm_draw_stride(b.num_samples));
    b.draws = h->draws.ptr;
  }

  PmParams p0 = ParamsForSweep(h, 0);
  if (opt.geom_consistency) {
    DevBuf<float> d, n;
    d.alloc((size_t)W * H);
    n.alloc((size_t)3 * W * H);
    HIP_CALL(hipMemcpyAsync(d.ptr, ref.depth_map, (size_t)W * H * sizeof(float), in_kind, h->stream));
    HIP_CALL(hipMemcpyAsync(n.ptr, ref.normal_map, (size_t)3 * W * H * sizeof(float), in_kind,
                            h->stream));
    pm_launch_init_state(p0, false, 0.0f, 0.0f, d.ptr, n.ptr, h->stream);
    HIP_CALL(hipStreamSynchronize(h->stream));
  } else {
    pm_launch_init_state(p0, true, (float)opt.depth_min, (float)opt.depth_max, nullptr, nullptr,
                         h->stream);
  }
  if (opt.filter) {
    h->mask.alloc((size_t)S * W * H);
    b.mask = h->mask.ptr;
  }
  h->evals.alloc(4);
  b.evals = h->evals.ptr;
  b.answered = h->evals.ptr + 1;
  h->out_depth.alloc((size_t)W * H);
  h->out_normal.alloc((size_t)3 * W * H);
  h->out_sel.alloc((size_t)S * W * H);
  h->out_cost.alloc((size_t)S * W * H);
  const int total_sweeps = opt.num_iterations * 4;
  h->ev.resize((size_t)2 * total_sweeps);
  for (auto& e2 : h->ev) HIP_CALL(hipEventCreate(&e2));
  HIP_CALL(hipGetLastError());
  HIP_CALL(hipStreamSynchronize(h->stream));
}

// RunWithWindowSizeAndStep, reference patch_match_cuda.cu:1393-1546, for a batch of
// `n` problems of identical shape solved together: every kernel launch covers all n
// reference images (grid.y / grid.z = problem), so one sweep launch fills the GPU
// even when a single image has too few columns. All work is enqueued on hs[0]'s
// stream; n == 1 is the reference's one-problem-at-a-time Run().
void RunBatchAsync(pm_handle** hs, int n, hipStream_t run_st = nullptr) {
  PM_CHECK(n >= 1, "empty batch");
  pm_handle* h0 = hs[0];
  HIP_CALL(hipSetDevice(h0->device));
  // the stream the run is enqueued on: the first handle's own, or the caller's (sub-batches: RunBatchSplitAsync)
  const hipStream_t st = run_st ? run_st : h0->stream;
  if (run_st) HIP_CALL(hipStreamSynchronize(h0->stream));  // create-time work of the leader (the others: below)
  const pm_options& opt = h0->opt;
  for (int b = 1; b < n; ++b) {
    // (a caller may batch profiled or traced problems, which no run gathers on its own: kRunDebug passes)
    const pm_host::RunMismatch differ = pm_host::CompareRunKeys(RunKeyOf(h0), RunKeyOf(hs[b]));
    PM_CHECK(differ != pm_host::kRunDevice, "batch on one device");
    PM_CHECK(differ != pm_host::kRunSizes, "batched problems must have identical image sizes and source counts");
    PM_CHECK(differ != pm_host::kRunOptions,
             "batched problems must share window / sample / iteration / filter options");
    // work enqueued on other streams at create time must be complete
    HIP_CALL(hipStreamSynchronize(hs[b]->stream));
  }
  // One launch geometry for the batch (pm_host::PlanRunShape: columns per wave and helper wave by occupancy)
  const bool geom = opt.geom_consistency != 0;
  const int cols_switch = dev_switch_int("COLMAP_AMD_PM_COLS", 0);
  std::vector<pm_host::HandleColumns> cols(n);
  for (int b = 0; b < n; ++b) {
    const PmParams& s = hs[b]->base;
    const bool requested = hs[b]->opt.columns_per_group > 0;
    cols[b] = {!requested && cols_switch > 0 ? pm_pick_columns(s.S, s.ntaps, s.num_samples, geom, s.radius, cols_switch)
                                             : s.C,
               requested};
  }
  const int live = g_live_handles[h0->device & 15].load(), help_switch = dev_switch_int("COLMAP_AMD_PM_HELP", 0);
  pm_host::RunShape run_shape = pm_host::PlanRunShape(cols.data(), n, h0->base.ntaps, h0->W, h0->H, live,
                                                      DeviceCUs(h0->device), cols_switch, help_switch);
  // ... and three columns per wave where that shape is the faster one (a full GPU, photometric, S <= 21)
  const int narrow_C = run_shape.C;
  run_shape = pm_host::PlanWideColumns(run_shape, cols.data(), n, h0->base.ntaps, h0->base.S, geom, h0->W, h0->H, live,
                                       DeviceCUs(h0->device), cols_switch, help_switch,
                                       dev_switch_int("COLMAP_AMD_PM_WIDE", 1),
                                       PmRunPlan::wave_kernels_fit(h0->base, pm_host::kWideColumns, geom));
  // Which kernels the run launches, decided once. One kernel serves the whole batch: buffer-resource addressing only if
  // every problem's images allow it -- otherwise NO parameter block of the run carries a base.
  PmParams shape = h0->base;
  shape.C = run_shape.C;
  shape.help = run_shape.help;
  bool fp_base_all = true;
  for (int b = 0; b < n; ++b) fp_base_all = fp_base_all && hs[b]->fp_base != nullptr;
  const PmRunPlan run_plan = pm_plan_run(shape, geom, h0->threads, fp_base_all, h0->base.prof != nullptr,
                                         h0->base.draws != nullptr);
  // parameter blocks: [initial cost | sweep 0 | ... | sweep limit-1] x n problems
  const pm_host::SweepSchedule sched = pm_host::PlanSweeps(opt.num_iterations, opt.max_sweeps, opt.filter != 0, geom,
                                                           h0->base.sel_out_off, h0->base.sel_in_off);
  const int limit = (int)sched.sweeps.size();
  std::vector<pm_host::RunProblem> probs(n);
  for (int b = 0; b < n; ++b) probs[b] = {&hs[b]->base, &hs[b]->tables, hs[b]->poses.ptr};
  std::vector<PmParams> host = pm_host::FillParamBlocks(sched, probs.data(), n, run_shape,
                                                        dev_switch_int("COLMAP_AMD_PM_XCD_MAP", 0), run_plan.fp_resource);
  {  // COLMAP_AMD_PM_PRUNE (tests, A/B runs; read once per run): 0 = every listed evaluation runs (single-stage P4)
    const int prune = dev_switch_int("COLMAP_AMD_PM_PRUNE", 1) != 0 ? 1 : 0;
    for (PmParams& p : host) p.prune = prune;
  }
#ifdef COLMAP_AMD_DIAG_BUILD
  {  // diagnostics only (results are garbage): a fixed perturbation, to time a launch without far-flung random
     // hypotheses, and the ablations of the sweep kernels
    const double pert = dev_switch_double("COLMAP_AMD_PM_DIAG_PERT", -1.0);
    const int ablate = dev_switch_int("COLMAP_AMD_PM_ABLATE", 0);
    for (size_t i = n; i < host.size(); ++i) {
      if (pert >= 0.0) {
        host[i].perturbation = (float)pert;
        host[i].perturbation_pi = (float)(host[i].perturbation * M_PI);
      }
      host[i].ablate = ablate;
    }
  }
#endif
  h0->plan.alloc(host.size());
  HIP_CALL(hipMemcpyAsync(h0->plan.ptr, host.data(), host.size() * sizeof(PmParams),
                          hipMemcpyHostToDevice, st));
  // the stream-ordered copy reads `host` asynchronously only for pageable memory in
  // theory; make the lifetime explicit
  HIP_CALL(hipStreamSynchronize(st));

  for (int b = 0; b < n; ++b) {
    pm_handle* h = hs[b];
    if (h->mask.ptr) HIP_CALL(hipMemsetAsync(h->mask.ptr, 0, h->mask.count, st));
    if (h->prof.ptr)
      HIP_CALL(hipMemsetAsync(h->prof.ptr, 0, kPmProfSlots * sizeof(unsigned long long), st));
    HIP_CALL(hipMemsetAsync(h->evals.ptr, 0, 4 * sizeof(unsigned long long), st));
  }
  pm_launch_initial_cost(run_plan, h0->plan.ptr, n, st);
  for (int k = 0; k < limit; ++k) {
    const pm_host::Sweep& sweep = sched.sweeps[k];
    for (int b = 0; b < n; ++b)  // debug progress trace: every launch starts from an empty buffer
      if (hs[b]->trace.ptr)
        HIP_CALL(hipMemsetAsync(hs[b]->trace.ptr, 0, hs[b]->trace.count * sizeof(unsigned long long), st));
    pm_launch_draws(run_plan, sweep.rot, h0->plan.ptr + (size_t)(k + 1) * n, n, st);
    HIP_CALL(hipEventRecord(h0->ev[2 * k], st));   // the events bracket the sweep kernel alone
    pm_launch_sweep(run_plan, sweep.rot, h0->plan.ptr + (size_t)(k + 1) * n, n, sweep.filter_photo, sweep.filter_geom,
                    st);
    // (a launch the library widened is a shape of its own: what was measured on the two-column launch, such as
    // profiles/pm_sweep_traffic.json, does not describe it, so the run says which one it was)
    h0->sweep_kernel = run_shape.C != narrow_C && run_plan.sweep == kPmQuad && run_plan.fp_resource
                           ? "pm_sweep_quad_kernel (three columns)"
                           : run_plan.sweep_name;
    HIP_CALL(hipEventRecord(h0->ev[2 * k + 1], st));
  }
  for (int b = 0; b < n; ++b) {
    pm_handle* h = hs[b];
    h->sweeps_done = b == 0 ? limit : 0;
    h->final_sel_off = sched.final_sel_off;  // the half written by the last sweep
    PmParams pe = ParamsForSweep(h, 0);
    pm_launch_extract(pe, h->final_sel_off, h->out_depth.ptr, h->out_normal.ptr, h->out_sel.ptr,
                      h->out_cost.ptr, st);
    h->ran = true;
    h->run_stream = st;
  }
  HIP_CALL(hipGetLastError());
}

void RunAsync(pm_handle* h) {
  RunBatchAsync(&h, 1);
  h->launch_images = 1;
  h->launch_concurrency = 1;
}

// pm_run_batch: a batch of 16 or more problems runs as TWO sub-batches (pm_host::FirstSubBatch) on the
// streams of their first handles, enqueued back to back. A sweep launch ends with a drain -- the last of its column
// groups finish one by one while the rest of the GPU idles, and the next sweep of the same images cannot start before
// that -- but the problems of the other sub-batch do not depend on it: its launches fill the drain. Measured at
// 16 x 2560 x 1920: 7.74 -> 8.07 Mpix/s; three or four sub-batches lose again (7.6-7.7: problems spread over XCDs,
// more distinct source images per L2). Results cannot change: problems are independent.
// Streams of the two sub-batches, two per device, created once and never destroyed. They carry a CU mask with every
// CU enabled: a masked stream owns its hardware queue, while ordinary streams are dealt to a pool of four queues by
// use count -- the streams of two handles may share one, and two launches in one queue run one after the other
// (measured: the same 16-image run at 8.3 Mpix/s on one process's streams and 7.3 on another's).
hipStream_t SubBatchStream(int device, int k) {
  static std::mutex mu;
  static hipStream_t streams[16][2];
  std::lock_guard<std::mutex> lock(mu);
  hipStream_t& st = streams[device & 15][k & 1];
  if (!st) {
    int ncu = 0;
    HIP_CALL(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    std::vector<uint32_t> mask((size_t)(std::max(ncu, 1) + 31) / 32, 0u);
    for (int i = 0; i < ncu; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
    HIP_CALL(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
  }
  return st;
}

void RunBatchSplitAsync(pm_handle** hs, int n) {
  const int first = pm_host::FirstSubBatch(n, dev_switch_int("COLMAP_AMD_PM_BATCH_SPLIT", 1));
  if (first == n) {
    RunBatchAsync(hs, n);
    for (int b = 0; b < n; ++b) {
      hs[b]->launch_images = n;
      hs[b]->launch_concurrency = 1;
    }
    return;
  }
  RunBatchAsync(hs, first, SubBatchStream(hs[0]->device, 0));
  RunBatchAsync(hs + first, n - first, SubBatchStream(hs[0]->device, 1));
  for (int b = 0; b < n; ++b) {
    hs[b]->launch_images = b < first ? first : n - first;
    hs[b]->launch_concurrency = 2;
  }
}

void Synchronize(pm_handle* h) {
  HIP_CALL(hipSetDevice(h->device));
  HIP_CALL(hipStreamSynchronize(h->run_stream ? h->run_stream : h->stream));
  // the batch's work is complete: later copies use the handle's own stream (the stream of the
  // batch leader may be destroyed before this handle)
  h->run_stream = nullptr;
  h->sweep_ms = 0.0;
  h->sweep_launches = h->sweeps_done;
  for (int i = 0; i < h->sweeps_done; ++i) {
    float ms = 0.0f;
    HIP_CALL(hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]));
    h->sweep_ms += ms;
  }
}

template <typename T>
void CopyOut(pm_handle* h, const T* dev, T* out, size_t n) {
  PM_CHECK(h->ran, "pm_run must be called first");
  HIP_CALL(hipSetDevice(h->device));
  hipStream_t st = h->run_stream ? h->run_stream : h->stream;
  HIP_CALL(hipMemcpyAsync(out, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
  HIP_CALL(hipStreamSynchronize(st));
}

template <typename F>
int Guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return 1;
  } catch (...) {
    g_last_error = "unknown error";
    return 2;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// pm_run from several host threads at once -- how the reference's controller drives the seam, one problem per worker
// thread (mvs/patch_match.cc:190-204, its `gpu_index = 0,0,...` idiom for several problems per GPU) -- is coalesced:
// the calls that arrive together run as ONE batch (RunBatchSplitAsync: every launch covers all of them), each caller
// returns when its own problem is done. The first arrival leads: it waits while further calls keep arriving (until
// 300 us pass without one, at most 3 ms -- 250 ms while other threads are still inside pm_create --, or until every
// live handle of the device has called), runs the calls that can
// share launches with the oldest pending one (same image size / source count / options: what pm_run_batch requires),
// and hands leadership on. Results do not depend on it (a batch equals its single runs bit for bit); a lone caller pays
// at most the 300 us. COLMAP_AMD_PM_COALESCE=0 (development switch) runs every call on its own.
// ---------------------------------------------------------------------------------------------------------------
struct RunCall {
  pm_handle* h;
  bool done = false;
  std::string err;
};
struct RunCoalescer {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<RunCall*> pending;
  bool leader_active = false;
};
static RunCoalescer g_coalescer[16];
static std::atomic<int> g_creating{0};   // pm_create calls in progress (any device)

void RunCoalesced(pm_handle* h) {
  if (dev_switch_int("COLMAP_AMD_PM_COALESCE", 1) == 0 || h->base.prof || h->base.trace) {
    RunAsync(h);
    Synchronize(h);
    return;
  }
  RunCoalescer& Q = g_coalescer[h->device & 15];
  RunCall me{h};
  std::unique_lock<std::mutex> lock(Q.mu);
  Q.pending.push_back(&me);
  Q.cv.notify_all();  // a gathering leader counts arrivals
  while (!me.done) {
    if (Q.leader_active) {
      Q.cv.wait(lock);
      continue;
    }
    Q.leader_active = true;
    {
      // gather: while other threads are inside pm_create (they are about to call: the controller's workers create and
      // run in a loop) up to 250 ms, otherwise until 300 us pass without an arrival (at most 3 ms); never beyond the
      // number of live handles. A caller that is alone -- nobody creating, nobody arriving -- leaves after 300 us.
      const auto t0 = std::chrono::steady_clock::now();
      size_t seen = Q.pending.size();
      while ((int)seen < g_live_handles[h->device & 15].load() + g_creating.load()) {
        const auto waited = std::chrono::steady_clock::now() - t0;
        const bool others_creating = g_creating.load() > 0;
        if (waited > (others_creating ? std::chrono::milliseconds(250) : std::chrono::milliseconds(3))) break;
        Q.cv.wait_for(lock, std::chrono::microseconds(300));
        if (Q.pending.size() == seen && g_creating.load() == 0) break;  // quiet: nobody else is about to call
        seen = Q.pending.size();
      }
    }
    std::vector<RunCall*> batch, rest;
    for (RunCall* c : Q.pending) {
      const bool together = pm_host::CompareRunKeys(RunKeyOf(Q.pending[0]->h), RunKeyOf(c->h)) == pm_host::kRunMatch;
      (together ? batch : rest).push_back(c);
    }
    Q.pending.swap(rest);
    lock.unlock();
    std::string err;
    try {
      std::vector<pm_handle*> hs;
      for (RunCall* c : batch) hs.push_back(c->h);
      if (hs.size() == 1) {
        RunAsync(hs[0]);
      } else {
        RunBatchSplitAsync(hs.data(), (int)hs.size());
      }
      for (pm_handle* x : hs) Synchronize(x);
    } catch (const std::exception& e) {
      err = e.what();
      if (err.empty()) err = "pm_run failed";
    }
    lock.lock();
    for (RunCall* c : batch) {
      c->done = true;
      c->err = err;
    }
    Q.leader_active = false;
    Q.cv.notify_all();
  }
  lock.unlock();
  if (!me.err.empty()) throw std::runtime_error(me.err);
}

extern "C" {

void pm_options_init(pm_options* o) {
  // reference mvs/patch_match_options.h:37-126 (float literals narrowed like the source)
  std::memset(o, 0, sizeof(*o));
  o->depth_min = -1.0f;
  o->depth_max = -1.0f;
  o->sigma_spatial = -1;
  o->sigma_color = 0.2f;
  o->ncc_sigma = 0.6f;
  o->min_triangulation_angle = 1.0f;
  o->incident_angle_sigma = 0.9f;
  o->geom_consistency_regularizer = 0.3f;
  o->geom_consistency_max_cost = 3.0f;
  o->filter_min_ncc = 0.1f;
  o->filter_min_triangulation_angle = 3.0f;
  o->filter_geom_consistency_max_cost = 1.0f;
  o->window_radius = 5;
  o->window_step = 1;
  o->num_samples = 15;
  o->num_iterations = 5;
  o->filter_min_num_consistent = 2;
  o->geom_consistency = 1;
  o->filter = 1;
  o->gpu_index = -1;
}

int pm_check(const pm_options* options, const pm_problem* problem) {
  return Guard([&] {
    PM_CHECK(options && problem, "null argument");
    pm_host::CheckOptions(*options);
    pm_host::CheckProblem(*options, *problem);
  });
}

int pm_image_cache_create(int32_t gpu_index, pm_image_cache** out) {
  return Guard([&] {
    PM_CHECK(out, "null argument");
    PM_CHECK(gpu_index >= -1, "gpu_index >= -1");
    auto* c = new pm_image_cache();
    c->device = gpu_index;  // -1: the device of the first problem that uses the cache
    *out = c;
  });
}

void pm_image_cache_destroy(pm_image_cache* cache) { delete cache; }

int pm_image_cache_set_capacity(pm_image_cache* cache, size_t max_bytes) {
  return Guard([&] {
    PM_CHECK(cache, "null argument");
    std::lock_guard<std::mutex> lock(cache->mu);
    cache->capacity = max_bytes;
    cache->Trim();
  });
}

int pm_image_cache_stats(pm_image_cache* cache, size_t* entries, size_t* hits, size_t* misses) {
  return Guard([&] {
    PM_CHECK(cache, "null argument");
    std::lock_guard<std::mutex> lock(cache->mu);
    if (entries) *entries = cache->entries.size();
    if (hits) *hits = cache->hits;
    if (misses) *misses = cache->misses;
  });
}

static int CreateImpl(const pm_options* options, const pm_problem* problem, pm_image_cache* cache, pm_handle** out) {
  if (out) *out = nullptr;
  pm_handle* h = nullptr;
  struct Creating {   // a pm_run that gathers concurrent calls waits for creations in flight (RunCoalesced)
    Creating() { ++g_creating; }
    ~Creating() { --g_creating; }
  } creating;
  const int rc = Guard([&] {
    PM_CHECK(options && problem && out, "null argument");
    h = new pm_handle();
    Create(*options, *problem, cache, h);
  });
  if (rc != 0) {
    delete h;
    return rc;
  }
  *out = h;
  return 0;
}

int pm_create(const pm_options* options, const pm_problem* problem, pm_handle** out) {
  return CreateImpl(options, problem, nullptr, out);
}

int pm_create_cached(const pm_options* options, const pm_problem* problem, pm_image_cache* cache,
                     pm_handle** out) {
  return CreateImpl(options, problem, cache, out);
}

int pm_run_async(pm_handle* h) {
  return Guard([&] {
    PM_CHECK(h, "null handle");
    RunAsync(h);
  });
}

int pm_synchronize(pm_handle* h) {
  return Guard([&] {
    PM_CHECK(h, "null handle");
    Synchronize(h);
  });
}

int pm_run(pm_handle* h) {
  return Guard([&] {
    PM_CHECK(h, "null handle");
    RunCoalesced(h);
  });
}

int pm_run_batch_async(pm_handle** handles, int32_t n) {
  return Guard([&] {
    PM_CHECK(handles && n >= 1, "empty batch");
    for (int i = 0; i < n; ++i) PM_CHECK(handles[i], "null handle");
    RunBatchSplitAsync(handles, n);
  });
}

int pm_run_batch(pm_handle** handles, int32_t n) {
  return Guard([&] {
    PM_CHECK(handles && n >= 1, "empty batch");
    for (int i = 0; i < n; ++i) PM_CHECK(handles[i], "null handle");
    RunBatchSplitAsync(handles, n);
    for (int i = 0; i < n; ++i) Synchronize(handles[i]);
  });
}

int pm_get_depth_map(pm_handle* h, float* out) {
  return Guard([&] { PM_CHECK(h && out, "null"); CopyOut(h, h->out_depth.ptr, out, (size_t)h->W * h->H); });
}
int pm_get_normal_map(pm_handle* h, float* out) {
  return Guard([&] { PM_CHECK(h && out, "null"); CopyOut(h, h->out_normal.ptr, out, (size_t)3 * h->W * h->H); });
}
int pm_get_sel_prob_map(pm_handle* h, float* out) {
  return Guard([&] { PM_CHECK(h && out, "null"); CopyOut(h, h->out_sel.ptr, out, (size_t)h->S * h->W * h->H); });
}
int pm_get_cost_map(pm_handle* h, float* out) {
  return Guard([&] { PM_CHECK(h && out, "null"); CopyOut(h, h->out_cost.ptr, out, (size_t)h->S * h->W * h->H); });
}

int pm_get_consistency_mask(pm_handle* h, uint8_t* out) {
  return Guard([&] {
    PM_CHECK(h && out, "null");
    const size_t n = (size_t)h->S * h->W * h->H;
    if (h->mask.ptr) CopyOut(h, h->mask.ptr, out, n);
    else std::memset(out, 0, n);
  });
}

int pm_get_consistent_image_idxs(pm_handle* h, int32_t* buf, size_t capacity, size_t* count) {
  // GetConsistentImageIdxs, reference patch_match_cuda.cu:1367-1391
  return Guard([&] {
    PM_CHECK(h && count, "null");
    const size_t n = (size_t)h->S * h->W * h->H;
    std::vector<uint8_t> mask(n, 0);
    if (h->mask.ptr) CopyOut(h, h->mask.ptr, mask.data(), n);
    std::vector<int32_t> out;
    std::vector<int32_t> pix;
    for (int r = 0; r < h->H; ++r) {
      for (int c = 0; c < h->W; ++c) {
        pix.clear();
        for (int d = 0; d < h->S; ++d)
          if (mask[((size_t)d * h->H + r) * h->W + c]) pix.push_back(h->src_idxs[d]);
        if (!pix.empty()) {
          out.push_back(c);
          out.push_back(r);
          out.push_back((int32_t)pix.size());
          out.insert(out.end(), pix.begin(), pix.end());
        }
      }
    }
    *count = out.size();
    if (buf) {
      PM_CHECK(capacity >= out.size(), "buffer too small");
      std::memcpy(buf, out.data(), out.size() * sizeof(int32_t));
    }
  });
}

int pm_get_ref_filter(pm_handle* h, uint8_t* image, float* sum, float* sqsum) {
  return Guard([&] {
    PM_CHECK(h, "null");
    HIP_CALL(hipSetDevice(h->device));
    const size_t n = (size_t)h->W * h->H;
    if (image) HIP_CALL(hipMemcpy(image, h->ref_img.ptr, n, hipMemcpyDeviceToHost));
    if (sum) HIP_CALL(hipMemcpy(sum, h->ref_sum.ptr, n * sizeof(float), hipMemcpyDeviceToHost));
    if (sqsum) HIP_CALL(hipMemcpy(sqsum, h->ref_sqsum.ptr, n * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int pm_get_pose_tables(pm_handle* h, float* poses, float* ref_K, float* ref_inv_K) {
  return Guard([&] {
    PM_CHECK(h, "null");
    const pm_host::PoseTables& t = h->tables;
    if (poses) std::memcpy(poses, t.poses.data(), t.poses.size() * sizeof(float));
    if (ref_K) std::memcpy(ref_K, t.ref_K, sizeof(t.ref_K));
    if (ref_inv_K) std::memcpy(ref_inv_K, t.ref_inv_K, sizeof(t.ref_inv_K));
  });
}

int pm_debug_rng_streams(int32_t gpu_index, const uint64_t* seeds, int32_t nseeds, int32_t ndraws,
                         float* out) {
  return Guard([&] {
    PM_CHECK(seeds && out && nseeds > 0 && ndraws > 0, "bad arguments");
    HIP_CALL(hipSetDevice(gpu_index));
    DevBuf<unsigned long long> d_seeds;
    DevBuf<float> d_out;
    d_seeds.alloc((size_t)nseeds);
    d_out.alloc((size_t)nseeds * ndraws);
    HIP_CALL(hipMemcpy(d_seeds.ptr, seeds, sizeof(uint64_t) * nseeds, hipMemcpyHostToDevice));
    pm_launch_rng_streams(d_seeds.ptr, nseeds, ndraws, d_out.ptr, nullptr);
    HIP_CALL(hipDeviceSynchronize());
    HIP_CALL(hipMemcpy(out, d_out.ptr, sizeof(float) * (size_t)nseeds * ndraws, hipMemcpyDeviceToHost));
  });
}

int pm_get_sweep_timing(pm_handle* h, double* total_ms, int32_t* num_launches) {
  return Guard([&] {
    PM_CHECK(h, "null");
    if (total_ms) *total_ms = h->sweep_ms;
    if (num_launches) *num_launches = h->sweep_launches;
  });
}

int pm_get_launch_shape(pm_handle* h, int32_t* images_per_launch, int32_t* concurrent_launches) {
  return Guard([&] {
    PM_CHECK(h, "null");
    if (images_per_launch) *images_per_launch = h->launch_images;
    if (concurrent_launches) *concurrent_launches = h->launch_concurrency;
  });
}

int pm_get_sweep_kernel_name(pm_handle* h, const char** name) {
  return Guard([&] {
    PM_CHECK(h && name, "null");
    *name = h->sweep_kernel;
  });
}

int pm_get_sweep_times(pm_handle* h, float* ms, int32_t capacity, int32_t* num_launches) {
  return Guard([&] {
    PM_CHECK(h && num_launches, "null");
    *num_launches = h->sweep_launches;
    for (int i = 0; ms && i < h->sweep_launches && i < capacity; ++i)
      HIP_CALL(hipEventElapsedTime(&ms[i], h->ev[2 * i], h->ev[2 * i + 1]));
  });
}

int pm_get_device_maps(pm_handle* h, const float** depth, const float** normal) {
  return Guard([&] {
    PM_CHECK(h && h->ran, "run first");
    if (depth) *depth = h->out_depth.ptr;
    if (normal) *normal = h->out_normal.ptr;
  });
}

int pm_copy_maps_to_device(pm_handle* h, float* depth_dev, float* normal_dev) {
  return Guard([&] {
    PM_CHECK(h && h->ran, "run first");
    HIP_CALL(hipSetDevice(h->device));
    const size_t n = (size_t)h->W * h->H;
    if (depth_dev)
      HIP_CALL(hipMemcpyAsync(depth_dev, h->out_depth.ptr, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (normal_dev)
      HIP_CALL(hipMemcpyAsync(normal_dev, h->out_normal.ptr, 3 * n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIP_CALL(hipStreamSynchronize(h->stream));
  });
}

int pm_get_evaluation_count(pm_handle* h, unsigned long long* sweep_evals, unsigned long long* initial_evals) {
  return Guard([&] {
    PM_CHECK(h && h->ran, "pm_run must be called first");
    HIP_CALL(hipSetDevice(h->device));
    if (sweep_evals)
      HIP_CALL(hipMemcpy(sweep_evals, h->evals.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (initial_evals) *initial_evals = (unsigned long long)h->W * h->H * h->S;  // ComputeInitialCost
  });
}

int pm_get_answered_count(pm_handle* h, unsigned long long* sweep_answered, unsigned long long* initial_answered) {
  return Guard([&] {
    PM_CHECK(h && h->ran, "pm_run must be called first");
    HIP_CALL(hipSetDevice(h->device));
    unsigned long long both[2];
    HIP_CALL(hipMemcpy(both, h->evals.ptr + 1, sizeof(both), hipMemcpyDeviceToHost));
    if (sweep_answered) *sweep_answered = both[0];
    if (initial_answered) *initial_answered = both[1];
  });
}

int pm_get_pruned_count(pm_handle* h, unsigned long long* sweep_pruned) {
  return Guard([&] {
    PM_CHECK(h && h->ran, "pm_run must be called first");
    HIP_CALL(hipSetDevice(h->device));
    if (sweep_pruned)
      HIP_CALL(hipMemcpy(sweep_pruned, h->evals.ptr + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  });
}

int pm_enable_phase_profile(pm_handle* h, int enable) {
  return Guard([&] {
    PM_CHECK(h, "null");
    HIP_CALL(hipSetDevice(h->device));
    if (enable) {
      h->prof.alloc(kPmProfSlots);
      h->base.prof = h->prof.ptr;
    } else {
      h->base.prof = nullptr;
    }
  });
}

int pm_enable_progress_trace(pm_handle* h, int enable) {
  return Guard([&] {
    PM_CHECK(h, "null");
    HIP_CALL(hipSetDevice(h->device));
    if (enable) {
      const int longest = std::max(h->W, h->H);
      h->base.trace_stride = longest / 128 + 2;
      const size_t groups = (size_t)longest;  // one column per wave is the finest launch shape (RunBatchAsync may choose it)
      h->trace.alloc(groups * h->base.trace_stride);
      HIP_CALL(hipMemset(h->trace.ptr, 0, groups * h->base.trace_stride * sizeof(unsigned long long)));
      h->base.trace = h->trace.ptr;
    } else {
      h->base.trace = nullptr;
    }
  });
}

int pm_get_progress_trace(pm_handle* h, unsigned long long* out, size_t capacity, int32_t* groups, int32_t* samples) {
  return Guard([&] {
    PM_CHECK(h && h->trace.ptr && groups && samples, "trace not enabled");
    HIP_CALL(hipSetDevice(h->device));
    *samples = h->base.trace_stride;
    *groups = (int32_t)(h->trace.count / h->base.trace_stride);
    if (out) {
      PM_CHECK(capacity >= h->trace.count, "buffer too small");
      HIP_CALL(hipMemcpy(out, h->trace.ptr, h->trace.count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
  });
}

int pm_get_phase_profile(pm_handle* h, unsigned long long* out10) {
  return Guard([&] {
    PM_CHECK(h && out10 && h->prof.ptr, "profile not enabled");
    HIP_CALL(hipSetDevice(h->device));
    HIP_CALL(hipMemcpy(out10, h->prof.ptr, 10 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  });
}

int pm_get_phase_profile_slots(pm_handle* h, unsigned long long* out, int32_t capacity) {
  return Guard([&] {
    PM_CHECK(h && out && h->prof.ptr, "profile not enabled");
    PM_CHECK(capacity >= kPmProfSlots, "buffer too small");
    HIP_CALL(hipSetDevice(h->device));
    HIP_CALL(hipMemcpy(out, h->prof.ptr, kPmProfSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  });
}

void pm_destroy(pm_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  // a non-leader handle of a batched run has its kernels on the leader's stream; that stream may
  // already be destroyed (the leader went first), in which case only a device-wide wait is safe
  // (pm_synchronize resets run_stream, so this is the exception / GC path only)
  if (h->run_stream && h->run_stream != h->stream) (void)hipDeviceSynchronize();
  delete h;
}

int pm_set_cached_memory_limit(double gigabytes) {
  return Guard([&] {
    PM_CHECK(gigabytes >= 0.0 && gigabytes <= 1e6, "limit in GB, >= 0");
    DevPool::Get().SetCap(static_cast<size_t>(gigabytes * (double)(1ull << 30)));
  });
}

void pm_release_cached_memory(void) {
  DevPool::Get().Release();
  FpSlabPool::Get().Release();
}

unsigned long long pm_debug_set_image_slab_slots(size_t slots) {
  g_fp_slab_slots = slots;
  return g_fp_rehomed.load();
}

size_t pm_debug_wave_lds_bytes(int32_t num_sources, int32_t num_samples, int32_t columns, int32_t geom) {
  return pm_quad_lds_bytes(num_sources, num_samples, columns, geom != 0);
}

int32_t pm_debug_pick_columns(int32_t num_sources, int32_t num_samples, int32_t geom) {
  return pm_pick_columns(num_sources, 121, num_samples, geom != 0, 5, 0);
}

const char* pm_last_error(void) { return g_last_error.c_str(); }

int pm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"
