// fusion_plan.h -- everything a depth-map fusion run decides on the host before and between its device calls: the
// checks on the caller's input, the fusion order, the image descriptors, the pool schedule of an image, the limits of
// a walk, the window of ticks of a pass, and the per-thread concatenation of the result. Plain C++17: no HIP runtime,
// no hipCUB, no switches (their values come in as ints) -- Run (fusion.hip) builds the plan, hands it to the workspace
// that owns the device buffers, and drives the passes with it; tests/cpp/test_fusion_plan.cc checks it without a GPU.
#ifndef COLMAP_AMD_FUSION_PLAN_H_
#define COLMAP_AMD_FUSION_PLAN_H_

#include "../../include/colmap_amd_fusion.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

struct fusion_result {
  std::vector<float> xyz_normal;
  std::vector<uint8_t> rgb;
  std::vector<int64_t> vis_ptr{0};
  std::vector<int32_t> vis_idx;
};

namespace fusion_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define FU_CHECK(cond, msg)                                                        \
  do {                                                                             \
    if (!(cond)) throw ::fusion_plan::Fail(std::string("Check failed: ") + (msg)); \
  } while (0)

// Pixels one walk can record: max_num_pixels itself between 1 024 and 16 384 (the reference's default 10 000 is NOT
// clamped), smaller options keep 1 024, larger ones are clamped to 16 384. oracle/fusion_oracle.cpp mirrors it.
constexpr int kElemCapMin = 1024, kElemCapMax = 16384;
inline int record_capacity(int max_num_pixels) { return std::min(std::max(max_num_pixels, kElemCapMin), kElemCapMax); }
constexpr int kRowStride = 10;        // rows of a pool task (fusion.cc:250-254)
constexpr int kWave = 64;
constexpr int kWindowFirst = 256, kWindowMin = 16, kWindowMax = 32768;  // ticks of a pass: doubled after a pass without a cut, halved after a cut (8192 -> 32768: 0.695 -> 0.667 s at 8 x 2560 x 1920)
constexpr int kTableBytes = 20 * 1024;  // LDS copy of the image descriptors + overlap lists of the walk kernel, when they fit

struct DevImage {
  float P[12], inv_P[12], inv_R[9];
  float sx, sy;          // depth map size / model image size
  const uint8_t* rgb;    // [bh][bw][3] or nullptr
  int dw, dh, bw, bh;
  long long pix_off;     // global offset of the image's first pixel (word / depth / normal arrays)
  int pos;               // step at which the image is fused; -1: not used
};

static_assert(sizeof(DevImage) % 8 == 0, "descriptors are copied to LDS word by word and hold 8-byte members");

// mvs/image.cc:106-135
inline void ComposeProjectionMatrix(const float K[9], const float R[9], const float T[3], float P[12]) {
  float RT[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) RT[4 * r + c] = R[3 * r + c];
    RT[4 * r + 3] = T[r];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) P[4 * r + c] = K[3 * r] * RT[c] + K[3 * r + 1] * RT[4 + c] + K[3 * r + 2] * RT[8 + c];
}

// top three rows of [P; 0 0 0 1]^-1 = [M^-1 | -M^-1 p], M^-1 by the adjugate
inline void ComposeInverseProjectionMatrix(const float P[12], float inv_P[12]) {
  const float a = P[0], b = P[1], c = P[2], d = P[4], e = P[5], f = P[6], g = P[8], h = P[9], i = P[10];
  const float A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const float det = a * A + b * B + c * C;
  const float inv_det = 1.0f / det;
  const float Mi[9] = {A * inv_det, -(b * i - c * h) * inv_det, (b * f - c * e) * inv_det,
                       B * inv_det, (a * i - c * g) * inv_det,  -(a * f - c * d) * inv_det,
                       C * inv_det, -(a * h - b * g) * inv_det, (a * e - b * d) * inv_det};
  for (int r = 0; r < 3; ++r) {
    for (int col = 0; col < 3; ++col) inv_P[4 * r + col] = Mi[3 * r + col];
    inv_P[4 * r + 3] = -(Mi[3 * r] * P[3] + Mi[3 * r + 1] * P[7] + Mi[3 * r + 2] * P[11]);
  }
}

// ---- the pool schedule of one image ----

inline int stripes(int height) { return (int)(((long long)height + kRowStride - 1) / kRowStride); }

// pool threads: one wave each. num_threads <= 0: one thread per stripe (the reference's default pool, all cores, is at
// least that large for ordinary images and then behaves the same in step).
inline int pool_threads(int height, int num_threads) {
  const int ns = stripes(height);
  return num_threads <= 0 ? ns : std::min(num_threads, ns);
}

// T threads take the ns stripes of ten rows in G groups; a stripe lasts L = 10 W ticks, the image `ticks`; the turns
// have the ranks tick * T + thread, all below r_end.
struct Schedule {
  int W, H, ns_px, ns, T, G;
  unsigned L;
  unsigned long long ticks, r_end;
};

inline Schedule make_schedule(int dw, int dh, int num_threads) {
  Schedule s;
  s.W = dw; s.H = dh; s.ns_px = dw * dh;
  s.ns = stripes(dh);
  s.T = pool_threads(dh, num_threads);
  s.G = (s.ns + s.T - 1) / s.T;
  const unsigned long long L = (unsigned long long)kRowStride * dw;
  s.ticks = (unsigned long long)s.G * L;
  s.r_end = s.ticks * (unsigned long long)s.T;
  FU_CHECK(s.r_end < 0xFFFFFFF0ull, "turns of one image < 2^32");
  s.L = (unsigned)L;
  return s;
}

// ---- the run plan ----

struct RunPlan {
  std::vector<int> order;        // used images in fusion order (FindNextImage, fusion.cc:51-73)
  std::vector<int> pos;          // [n] step at which an image is fused; -1: not used
  std::vector<DevImage> images;  // [n] descriptors; rgb is null (it is a device pointer: set after the colour upload)
  long long total_pix = 0;       // depth-map pixels of the used images
  int max_seeds = 0, max_height = 1, max_threads = 1, max_overlap = 1;
};

// Checks the caller's lists and images, then computes. Nothing is read through overlap_ptr / overlap_idx before the
// checks on them have passed, and they are made whether or not any image is used.
inline RunPlan make_plan(const fusion_options& opt, int n, const fusion_image* images, const int32_t* optr,
                         const int32_t* oidx) {
  FU_CHECK(optr[0] == 0, "overlap_ptr[0] == 0");
  for (int i = 0; i < n; ++i) FU_CHECK(optr[i + 1] >= optr[i], "overlap_ptr does not decrease");
  RunPlan plan;
  for (int i = 0; i < n; ++i) {
    FU_CHECK(optr[i + 1] - optr[i] < (1 << 20), "overlap list length");
    plan.max_overlap = std::max(plan.max_overlap, optr[i + 1] - optr[i]);
  }
  for (int k = 0; k < (n > 0 ? optr[n] : 0); ++k) FU_CHECK(oidx[k] >= 0 && oidx[k] < n, "overlap index");
  for (int i = 0; i < n; ++i) {
    const fusion_image& im = images[i];
    if (!im.used) continue;
    FU_CHECK(im.depth_map && im.normal_map && im.depth_width > 0 && im.depth_height > 0, "depth / normal map");
    FU_CHECK(im.width > 0 && im.height > 0, "image size");
    FU_CHECK((int64_t)im.depth_width * im.depth_height < (1ll << 31), "depth map size");
    if (im.rgb) FU_CHECK(im.bitmap_width > 0 && im.bitmap_height > 0, "bitmap size");
  }
  FU_CHECK(n < 65536, "at most 65535 images");
  FU_CHECK(opt.max_traversal_depth <= 32767, "max_traversal_depth <= 32767");

  // fusion order (FindNextImage, fusion.cc:51-73): depends on the overlap lists only
  std::vector<char> fused(n > 0 ? n : 0, 0);
  plan.pos.assign(fused.size(), -1);
  if (n > 0) {
    for (int cur = 0; cur >= 0;) {
      if (images[cur].used) {
        plan.pos[cur] = (int)plan.order.size();
        plan.order.push_back(cur);
      }
      fused[cur] = 1;
      int nxt = -1;
      for (int k = optr[cur]; k < optr[cur + 1] && nxt < 0; ++k)
        if (images[oidx[k]].used && !fused[oidx[k]]) nxt = oidx[k];
      for (int i = 0; i < n && nxt < 0; ++i)
        if (images[i].used && !fused[i]) nxt = i;
      cur = nxt;
    }
  }

  plan.images.resize(fused.size());
  for (int i = 0; i < n; ++i) {
    DevImage& d = plan.images[i];
    std::memset(&d, 0, sizeof(d));
    d.pos = plan.pos[i];
    const fusion_image& im = images[i];
    if (!im.used) continue;
    const size_t npix = (size_t)im.depth_width * im.depth_height;
    d.sx = static_cast<float>(im.depth_width) / im.width;
    d.sy = static_cast<float>(im.depth_height) / im.height;
    float K[9];
    std::memcpy(K, im.K, sizeof(K));
    K[0] *= d.sx; K[2] *= d.sx;
    K[4] *= d.sy; K[5] *= d.sy;
    ComposeProjectionMatrix(K, im.R, im.T, d.P);
    ComposeInverseProjectionMatrix(d.P, d.inv_P);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) d.inv_R[3 * r + c] = im.R[3 * c + r];
    d.dw = im.depth_width; d.dh = im.depth_height; d.bw = im.bitmap_width; d.bh = im.bitmap_height;
    d.pix_off = plan.total_pix;
    plan.total_pix += (long long)npix;
    plan.max_seeds = std::max(plan.max_seeds, (int)npix);
    plan.max_height = std::max(plan.max_height, im.depth_height);
  }
  plan.max_threads = pool_threads(plan.max_height, opt.num_threads);
  return plan;
}

// ---- the limits of a walk, and what follows from them for the workspace ----

struct Switches {  // development switches COLMAP_AMD_FUSION_LDS_TABLES / _WIDE / _WINDOW_FIRST / _WINDOW_MAX
  int lds_tables = 2, wide = 1, window_first = kWindowFirst, window_max = kWindowMax;
};

struct WalkLimits {
  int rec_cap;                  // record_capacity(max_num_pixels), at most the pixels of the workspace
  int elem_cap;                 // min(max_num_pixels, rec_cap)
  int max_level;                // max_traversal_depth - 1
  int min_num_pixels;
  double max_depth_error;
  float max_sq_reproj, min_cos_normal;
  float bmin[3], bmax[3];
  // what the walk kernel copies into LDS: 1 = image descriptors + overlap offsets, 2 = also the overlap lists;
  // 0 = neither fits kTableBytes
  int lds_tables;
  // breadth-first walks where their result provably equals the depth-first one: lanes per popped entry (0 = depth-first
  // walks only), and the walk size up to which the absorbed set cannot depend on the order of the traversal
  int wide_group, wide_bound;
  long long spill_bound;        // a stack can never hold more than (pixels a walk records) x (longest overlap list) entries
  // The visibility pool is refilled per reference image (cursor reset every step) and its int offsets only have to cover
  // what ONE image's walks absorb: capacity min(total pixels, 2^31 - 1), an overflow fails the run instead of wrapping.
  long long pool_cap;
  // Schedule knobs for experiments (the result does not depend on them: bit-exact against the sequential algorithm for
  // any window)
  int window_first, window_max;
};

inline WalkLimits make_limits(const fusion_options& opt, long long total_pix, int n, int n_overlap, int max_overlap,
                              const Switches& sw) {
  WalkLimits w;
  w.rec_cap = (int)std::min<long long>(record_capacity(opt.max_num_pixels), std::max<long long>(total_pix, 1));
  w.elem_cap = std::min(opt.max_num_pixels, w.rec_cap);
  w.max_level = opt.max_traversal_depth - 1;
  w.min_num_pixels = opt.min_num_pixels;
  w.max_depth_error = opt.max_depth_error;
  w.max_sq_reproj = static_cast<float>(opt.max_reproj_error * opt.max_reproj_error);
  w.min_cos_normal = static_cast<float>(std::cos(opt.max_normal_error * 0.017453292519943295769));
  for (int c = 0; c < 3; ++c) { w.bmin[c] = opt.bbox_min[c]; w.bmax[c] = opt.bbox_max[c]; }
  const size_t desc = (size_t)n * sizeof(DevImage) + ((size_t)n + 1) * sizeof(int);
  w.lds_tables = desc > (size_t)kTableBytes ? 0 : (desc + (size_t)n_overlap * sizeof(int) > (size_t)kTableBytes ? 1 : 2);
  w.lds_tables = std::min(w.lds_tables, std::max(0, sw.lds_tables));
  const int bound = std::min(std::min(w.max_level, w.elem_cap - 1), w.rec_cap);
  const bool wide = sw.wide != 0 && max_overlap <= kWave / 2 && bound >= 16;
  w.wide_group = wide ? std::max(max_overlap, 1) : 0;
  w.wide_bound = bound;
  w.spill_bound = (long long)w.rec_cap * max_overlap + kWave;
  w.pool_cap = std::min<long long>(total_pix, 0x7FFFFFFFll);
  w.window_first = std::max(1, sw.window_first);
  w.window_max = std::max(w.window_first, sw.window_max);
  return w;
}

// ---- the window of ticks of a pass ----

// ticks [tau0 (+1 for threads below rmod), tau_end), ranks below `limit`
struct Pass {
  unsigned tau0, rmod, tau_end, limit;
};

// Ranks [r_next, limit) are walked speculatively, [r_next, rstar) commit; the next pass starts at rstar with half the
// window after a cut and twice the window otherwise.
struct PassWindow {
  unsigned long long r_next = 0;
  long long window;
  explicit PassWindow(int window_first) : window(window_first) {}

  Pass pass(const Schedule& s) const {
    const unsigned long long T = (unsigned long long)s.T, tau0 = r_next / T;
    const unsigned long long tau_end = std::min<unsigned long long>(tau0 + (unsigned long long)window, s.ticks);
    return Pass{(unsigned)tau0, (unsigned)(r_next % T), (unsigned)tau_end, (unsigned)(tau_end * T)};
  }
  // rstar_read: the lowest rank that must not commit, as read back; overflowed: a walk ran out of stack spill (it cut
  // the pass at its own rank, which may be the first). Returns whether the pass was cut.
  bool advance(const Pass& ps, unsigned rstar_read, bool overflowed, int window_max) {
    const unsigned long long rstar = std::min<unsigned long long>(rstar_read, ps.limit);
    if (!overflowed) FU_CHECK(rstar > r_next, "pass made no progress");
    const bool cut = rstar < (unsigned long long)ps.limit;
    window = cut ? std::max<long long>(kWindowMin, window / 2) : std::min<long long>(window_max, 2 * window);
    r_next = rstar;
    return cut;
  }
};

// ---- the result ----

// the points of one image, in (thread, tick) order, with their thread
struct Chunk {
  std::vector<float> pt;
  std::vector<unsigned char> col;
  std::vector<int> nvis, vis, thread;
};

// task_fused_points_[thread] concatenated over the threads (fusion.cc:322-337): every chunk is sorted by thread
inline void concatenate(const std::vector<Chunk>& chunks, int max_threads, fusion_result* out) {
  std::vector<size_t> at(chunks.size(), 0), vat(chunks.size(), 0);
  for (int t = 0; t < max_threads; ++t) {
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
      const Chunk& c = chunks[ci];
      const size_t b = at[ci];
      size_t e = b, nv = 0;
      while (e < c.thread.size() && c.thread[e] == t) nv += (size_t)c.nvis[e++];
      if (e == b) continue;
      out->xyz_normal.insert(out->xyz_normal.end(), c.pt.begin() + 6 * b, c.pt.begin() + 6 * e);
      out->rgb.insert(out->rgb.end(), c.col.begin() + 3 * b, c.col.begin() + 3 * e);
      out->vis_idx.insert(out->vis_idx.end(), c.vis.begin() + vat[ci], c.vis.begin() + vat[ci] + nv);
      int64_t base = out->vis_ptr.back();
      for (size_t k = b; k < e; ++k) {
        base += c.nvis[k];
        out->vis_ptr.push_back(base);
      }
      at[ci] = e;
      vat[ci] += nv;
    }
  }
}

}  // namespace fusion_plan

#endif  // COLMAP_AMD_FUSION_PLAN_H_
