// The host-only plan of a depth-map fusion run (colmap_amd/csrc/fusion_plan.h) against brute-force code written here:
// input checks, fusion order, descriptors, the pool schedule, the limits of a walk, the pass window, the per-thread
// concatenation. No GPU, nothing linked from the library. Lists and images live in exactly sized heap vectors, so a
// sanitizer build of this program shows that a rejected input is rejected before anything is read through it.
#include "fusion_plan.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>

using namespace fusion_plan;

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

namespace {

float g_map[1];       // the plan looks at whether a map is there, never into it
uint8_t g_bitmap[1];

fusion_options default_options() {  // fusion_options_init lives in the library
  fusion_options o{};
  o.min_num_pixels = 5;
  o.max_num_pixels = 10000;
  o.max_traversal_depth = 100;
  o.check_num_images = 50;
  o.max_reproj_error = 2.0;
  o.max_depth_error = 0.01;
  o.max_normal_error = 10.0;
  for (int c = 0; c < 3; ++c) { o.bbox_min[c] = -3.0f - c; o.bbox_max[c] = 4.0f + c; }
  o.num_threads = -1;
  return o;
}

fusion_image image(int w, int h, int dw, int dh, bool used = true, bool rgb = false) {
  fusion_image im{};
  im.width = w; im.height = h;
  const float K[9] = {100.f, 0.f, 0.5f * w, 0.f, 100.f, 0.5f * h, 0.f, 0.f, 1.f};
  const float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  for (int k = 0; k < 9; ++k) { im.K[k] = K[k]; im.R[k] = R[k]; }
  im.depth_map = g_map; im.normal_map = g_map;
  im.depth_width = dw; im.depth_height = dh;
  if (rgb) { im.rgb = g_bitmap; im.bitmap_width = w; im.bitmap_height = h; }
  im.used = used ? 1 : 0;
  return im;
}

struct Lists {
  std::vector<int32_t> ptr{0}, idx;
  explicit Lists(const std::vector<std::vector<int>>& lists) {
    for (const auto& l : lists) {
      idx.insert(idx.end(), l.begin(), l.end());
      ptr.push_back((int32_t)idx.size());
    }
  }
};

bool throws(const std::function<void()>& f, const char* msg) {
  try {
    f();
  } catch (const Fail& e) {
    return std::string(e.what()) == std::string("Check failed: ") + msg;
  }
  return false;
}

// ---- order ----

// the image after `prev`: its first overlapping image that is used and not fused, else the first such image at all
int next_image(const std::vector<std::vector<int>>& lists, const std::vector<char>& used, const std::vector<char>& fused, int prev) {
  for (int j : lists[prev])
    if (used[j] && !fused[j]) return j;
  for (size_t j = 0; j < used.size(); ++j)
    if (used[j] && !fused[j]) return (int)j;
  return -1;
}

void check_order(const std::vector<std::vector<int>>& lists, const std::vector<char>& used) {
  const int n = (int)lists.size();
  std::vector<fusion_image> images;
  for (int i = 0; i < n; ++i) images.push_back(image(8, 8, 8, 8, used[i] != 0));
  const Lists L(lists);
  const RunPlan plan = make_plan(default_options(), n, images.data(), L.ptr.data(), L.idx.data());
  std::vector<int> order;
  std::vector<char> fused(n, 0);
  for (int i = 0; i >= 0; i = next_image(lists, used, fused, i)) {
    if (used[i]) order.push_back(i);
    fused[i] = 1;
  }
  CHECK(plan.order == order);
  CHECK((int)plan.pos.size() == n);
  std::vector<int> seen(n, 0);
  for (size_t s = 0; s < plan.order.size(); ++s) {
    seen[plan.order[s]] += 1;
    CHECK(plan.pos[plan.order[s]] == (int)s);
  }
  for (int i = 0; i < n; ++i) {
    CHECK(seen[i] == (used[i] ? 1 : 0));
    if (!used[i]) CHECK(plan.pos[i] == -1);
    CHECK(plan.images[i].pos == plan.pos[i]);
  }
}

void test_order() {
  const int n = 6;
  std::vector<std::vector<int>> all(n), chain(n), ring(n), none(n), back(n);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j)
      if (j != i) all[i].push_back(j);
    if (i + 1 < n) chain[i].push_back(i + 1);
    ring[i] = {(i + 2) % n, (i + 1) % n};
    back[i] = {(i + n - 1) % n, i};
  }
  const std::vector<char> every(n, 1), middle = {1, 1, 0, 0, 1, 1}, first = {0, 1, 1, 1, 1, 1}, nobody(n, 0);
  for (const auto& lists : {all, chain, ring, none, back})
    for (const auto& used : {every, middle, first, nobody}) check_order(lists, used);
  check_order(std::vector<std::vector<int>>(1), {1});
  check_order({{0, 0}}, {1});
}

// ---- validation ----

void test_validation() {
  const fusion_options opt = default_options();
  const int n = 3;
  const std::vector<fusion_image> good = {image(8, 8, 8, 8), image(8, 8, 8, 8), image(8, 8, 8, 8)};
  auto plan_of = [&](const std::vector<fusion_image>& im, const std::vector<int32_t>& ptr, const std::vector<int32_t>& idx) {
    return [&, im, ptr, idx] { (void)make_plan(opt, n, im.data(), ptr.data(), idx.data()); };
  };
  (void)make_plan(opt, n, good.data(), Lists({{1}, {2}, {0}}).ptr.data(), Lists({{1}, {2}, {0}}).idx.data());
  CHECK(throws(plan_of(good, {1, 2, 3, 3}, {1, 2}), "overlap_ptr[0] == 0"));
  CHECK(throws(plan_of(good, {0, 2, 1, 3}, {1, 2, 0}), "overlap_ptr does not decrease"));
  CHECK(throws(plan_of(good, {0, 1, 2, 3}, {1, n, 0}), "overlap index"));
  CHECK(throws(plan_of(good, {0, 1, 2, 3}, {-1, 2, 0}), "overlap index"));
  CHECK(throws(plan_of(good, {0, 0, 0, 1}, {1 << 30}), "overlap index"));  // a list the order would not even reach
  {
    std::vector<int32_t> ptr = {0, 1 << 20, 1 << 20, 1 << 20};
    CHECK(throws(plan_of(good, ptr, std::vector<int32_t>(1 << 20, 1)), "overlap list length"));
  }
  std::vector<fusion_image> bad = good;
  bad[1].depth_map = nullptr;
  CHECK(throws(plan_of(bad, {0, 1, 2, 3}, {1, 2, 0}), "depth / normal map"));
  bad = good;
  bad[1].depth_height = 0;
  CHECK(throws(plan_of(bad, {0, 1, 2, 3}, {1, 2, 0}), "depth / normal map"));
  bad = good;
  bad[2].width = 0;
  CHECK(throws(plan_of(bad, {0, 1, 2, 3}, {1, 2, 0}), "image size"));
  bad = good;
  bad[0].depth_width = 1 << 16; bad[0].depth_height = 1 << 15;
  CHECK(throws(plan_of(bad, {0, 1, 2, 3}, {1, 2, 0}), "depth map size"));
  bad = good;
  bad[2] = image(8, 8, 8, 8, true, true);
  bad[2].bitmap_width = 0;
  CHECK(throws(plan_of(bad, {0, 1, 2, 3}, {1, 2, 0}), "bitmap size"));
  bad[2].used = 0;  // an unused image is not looked at
  (void)make_plan(opt, n, bad.data(), Lists({{1}, {2}, {0}}).ptr.data(), Lists({{1}, {2}, {0}}).idx.data());
  // bad lists when no image is used
  for (auto& im : bad) im.used = 0;
  CHECK(throws(plan_of(bad, {0, 1, 2, 3}, {1, n, 0}), "overlap index"));
  CHECK(throws(plan_of(bad, {1, 2, 3, 3}, {1, 2}), "overlap_ptr[0] == 0"));
  CHECK(throws(plan_of(bad, {0, 2, 1, 3}, {1, 2, 0}), "overlap_ptr does not decrease"));
  CHECK(make_plan(opt, n, bad.data(), Lists({{1}, {2}, {0}}).ptr.data(), Lists({{1}, {2}, {0}}).idx.data()).order.empty());
  fusion_options deep = opt;
  deep.max_traversal_depth = 32768;
  CHECK(throws([&] { (void)make_plan(deep, n, good.data(), Lists({{1}, {2}, {0}}).ptr.data(), Lists({{1}, {2}, {0}}).idx.data()); },
               "max_traversal_depth <= 32767"));
  {
    const int many = 65536;
    const std::vector<fusion_image> im(many, image(8, 8, 8, 8, false));
    const std::vector<int32_t> ptr(many + 1, 0), idx;
    CHECK(throws([&] { (void)make_plan(opt, many, im.data(), ptr.data(), idx.data()); }, "at most 65535 images"));
  }
}

// ---- descriptors ----

void test_descriptors() {
  std::vector<fusion_image> im = {image(64, 48, 64, 48, true, true), image(64, 48, 32, 24), image(4000, 3000, 4000, 3000, false, true),
                                  image(100, 60, 50, 20, true, true)};
  const Lists L({{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0}});
  fusion_options opt = default_options();
  const RunPlan plan = make_plan(opt, 4, im.data(), L.ptr.data(), L.idx.data());
  CHECK((plan.order == std::vector<int>{0, 1, 3}));
  CHECK((plan.pos == std::vector<int>{0, 1, -1, 2}));
  CHECK(plan.total_pix == 64 * 48 + 32 * 24 + 50 * 20);
  CHECK(plan.max_seeds == 64 * 48);
  CHECK(plan.max_height == 48);
  CHECK(plan.max_threads == 5);
  CHECK(plan.max_overlap == 3);
  const long long off[4] = {0, 64 * 48, 0, 64 * 48 + 32 * 24};
  const int dw[4] = {64, 32, 0, 50}, dh[4] = {48, 24, 0, 20}, bw[4] = {64, 0, 0, 100}, bh[4] = {48, 0, 0, 60};
  const float sx[4] = {1.0f, 0.5f, 0.0f, 0.5f}, sy[4] = {1.0f, 0.5f, 0.0f, static_cast<float>(20) / 60};
  for (int i = 0; i < 4; ++i) {
    const DevImage& d = plan.images[i];
    CHECK(d.pos == plan.pos[i]);
    CHECK(d.rgb == nullptr);
    CHECK(d.dw == dw[i] && d.dh == dh[i] && d.bw == bw[i] && d.bh == bh[i]);
    CHECK(d.sx == sx[i] && d.sy == sy[i]);
    CHECK(d.pix_off == off[i]);
  }
  for (float v : plan.images[2].P) CHECK(v == 0.0f);  // an unused image contributes nothing
  CHECK(plan.images[1].P[0] == 50.0f && plan.images[1].P[2] == 16.0f && plan.images[1].P[6] == 12.0f);  // K scaled to the depth map
  opt.num_threads = 3;
  CHECK(make_plan(opt, 4, im.data(), L.ptr.data(), L.idx.data()).max_threads == 3);
  opt.num_threads = 100;
  CHECK(make_plan(opt, 4, im.data(), L.ptr.data(), L.idx.data()).max_threads == 5);
}

// ---- schedule ----

void test_schedule() {
  const int shapes[6][2] = {{1, 1}, {7, 9}, {7, 10}, {7, 11}, {24, 160}, {64, 48}};
  for (const auto& wh : shapes)
    for (int num_threads : {-1, 1, 3, 100}) {
      const int W = wh[0], H = wh[1];
      const Schedule s = make_schedule(W, H, num_threads);
      const int ns = (H + 9) / 10, T = num_threads <= 0 ? ns : std::min(num_threads, ns);
      CHECK(s.W == W && s.H == H && s.ns_px == W * H);
      CHECK(s.ns == ns && s.T == T);
      CHECK(s.T == pool_threads(H, num_threads));
      CHECK(s.G == (ns + T - 1) / T);
      CHECK(s.L == 10u * (unsigned)W);
      CHECK(s.ticks == (unsigned long long)s.G * s.L);
      CHECK(s.r_end == s.ticks * (unsigned long long)T);
      // thread t takes the stripes t, t + T, ...; in every tick the next pixel of its stripe, row-major
      std::vector<int> taken(W * H, 0);
      for (unsigned long long tau = 0; tau < s.ticks; ++tau)
        for (int t = 0; t < T; ++t) {
          const long long stripe = (long long)(tau / s.L) * T + t, within = (long long)(tau % s.L);
          const long long row = 10 * stripe + within / W, col = within % W;
          if (stripe >= ns || row >= H) continue;
          taken[row * W + col] += 1;
          CHECK(tau * (unsigned long long)T + (unsigned long long)t < s.r_end);
        }
      for (int v : taken) CHECK(v == 1);
    }
  // the most turns a depth map below 2^31 pixels can have: two groups of stripes, the second all but empty
  CHECK(make_schedule(46341, 46340, 4633).r_end == 2ull * 4633 * 463410);
  CHECK(throws([] { (void)make_schedule(1, 2147483641, 214748364); }, "turns of one image < 2^32"));  // r_end = 0xFFFFFFF0
}

// ---- walk limits ----

void test_limits() {
  const fusion_options opt = default_options();
  const Switches sw;
  const long long big = 1000000;
  WalkLimits w = make_limits(opt, big, 4, 12, 3, sw);
  CHECK(w.rec_cap == 10000 && w.elem_cap == 10000 && w.max_level == 99);
  CHECK(w.min_num_pixels == 5 && w.max_depth_error == 0.01);
  CHECK(w.max_sq_reproj == 4.0f);
  CHECK(std::fabs(w.min_cos_normal - 0.98480775f) < 1e-6f);  // cos(10 degrees)
  for (int c = 0; c < 3; ++c) CHECK(w.bmin[c] == opt.bbox_min[c] && w.bmax[c] == opt.bbox_max[c]);
  CHECK(w.window_first == kWindowFirst && w.window_max == kWindowMax);
  fusion_options o = opt;
  o.max_num_pixels = 2;
  w = make_limits(o, big, 4, 12, 3, sw);
  CHECK(w.rec_cap == 1024 && w.elem_cap == 2);
  o.max_num_pixels = 100000;
  w = make_limits(o, big, 4, 12, 3, sw);
  CHECK(w.rec_cap == 16384 && w.elem_cap == 16384);
  w = make_limits(opt, 10, 4, 12, 3, sw);
  CHECK(w.rec_cap == 10 && w.elem_cap == 10 && w.pool_cap == 10);
  CHECK(make_limits(opt, 0, 4, 12, 3, sw).rec_cap == 1);

  // LDS table tiers around kTableBytes
  auto desc_bytes = [](int n) { return (size_t)n * sizeof(DevImage) + ((size_t)n + 1) * sizeof(int); };
  int fit = 1;
  while (desc_bytes(fit + 1) <= (size_t)kTableBytes) ++fit;
  const int room = (int)(((size_t)kTableBytes - desc_bytes(fit)) / sizeof(int));
  CHECK(make_limits(opt, big, fit, 0, 3, sw).lds_tables == 2);
  CHECK(make_limits(opt, big, fit + 1, 0, 3, sw).lds_tables == 0);
  CHECK(make_limits(opt, big, fit, room, 3, sw).lds_tables == 2);
  CHECK(make_limits(opt, big, fit, room + 1, 3, sw).lds_tables == 1);
  for (int value : {-3, 0, 1, 2, 5}) {  // the switch lowers the tier and never raises it
    Switches s2;
    s2.lds_tables = value;
    const int cap = std::max(0, value);
    CHECK(make_limits(opt, big, fit, room, 3, s2).lds_tables == std::min(2, cap));
    CHECK(make_limits(opt, big, fit, room + 1, 3, s2).lds_tables == std::min(1, cap));
    CHECK(make_limits(opt, big, fit + 1, 0, 3, s2).lds_tables == 0);
  }

  // breadth-first walks
  w = make_limits(opt, big, 8, 56, 7, sw);
  CHECK(w.wide_group == 7 && w.wide_bound == 99);
  CHECK(make_limits(opt, big, 8, 56, 32, sw).wide_group == 32);
  CHECK(make_limits(opt, big, 8, 56, 33, sw).wide_group == 0);
  Switches narrow;
  narrow.wide = 0;
  CHECK(make_limits(opt, big, 8, 56, 7, narrow).wide_group == 0);
  o = opt;
  o.max_traversal_depth = 17;
  w = make_limits(o, big, 8, 56, 7, sw);
  CHECK(w.wide_group == 7 && w.wide_bound == 16);
  o.max_traversal_depth = 16;
  w = make_limits(o, big, 8, 56, 7, sw);
  CHECK(w.wide_group == 0 && w.wide_bound == 15);
  o = opt;
  o.max_num_pixels = 16;
  CHECK(make_limits(o, big, 8, 56, 7, sw).wide_group == 0);
  CHECK(make_limits(opt, 15, 8, 56, 7, sw).wide_group == 0);  // a workspace of 15 pixels: rec_cap 15

  // spill and pool
  w = make_limits(opt, big, 8, 56, 7, sw);
  CHECK(w.spill_bound == 10000ll * 7 + 64);
  CHECK(w.pool_cap == big);
  CHECK(make_limits(opt, 3000000000ll, 8, 56, 7, sw).pool_cap == 0x7FFFFFFFll);
  CHECK(make_limits(opt, 0x7FFFFFFFll, 8, 56, 7, sw).pool_cap == 0x7FFFFFFFll);

  Switches odd;
  odd.window_first = 0; odd.window_max = -5;
  w = make_limits(opt, big, 8, 56, 7, odd);
  CHECK(w.window_first == 1 && w.window_max == 1);
}

// ---- pass window ----

// what the device reports for a pass: (rank where the pass ended, spill overflowed)
using Script = std::function<std::pair<unsigned, bool>(const PassWindow&, const Pass&, int pass)>;

void run_window(const Schedule& s, int window_first, int window_max, const Script& script) {
  PassWindow win(window_first);
  long long window = window_first;
  int pass = 0;
  for (; win.r_next < s.r_end; ++pass) {
    CHECK(pass < 10000000);
    const unsigned long long before = win.r_next;
    const Pass ps = win.pass(s);
    CHECK(ps.tau0 == before / (unsigned long long)s.T && ps.rmod == before % (unsigned long long)s.T);
    CHECK(ps.tau_end > ps.tau0 && ps.tau_end <= s.ticks);
    CHECK(ps.tau_end == std::min<unsigned long long>(ps.tau0 + (unsigned long long)window, s.ticks));
    CHECK(ps.limit == (unsigned long long)ps.tau_end * (unsigned long long)s.T);
    CHECK(ps.limit > before);
    const std::pair<unsigned, bool> r = script(win, ps, pass);
    const bool cut = win.advance(ps, r.first, r.second, window_max);
    CHECK(cut == (r.first < ps.limit));
    window = cut ? std::max<long long>(kWindowMin, window / 2) : std::min<long long>(window_max, 2 * window);
    CHECK(win.window == window);
    CHECK(win.window >= kWindowMin && win.window <= window_max);
    CHECK(win.r_next >= before);
    CHECK(win.r_next == std::min<unsigned long long>(r.first, ps.limit));
  }
  CHECK(win.r_next == s.r_end);
}

void test_window() {
  const Schedule wide = make_schedule(64, 480, 3), tiny = make_schedule(7, 11, -1);
  const Script no_cut = [](const PassWindow&, const Pass&, int) { return std::make_pair(0xFFFFFFFFu, false); };
  const Script half = [](const PassWindow& w, const Pass& ps, int) {  // a cut every pass that has room for one
    return std::make_pair((unsigned)(w.r_next + std::max<unsigned long long>(1, (ps.limit - w.r_next) / 2)), false);
  };
  const Script one = [](const PassWindow& w, const Pass&, int) { return std::make_pair((unsigned)(w.r_next + 1), false); };
  const Script overflow = [](const PassWindow& w, const Pass&, int pass) {  // every third pass: no turn commits
    return pass % 3 == 1 ? std::make_pair((unsigned)w.r_next, true) : std::make_pair(0xFFFFFFFFu, false);
  };
  for (const Schedule& s : {wide, tiny})
    for (const Script& script : {no_cut, half, one, overflow}) {
      run_window(s, kWindowFirst, 1024, script);
      run_window(s, kWindowFirst, kWindowMax, script);
      run_window(s, kWindowMin, kWindowMin, script);
    }
  {  // without a cut the window doubles up to its maximum, with one a pass it halves down to kWindowMin
    PassWindow w(kWindowFirst);
    for (int k = 0; k < 4; ++k) (void)w.advance(w.pass(wide), 0xFFFFFFFFu, false, 1024);
    CHECK(w.window == 1024);
    for (int k = 0; k < 10; ++k) (void)w.advance(w.pass(wide), (unsigned)w.r_next + 1, false, 1024);
    CHECK(w.window == kWindowMin);
  }
  PassWindow stuck(kWindowFirst);
  (void)stuck.advance(stuck.pass(wide), 100u, false, kWindowMax);
  const Pass ps = stuck.pass(wide);
  CHECK(throws([&] { (void)stuck.advance(ps, 100u, false, kWindowMax); }, "pass made no progress"));
  CHECK(stuck.r_next == 100 && stuck.advance(ps, 100u, true, kWindowMax));
}

// ---- concatenation ----

void test_concatenation() {
  std::mt19937 rng(7);
  for (int round = 0; round < 50; ++round) {
    const int threads = 1 + (int)(rng() % 6);
    std::vector<Chunk> chunks(rng() % 5);
    for (Chunk& c : chunks)
      for (int t = 0; t < threads; ++t) {
        if (rng() % 3 == 0) continue;  // this thread fused nothing in this image
        for (int k = (int)(rng() % 4); k > 0; --k) {
          c.thread.push_back(t);
          for (int j = 0; j < 6; ++j) c.pt.push_back((float)(rng() % 1000) * 0.125f);
          for (int j = 0; j < 3; ++j) c.col.push_back((unsigned char)(rng() % 256));
          c.nvis.push_back((int)(rng() % 4));
          for (int j = 0; j < c.nvis.back(); ++j) c.vis.push_back((int)(rng() % 100));
        }
      }
    fusion_result got;
    concatenate(chunks, threads, &got);
    // for each thread, for each chunk, its points in the chunk's order
    fusion_result want;
    for (int t = 0; t < threads; ++t)
      for (const Chunk& c : chunks) {
        size_t v = 0;
        for (size_t k = 0; k < c.thread.size(); v += (size_t)c.nvis[k], ++k) {
          if (c.thread[k] != t) continue;
          want.xyz_normal.insert(want.xyz_normal.end(), c.pt.begin() + 6 * k, c.pt.begin() + 6 * k + 6);
          want.rgb.insert(want.rgb.end(), c.col.begin() + 3 * k, c.col.begin() + 3 * k + 3);
          want.vis_idx.insert(want.vis_idx.end(), c.vis.begin() + v, c.vis.begin() + v + c.nvis[k]);
          want.vis_ptr.push_back((int64_t)want.vis_idx.size());
        }
      }
    CHECK(got.xyz_normal == want.xyz_normal && got.rgb == want.rgb);
    CHECK(got.vis_ptr == want.vis_ptr && got.vis_idx == want.vis_idx);
    CHECK(got.vis_ptr.front() == 0 && got.vis_ptr.size() == got.rgb.size() / 3 + 1);
    CHECK(got.vis_ptr.back() == (int64_t)got.vis_idx.size());
  }
}

}  // namespace

int main() {
  test_order();
  test_validation();
  test_descriptors();
  test_schedule();
  test_limits();
  test_window();
  test_concatenation();
  std::printf("fusion plan checks OK\n");
  return 0;
}
