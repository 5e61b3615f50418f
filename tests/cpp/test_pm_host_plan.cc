// The host-only plan of PatchMatch (colmap_amd/csrc/pm_host_plan.h) against brute-force code written here: input
// checks, pose tables, shape scalars, source-image span, re-homing order, run compatibility, run shape, sweep schedule
// with its parameter blocks, sub-batch sizes. No GPU, nothing linked from the library. Index arrays and images live in
// exactly sized heap buffers, so a sanitizer build of this program shows that a rejected input is rejected before
// anything is read through it.
#include "pm_host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>

using namespace pm_host;
using colmap_amd::kFpStrip;

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

namespace {

uint8_t g_gray[1];  // the plan looks at whether a map is there, never into it
float g_map[1];

pm_options default_options() {  // pm_options_init lives in the library; depth range and sigma_spatial as a caller sets them
  pm_options o{};
  o.depth_min = 1.0;
  o.depth_max = 5.0;
  o.sigma_spatial = 5.0;
  o.sigma_color = 0.2f;
  o.ncc_sigma = 0.6f;
  o.min_triangulation_angle = 1.0f;
  o.incident_angle_sigma = 0.9f;
  o.geom_consistency_regularizer = 0.3f;
  o.geom_consistency_max_cost = 3.0f;
  o.filter_min_ncc = 0.1f;
  o.filter_min_triangulation_angle = 3.0f;
  o.filter_geom_consistency_max_cost = 1.0f;
  o.window_radius = 5;
  o.window_step = 1;
  o.num_samples = 15;
  o.num_iterations = 5;
  o.filter_min_num_consistent = 2;
  o.geom_consistency = 0;
  o.filter = 1;
  o.gpu_index = -1;
  return o;
}

pm_image image(int w, int h) {
  pm_image im{};
  im.width = w; im.height = h;
  const float K[9] = {4.f, 0.f, 1.f, 0.f, 8.f, 1.f, 0.f, 0.f, 1.f};
  const float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  for (int k = 0; k < 9; ++k) { im.K[k] = K[k]; im.R[k] = R[k]; }
  im.gray = g_gray;
  return im;
}

// A problem whose arrays are heap buffers of exactly the stated sizes.
struct Problem {
  std::unique_ptr<pm_image[]> images;
  std::unique_ptr<int32_t[]> src;
  pm_problem p{};
  Problem(int num_images, int ref, const std::vector<int>& src_idxs) {
    images.reset(new pm_image[num_images]);
    for (int i = 0; i < num_images; ++i) images[i] = image(3, 2);
    src.reset(new int32_t[src_idxs.size()]);
    for (size_t s = 0; s < src_idxs.size(); ++s) src[s] = src_idxs[s];
    p.ref_image_idx = ref;
    p.num_src_images = (int)src_idxs.size();
    p.src_image_idxs = src.get();
    p.num_images = num_images;
    p.images = images.get();
  }
};

// f is rejected, and with exactly this message ("Check failed: <condition> <explanation>")
bool rejects(const std::function<void()>& f, const char* cond, const char* msg) {
  try {
    f();
  } catch (const Fail& e) {
    const std::string want = std::string("Check failed: ") + cond + " " + msg;
    if (want != e.what()) std::fprintf(stderr, "got \"%s\", expected \"%s\"\n", e.what(), want.c_str());
    return want == e.what();
  }
  return false;
}

// ---- validation ----

void test_check_options() {
  CheckOptions(default_options());
  const auto bad = [](const std::function<void(pm_options&)>& change, const char* cond, const char* msg) {
    pm_options o = default_options();
    change(o);
    return rejects([&] { CheckOptions(o); }, cond, msg);
  };
  const auto good = [](const std::function<void(pm_options&)>& change) {
    pm_options o = default_options();
    change(o);
    CheckOptions(o);
  };
  const char* depth_msg = "depth range must be set (PatchMatchController::ProcessProblem, patch_match.cc:425-434)";
  CHECK(bad([](pm_options& o) { o.depth_min = 6.0; }, "o.depth_min <= o.depth_max", "depth_min <= depth_max"));
  CHECK(bad([](pm_options& o) { o.depth_min = -2.0; }, "o.depth_min >= 0.0", "depth_min >= 0"));
  CHECK(bad([](pm_options& o) { o.depth_min = o.depth_max = -1.0; }, "o.depth_min > 0.0 && o.depth_max > 0.0", depth_msg));
  CHECK(bad([](pm_options& o) { o.depth_min = 0.0; }, "o.depth_min > 0.0 && o.depth_max > 0.0", depth_msg));
  good([](pm_options& o) { o.depth_min = o.depth_max = 2.0; });
  CHECK(bad([](pm_options& o) { o.window_radius = 33; }, "o.window_radius <= 32", "window_radius <= kMaxPatchMatchWindowRadius"));
  CHECK(bad([](pm_options& o) { o.window_radius = 21; }, "o.window_radius <= 20",
            "window size not supported (reference instantiates radius 1..20)"));
  good([](pm_options& o) { o.window_radius = 20; o.sigma_spatial = 20.0; });
  good([](pm_options& o) { o.window_radius = 1; });
  CHECK(bad([](pm_options& o) { o.window_radius = 0; }, "o.window_radius > 0", ""));
  CHECK(bad([](pm_options& o) { o.sigma_color = 0.0; }, "o.sigma_color > 0.0", ""));
  CHECK(bad([](pm_options& o) { o.window_step = 0; }, "o.window_step > 0", ""));
  CHECK(bad([](pm_options& o) { o.window_step = 3; }, "o.window_step <= 2", ""));
  good([](pm_options& o) { o.window_step = 2; });
  CHECK(bad([](pm_options& o) { o.num_samples = 0; }, "o.num_samples > 0", ""));
  CHECK(bad([](pm_options& o) { o.ncc_sigma = 0.0; }, "o.ncc_sigma > 0.0", ""));
  CHECK(bad([](pm_options& o) { o.min_triangulation_angle = -0.5; }, "o.min_triangulation_angle >= 0.0", ""));
  CHECK(bad([](pm_options& o) { o.min_triangulation_angle = 180.0; }, "o.min_triangulation_angle < 180.0", ""));
  good([](pm_options& o) { o.min_triangulation_angle = 0.0; });
  CHECK(bad([](pm_options& o) { o.incident_angle_sigma = 0.0; }, "o.incident_angle_sigma > 0.0", ""));
  CHECK(bad([](pm_options& o) { o.num_iterations = 0; }, "o.num_iterations > 0", ""));
  good([](pm_options& o) { o.num_iterations = 1; });
  CHECK(bad([](pm_options& o) { o.geom_consistency_regularizer = -0.1; }, "o.geom_consistency_regularizer >= 0.0", ""));
  CHECK(bad([](pm_options& o) { o.geom_consistency_max_cost = -0.1; }, "o.geom_consistency_max_cost >= 0.0", ""));
  CHECK(bad([](pm_options& o) { o.filter_min_ncc = -1.5; }, "o.filter_min_ncc >= -1.0", ""));
  CHECK(bad([](pm_options& o) { o.filter_min_ncc = 1.5; }, "o.filter_min_ncc <= 1.0", ""));
  good([](pm_options& o) { o.filter_min_ncc = -1.0; });
  good([](pm_options& o) { o.filter_min_ncc = 1.0; });
  CHECK(bad([](pm_options& o) { o.filter_min_triangulation_angle = -1.0; }, "o.filter_min_triangulation_angle >= 0.0", ""));
  CHECK(bad([](pm_options& o) { o.filter_min_triangulation_angle = 181.0; }, "o.filter_min_triangulation_angle <= 180.0", ""));
  good([](pm_options& o) { o.filter_min_triangulation_angle = 180.0; });
  CHECK(bad([](pm_options& o) { o.filter_min_num_consistent = -1; }, "o.filter_min_num_consistent >= 0", ""));
  good([](pm_options& o) { o.filter_min_num_consistent = 0; });
  CHECK(bad([](pm_options& o) { o.filter_geom_consistency_max_cost = -1.0; }, "o.filter_geom_consistency_max_cost >= 0.0", ""));
  CHECK(bad([](pm_options& o) { o.sigma_spatial = -1.0; }, "o.sigma_spatial > 0.0",
            "sigma_spatial must be resolved by the caller (PatchMatchController sets it to window_radius, "
            "patch_match.cc:436-438)"));
}

void test_check_problem() {
  const pm_options opt = default_options();
  pm_options geom = opt;
  geom.geom_consistency = 1;
  { Problem q(4, 1, {0, 2, 3}); CheckProblem(opt, q.p); }
  { Problem q(2, 1, {0}); CheckProblem(opt, q.p); }
  const auto bad = [&](const pm_options& o, Problem& q, const char* cond, const char* msg) {
    return rejects([&] { CheckProblem(o, q.p); }, cond, msg);
  };
  { pm_options o = opt; o.gpu_index = -2; Problem q(3, 1, {0, 2}); CHECK(bad(o, q, "o.gpu_index >= -1", "gpu_index >= -1")); }
  { Problem q(3, 1, {0, 2}); q.p.images = nullptr; CHECK(bad(opt, q, "p.images != nullptr", "problem.images")); }
  { Problem q(3, 1, {}); CHECK(bad(opt, q, "p.num_src_images > 0", "src_image_idxs.size() > 0")); }
  { Problem q(3, 1, {0, 2}); q.p.src_image_idxs = nullptr; CHECK(bad(opt, q, "p.src_image_idxs != nullptr", "src_image_idxs")); }
  const char* dup_cond = "(int)unique.size() == p.num_src_images + 1";
  const char* dup_msg = "duplicate source images or reference image used as source";
  { Problem q(3, 1, {0, 0}); CHECK(bad(opt, q, dup_cond, dup_msg)); }   // duplicate source
  { Problem q(3, 1, {1, 2}); CHECK(bad(opt, q, dup_cond, dup_msg)); }   // the reference as a source
  { Problem q(3, 1, {0, -1}); CHECK(bad(opt, q, "idx >= 0", "image_idx >= 0")); }
  { Problem q(3, -1, {0, 2}); CHECK(bad(opt, q, "idx >= 0", "image_idx >= 0")); }
  { Problem q(3, 1, {0, 3}); CHECK(bad(opt, q, "idx < p.num_images", "image_idx < images.size()")); }
  { Problem q(3, 3, {0, 2}); CHECK(bad(opt, q, "idx < p.num_images", "image_idx < images.size()")); }
  { Problem q(3, 1, {0, 2}); q.images[2].width = 0; CHECK(bad(opt, q, "im.width > 0 && im.height > 0", "bitmap size")); }
  { Problem q(3, 1, {0, 2}); q.images[1].height = 0; CHECK(bad(opt, q, "im.width > 0 && im.height > 0", "bitmap size")); }
  { Problem q(3, 1, {0, 2}); q.images[0].gray = nullptr; CHECK(bad(opt, q, "im.gray != nullptr", "grey bitmap")); }
  const int kidx[5] = {1, 3, 6, 7, 8};
  for (int k : kidx) {
    Problem q(3, 1, {0, 2});
    q.images[2].K[k] += 0.5f;
    const std::string c = "std::abs(im.K[" + std::to_string(k) + "] - " + (k == 8 ? "1.0f" : "0.0f") + ") < 1e-6f";
    const std::string m = "K[" + std::to_string(k) + "]";
    CHECK(bad(opt, q, c.c_str(), m.c_str()));
  }
  { Problem q(3, 1, {0, 2}); q.images[1].R[0] = 0.5f; CheckProblem(opt, q.p); }   // (a pose is not checked)
  { Problem q(4, 1, {0, 2}); q.images[3].gray = nullptr; CheckProblem(opt, q.p); }  // (nor an image the problem does not use)
  // geometric consistency: every used image needs its depth map, the reference its normal map as well
  const auto with_maps = [](Problem& q) {
    for (int i = 0; i < q.p.num_images; ++i) q.images[i].depth_map = g_map;
    q.images[q.p.ref_image_idx].normal_map = g_map;
  };
  { Problem q(3, 1, {0, 2}); with_maps(q); CheckProblem(geom, q.p); }
  { Problem q(3, 1, {0, 2}); with_maps(q); q.images[2].depth_map = nullptr;
    CHECK(bad(geom, q, "im.depth_map != nullptr", "depth map for geom_consistency")); }
  { Problem q(3, 1, {0, 2}); with_maps(q); q.images[1].depth_map = nullptr;
    CHECK(bad(geom, q, "im.depth_map != nullptr", "depth map for geom_consistency")); }
  { Problem q(3, 1, {0, 2}); with_maps(q); q.images[1].normal_map = nullptr;
    CHECK(bad(geom, q, "p.images[p.ref_image_idx].normal_map != nullptr", "reference normal map")); }
  { Problem q(3, 1, {0, 2}); CheckProblem(opt, q.p); }  // (no maps needed without it)
}

// ---- pose tables ----
// Signed permutation rotations, integer translations, power-of-two focal lengths and integer principal points: every
// product and sum below is an integer (or an integer over a power of two) far below 2^24, so float arithmetic is exact
// and the tables are compared with == against integer arithmetic.

struct IPose { long R[9], T[3]; };

IPose rotate_z90(const IPose& a) {  // (x, y, z) -> (y, -x, z): the camera frame after one 90-degree rotation of the image
  IPose r;
  for (int j = 0; j < 3; ++j) { r.R[j] = a.R[3 + j]; r.R[3 + j] = -a.R[j]; r.R[6 + j] = a.R[6 + j]; }
  r.T[0] = a.T[1]; r.T[1] = -a.T[0]; r.T[2] = a.T[2];
  return r;
}

void set_pose(pm_image& im, const IPose& p, long fx, long cx, long fy, long cy) {
  for (int k = 0; k < 9; ++k) im.R[k] = (float)p.R[k];
  for (int k = 0; k < 3; ++k) im.T[k] = (float)p.T[k];
  const float K[9] = {(float)fx, 0.f, (float)cx, 0.f, (float)fy, (float)cy, 0.f, 0.f, 1.f};
  for (int k = 0; k < 9; ++k) im.K[k] = K[k];
}

void test_pose_tables() {
  const int W = 3, H = 2;
  const IPose ref = {{0, -1, 0, 0, 0, 1, -1, 0, 0}, {2, -3, 1}};
  const IPose src[2] = {{{0, 0, 1, -1, 0, 0, 0, -1, 0}, {-1, 2, 4}}, {{-1, 0, 0, 0, 0, 1, 0, 1, 0}, {3, 0, -2}}};
  const long sK[2][4] = {{4, 1, 8, 2}, {16, 3, 2, 1}};  // fx, cx, fy, cy
  Problem q(3, 0, {1, 2});
  set_pose(q.images[0], ref, 4, 1, 8, 1);
  for (int s = 0; s < 2; ++s) set_pose(q.images[1 + s], src[s], sK[s][0], sK[s][1], sK[s][2], sK[s][3]);
  const std::vector<int> idxs = {1, 2};
  const PoseTables t = BuildPoseTables(q.p, W, H, idxs);
  CHECK(t.poses.size() == (size_t)4 * 2 * 43);

  IPose rr = ref;
  for (int rot = 0; rot < 4; ++rot, rr = rotate_z90(rr)) {
    for (int s = 0; s < 2; ++s) {
      const float* p = t.poses.data() + ((size_t)rot * 2 + s) * 43;
      for (int k = 0; k < 4; ++k) CHECK(p[k] == (float)sK[s][k]);
      // relative pose of the source to the rotated reference: R = Rs Rr^T, T = Ts - R Tr
      long R[9], T[3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          R[3 * i + j] = 0;
          for (int k = 0; k < 3; ++k) R[3 * i + j] += src[s].R[3 * i + k] * rr.R[3 * j + k];
        }
      for (int i = 0; i < 3; ++i) {
        T[i] = src[s].T[i];
        for (int k = 0; k < 3; ++k) T[i] -= R[3 * i + k] * rr.T[k];
      }
      for (int k = 0; k < 9; ++k) CHECK(p[4 + k] == (float)R[k]);
      for (int k = 0; k < 3; ++k) CHECK(p[13 + k] == (float)T[k]);
      // C = -R^T T
      for (int i = 0; i < 3; ++i) {
        long c = 0;
        for (int k = 0; k < 3; ++k) c -= R[3 * k + i] * T[k];
        CHECK(p[16 + i] == (float)c);
      }
      // P = K [R | T]
      const long K[9] = {sK[s][0], 0, sK[s][1], 0, sK[s][2], sK[s][3], 0, 0, 1};
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
          long v = 0;
          for (int k = 0; k < 3; ++k) v += K[3 * i + k] * (j < 3 ? R[3 * k + j] : T[k]);
          CHECK(p[19 + 4 * i + j] == (float)v);
        }
      // P [invP; 0 0 0 1] = [I | 0]
      const float* P = p + 19;
      const float* iP = p + 31;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
          float v = j == 3 ? P[4 * i + 3] : 0.0f;
          for (int k = 0; k < 3; ++k) v += P[4 * i + k] * iP[4 * k + j];
          CHECK(v == (i == j ? 1.0f : 0.0f));
        }
    }
  }
  // four applications of the rotation return the first table: a problem whose reference is rotated once has the
  // tables of this one, one direction on -- and in its last direction, the fourth rotation, this one's first
  {
    Problem q1(3, 0, {1, 2});
    set_pose(q1.images[0], rotate_z90(ref), 4, 1, 8, 1);
    for (int s = 0; s < 2; ++s) set_pose(q1.images[1 + s], src[s], sK[s][0], sK[s][1], sK[s][2], sK[s][3]);
    const PoseTables t1 = BuildPoseTables(q1.p, W, H, idxs);
    const size_t n = (size_t)2 * 43;
    for (int rot = 0; rot < 4; ++rot)
      for (size_t k = 0; k < n; ++k) CHECK(t1.poses[rot * n + k] == t.poses[((rot + 1) % 4) * n + k]);
  }
  // ref_K[rot] maps the rotated pixel of (x, y) to the ray ref_K[0] maps (x, y) to, seen from the rotated camera. One
  // rotation takes pixel (x, y) of a w x h image to (y, w - 1 - x) of an h x w image and a ray (a, b) to (b, -a).
  const float fx = 4.f, cx = 1.f, fy = 8.f, cy = 1.f;
  for (int k = 0; k < 4; ++k) CHECK(t.ref_K[0][k] == (k == 0 ? fx : k == 1 ? cx : k == 2 ? fy : cy));
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int px = x, py = y, w = W, h = H;
      float a = (x - cx) / fx, b = (y - cy) / fy;
      for (int rot = 0; rot < 4; ++rot) {
        const float* K = t.ref_K[rot];
        const float* iK = t.ref_inv_K[rot];
        CHECK((px - K[1]) / K[0] == a && (py - K[3]) / K[2] == b);
        CHECK(px * iK[0] + iK[1] == a && py * iK[2] + iK[3] == b);
        const int nx = py, ny = w - 1 - px;
        px = nx; py = ny;
        std::swap(w, h);
        const float na = b, nb = -a;
        a = na; b = nb;
      }
      CHECK(px == x && py == y);  // (the brute-force rotation itself closes after four steps)
    }
}

// ---- shape scalars ----

void test_shape_scalars() {
  pm_options o = default_options();
  PmParams b = ShapeParams(o, 70, 50, 3, 80, 60);
  CHECK(b.W == 70 && b.H == 50 && b.S == 3 && b.src_w == 80 && b.src_h == 60);
  CHECK(b.radius == 5 && b.step == 1 && b.ntap1d == 11 && b.ntaps == 121 && b.num_samples == 15);
  CHECK(b.rec_stride == 13 && b.sel_out_off == 7 && b.sel_in_off == 10);
  CHECK(b.fp_xmax == 80.f + 16.f && b.fp_ymax == 60.f + 4.f && b.fp_rows1 == 68 - 1);  // 60 + 4 + 1 rows, whole fours
  CHECK(b.C == 0 && b.help == 0 && b.rec == nullptr && b.poses == nullptr && b.prof == nullptr);
  CHECK(b.filter_min_num_consistent == 2 && b.filter_min_ncc == 0.1f && b.geom_reg == 0.3f);
  o.window_step = 2;  // taps at -5, -3, .., 5
  b = ShapeParams(o, 70, 50, 3, 80, 60);
  CHECK(b.ntap1d == 6 && b.ntaps == 36);
  o.window_radius = 20;
  CHECK(ShapeParams(o, 70, 50, 3, 80, 60).ntap1d == 21);
  CHECK(SweepThreads(0) == 128 && SweepThreads(-3) == 128 && SweepThreads(1) == 64 && SweepThreads(64) == 64);
  CHECK(SweepThreads(65) == 128 && SweepThreads(256) == 256 && SweepThreads(257) == 256 && SweepThreads(1000) == 256);
}

// ---- span ----

void check_span(const std::vector<uint64_t>& addrs, size_t fp_count, uint64_t limit, bool fits) {
  const FpSpan span = PlanFpSpan(addrs.data(), (int)addrs.size(), fp_count, limit);
  uint64_t lo = addrs[0];
  for (uint64_t a : addrs)
    if (a < lo) lo = a;
  CHECK(span.base == lo);
  CHECK(span.offs.size() == addrs.size());
  for (size_t s = 0; s < addrs.size(); ++s) CHECK(span.offs[s] == (addrs[s] - lo) / kFpStrip);
  CHECK(span.fits == fits);
}

void test_span() {
  const size_t fp_count = colmap_amd::pm_fp_entries(64, 48);
  const uint64_t bytes = fp_count * 4, base = 0x7f0000000000ull;
  CHECK(bytes % 256 == 0);
  CHECK(FpSpanLimit(0, bytes) == (1ull << 32));
  CHECK(FpSpanLimit(3, bytes) == 3 * bytes + 4097);
  const uint64_t limit = 1ull << 32;
  // the furthest image must END before limit - 4096
  const uint64_t edge = limit - 4096 - bytes;  // the offset at which it ends exactly there
  check_span({base + 512, base, base + edge - 256}, fp_count, limit, true);
  check_span({base + 512, base, base + edge}, fp_count, limit, false);
  check_span({base + 512, base, base + edge + 256}, fp_count, limit, false);
  check_span({base + edge - 256, base + 512, base}, fp_count, limit, true);   // (the base may come last)
  check_span({base + edge + 256, base + 512, base}, fp_count, limit, false);
  // the test mode's limit: `slots` images side by side fit, one more slot does not
  const uint64_t small = FpSpanLimit(3, bytes);
  check_span({base, base + bytes, base + 2 * bytes}, fp_count, small, true);
  check_span({base, base + bytes, base + 3 * bytes}, fp_count, small, false);
  // alignment: the resource's base and every offset in whole 256 bytes
  check_span({base + 128, base + 128 + 256}, fp_count, limit, false);
  check_span({base, base + 128}, fp_count, limit, false);
  check_span({base, base + 256}, fp_count, limit, true);
  // S = 1
  check_span({base + 4096}, fp_count, limit, true);
  check_span({base + 4096}, fp_count, bytes + 4096, false);
  check_span({base + 4096}, fp_count, bytes + 4097, true);
  check_span({base + 64}, fp_count, limit, false);
}

// ---- re-homing order ----

void test_rehome_order() {
  static const char mem[5] = {};
  const char *a = mem + 1, *b = mem + 2, *c = mem + 3, *d = mem + 4;
  typedef std::vector<const char*> V;
  // votes 3 / 2 / 1 in every address order, then the newest slab
  CHECK(RehomeCandidates({a, b, c, b, a, a}, d) == (V{a, b, c, d}));
  CHECK(RehomeCandidates({c, b, a, b, c, c}, d) == (V{c, b, a, d}));
  CHECK(RehomeCandidates({b, b, c, a, b, c}, d) == (V{b, c, a, d}));
  CHECK(RehomeCandidates({a, b, c, b, a, a}, nullptr) == (V{a, b, c}));   // no slab with a free slot
  CHECK(RehomeCandidates({a, b, c, b, a, a}, c) == (V{a, b, c}));         // the newest already has a vote
  CHECK(RehomeCandidates({a, b, c, b, a, a}, a) == (V{a, b, c}));
  CHECK(RehomeCandidates({a, nullptr, b, nullptr, b}, d) == (V{b, a, d}));  // images outside the pool do not vote
  CHECK(RehomeCandidates({nullptr, nullptr, nullptr}, d) == (V{d}));       // no slab known
  CHECK(RehomeCandidates({nullptr, nullptr}, nullptr).empty());
  CHECK(RehomeCandidates({a}, a) == (V{a}));
}

// ---- compatibility ----

void test_compatibility() {
  const RunKey k0 = {0, 64, 48, 3, 64, 48, 5, 1, 15, 5, 0, 1, 0, false, false};
  CHECK(CompareRunKeys(k0, k0) == kRunMatch);
  int RunKey::*const sizes[] = {&RunKey::W, &RunKey::H, &RunKey::S, &RunKey::src_w, &RunKey::src_h};
  int RunKey::*const options[] = {&RunKey::window_radius, &RunKey::window_step, &RunKey::num_samples,
                                  &RunKey::num_iterations, &RunKey::geom_consistency, &RunKey::filter,
                                  &RunKey::max_sweeps};
  const auto differ = [&](const std::function<void(RunKey&)>& change, RunMismatch why) {
    RunKey k = k0;
    change(k);
    return CompareRunKeys(k0, k) == why && CompareRunKeys(k, k0) == why;
  };
  CHECK(differ([](RunKey& k) { k.device += 1; }, kRunDevice));
  for (auto f : sizes) CHECK(differ([f](RunKey& k) { k.*f += 1; }, kRunSizes));
  for (auto f : options) CHECK(differ([f](RunKey& k) { k.*f += 1; }, kRunOptions));
  CHECK(differ([](RunKey& k) { k.prof = true; }, kRunDebug));
  CHECK(differ([](RunKey& k) { k.trace = true; }, kRunDebug));
  // a profiled or traced problem shares no launch on its own accord, not even with its like
  RunKey p = k0;
  p.prof = true;
  CHECK(CompareRunKeys(p, p) == kRunDebug);
  p = k0;
  p.trace = true;
  CHECK(CompareRunKeys(p, p) == kRunDebug);
  // the key of a handle
  pm_options o = default_options();
  o.max_sweeps = 3;
  PmParams base = ShapeParams(o, 70, 50, 3, 80, 60);
  unsigned long long word;
  RunKey k = MakeRunKey(2, base, o);
  const RunKey want = {2, 70, 50, 3, 80, 60, 5, 1, 15, 5, 0, 1, 3, false, false};
  CHECK(CompareRunKeys(k, want) == kRunMatch && !k.prof && !k.trace);
  base.prof = &word;
  k = MakeRunKey(2, base, o);
  CHECK(k.prof && !k.trace);
  base.prof = nullptr;
  base.trace = &word;
  k = MakeRunKey(2, base, o);
  CHECK(!k.prof && k.trace);
}

// ---- run shape ----
// The rules, for ncu compute units, alive = max(n, live handles), m = min(W, H), w2 = alive * ((m + 1) / 2):
//   automatic  <=>  ntaps == 121, no handle requested its columns, COLS unset
//   C = the smallest of the handles' columns; if automatic, also of (m >= 512 and 4 w2 < 3 * 16 ncu ? 1 : 2)
//   help = 2   <=>  automatic, that choice was 1, C == 1 and 20 w2 <= 120 ncu
//   HELP = 1: help = 1; HELP = 2 and ntaps == 121: C = 1, help = 2.
// With ncu = 256: 4 w2 < 12288 and 20 w2 <= 30720.

struct ShapeCase {
  std::vector<HandleColumns> cols;
  int ntaps, W, H, live, cols_switch, help_switch, C, help;
};

void test_run_shape() {
  const int ncu = 256;
  const std::vector<ShapeCase> cases = {
      // one 2560 x 1920 problem: w2 = 960; 3840 < 12288: C = 1; 19200 <= 30720: helper
      {{{2, false}}, 121, 2560, 1920, 1, 0, 0, 1, 2},
      {{{2, false}}, 121, 1920, 2560, 1, 0, 0, 1, 2},
      // two alive: w2 = 1920; 7680 < 12288: C = 1; 38400 > 30720: no helper
      {{{2, false}}, 121, 2560, 1920, 2, 0, 0, 1, 1},
      // the helper rule's edge, m = 1024 (512 waves each): 3 alive, 20 * 1536 = 30720; 4 alive, 20 * 2048 = 40960
      {{{2, false}}, 121, 1024, 1024, 3, 0, 0, 1, 2},
      {{{2, false}}, 121, 1024, 1024, 4, 0, 0, 1, 1},
      // the 3/4 rule's edge: 5 alive, 4 * 2560 = 10240 < 12288; 6 alive, 4 * 3072 = 12288 is not
      {{{2, false}}, 121, 1024, 1024, 5, 0, 0, 1, 1},
      {{{2, false}}, 121, 1024, 1024, 6, 0, 0, 2, 1},
      // the problems of the run count even where fewer handles are reported alive
      {std::vector<HandleColumns>(6, {2, false}), 121, 1024, 1024, 1, 0, 0, 2, 1},
      {std::vector<HandleColumns>(5, {2, false}), 121, 1024, 1024, 1, 0, 0, 1, 1},
      // small images keep two columns: m = 511 / 512 (w2 = 256: C = 1, 5120 <= 30720: helper)
      {{{2, false}}, 121, 511, 2000, 1, 0, 0, 2, 1},
      {{{2, false}}, 121, 2000, 511, 1, 0, 0, 2, 1},
      {{{2, false}}, 121, 512, 2000, 1, 0, 0, 1, 2},
      // a handle that already has one column (many sources) where the rule says two: no helper
      {{{1, false}}, 121, 64, 48, 1, 0, 0, 1, 1},
      // an explicit columns_per_group on one handle of the batch: nothing automatic, the minimum wins
      {{{2, false}, {3, true}}, 121, 2560, 1920, 2, 0, 0, 2, 1},
      {{{2, false}, {1, true}}, 121, 2560, 1920, 2, 0, 0, 1, 1},
      {{{4, true}}, 121, 2560, 1920, 1, 0, 0, 4, 1},
      // another window: nothing automatic
      {{{4, false}}, 49, 2560, 1920, 1, 0, 0, 4, 1},
      {{{4, false}, {3, false}}, 441, 2560, 1920, 2, 0, 0, 3, 1},
      // COLS set (the handles' values come re-picked): nothing automatic
      {{{3, false}}, 121, 2560, 1920, 1, 3, 0, 3, 1},
      {{{1, false}}, 121, 2560, 1920, 1, 1, 0, 1, 1},
      // HELP = 1: never
      {{{2, false}}, 121, 2560, 1920, 1, 0, 1, 1, 1},
      // HELP = 2: always at the 11 x 11 window, whatever the size and the handles' columns; nothing at another window
      {{{2, false}}, 121, 64, 48, 1, 0, 2, 1, 2},
      {{{4, true}, {2, false}}, 121, 64, 48, 9, 0, 2, 1, 2},
      {{{3, false}}, 121, 64, 48, 1, 3, 2, 1, 2},
      {{{4, false}}, 49, 64, 48, 1, 0, 2, 4, 1},
      {{{4, false}}, 36, 2560, 1920, 1, 0, 2, 4, 1},
  };
  for (const ShapeCase& c : cases) {
    const RunShape s = PlanRunShape(c.cols.data(), (int)c.cols.size(), c.ntaps, c.W, c.H, c.live, ncu, c.cols_switch,
                                    c.help_switch);
    if (s.C != c.C || s.help != c.help)
      std::fprintf(stderr, "case %d: got C = %d, help = %d\n", (int)(&c - cases.data()), s.C, s.help);
    CHECK(s.C == c.C && s.help == c.help);
  }
  // another device: 64 CUs, 4 w2 < 3072 and 20 w2 <= 7680; one 1024 x 1024 problem has w2 = 512: C = 1, no helper
  const HandleColumns one = {2, false};
  RunShape s = PlanRunShape(&one, 1, 121, 1024, 1024, 1, 64, 0, 0);
  CHECK(s.C == 1 && s.help == 1);
  s = PlanRunShape(&one, 1, 121, 1024, 1024, 2, 64, 0, 0);  // 4 * 1024 = 4096: two columns
  CHECK(s.C == 2 && s.help == 1);
}

// ---- schedule ----

void test_schedule() {
  const int S = 3;
  const int iters[] = {1, 5};
  for (int num_iterations : iters) {
    const int total = 4 * num_iterations;
    const int max_sweeps[] = {-1, 0, 3, total + 7};
    for (int ms : max_sweeps) {
      for (int flags = 0; flags < 4; ++flags) {
        const bool filter = flags & 1, geom = flags & 2;
        const SweepSchedule sch = PlanSweeps(num_iterations, ms, filter, geom, 4 + S, 4 + 2 * S);
        const int limit = ms < 0 ? 0 : ms == 0 ? total : ms < total ? ms : total;
        CHECK(sch.total == total && (int)sch.sweeps.size() == limit);
        for (int k = 0; k < limit; ++k) {
          const Sweep& s = sch.sweeps[k];
          CHECK(s.rot == k % 4);
          const float pert = 1.0f / std::pow(2.0f, (float)(k / 4) + (float)(k % 4) / 4.0f);
          CHECK(s.perturbation == pert);
          CHECK(s.perturbation_pi == (float)(pert * M_PI));
          CHECK(s.prev_sel_prob_weight == (float)k / (float)total);
          CHECK(s.sel_out_off == (k % 2 == 0 ? 4 + S : 4 + 2 * S));
          CHECK(s.sel_in_off == (k % 2 == 0 ? 4 + 2 * S : 4 + S));
          CHECK(s.filter_photo == (filter && k == total - 1));
          CHECK(s.filter_geom == (filter && geom && k == total - 1));
        }
        // the half the last sweep wrote; without a sweep the initial sel_in_off
        CHECK(sch.final_sel_off == (limit == 0 ? 4 + 2 * S : sch.sweeps[limit - 1].sel_out_off));
      }
    }
  }
  // the first perturbations by hand: 1, 2^-1/4 ..; the second iteration starts at 1/2
  const SweepSchedule sch = PlanSweeps(5, 0, true, false, 7, 10);
  CHECK(sch.sweeps[0].perturbation == 1.0f && sch.sweeps[4].perturbation == 0.5f && sch.sweeps[16].perturbation == 0.0625f);
  CHECK(sch.sweeps[0].prev_sel_prob_weight == 0.0f && sch.sweeps[10].prev_sel_prob_weight == 0.5f);
  CHECK(sch.sweeps[19].filter_photo && !sch.sweeps[19].filter_geom && !sch.sweeps[18].filter_photo);
  CHECK(sch.final_sel_off == 10);  // sweep 19 is odd: it wrote the half sweep 0 read
}

void test_param_blocks() {
  const int S = 3;
  pm_options o = default_options();
  o.num_iterations = 2;
  static float rec[8], poses[8][4 * 3 * 43];
  static uint32_t fp[8];
  const int batch[] = {1, 3, 8};
  for (int n : batch) {
    for (int xcd_switch = 0; xcd_switch < 3; ++xcd_switch) {
      for (int fp_resource = 0; fp_resource < 2; ++fp_resource) {
        std::vector<PmParams> bases(n);
        std::vector<PoseTables> tables(n);
        std::vector<RunProblem> probs(n);
        for (int b = 0; b < n; ++b) {
          bases[b] = ShapeParams(o, 70, 50, S, 80, 60);
          bases[b].C = 2 + b;  // (what the handle chose: the run's shape overrides it)
          bases[b].rec = rec + b;
          bases[b].fp_base = fp + b;
          for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k) {
              tables[b].ref_K[r][k] = (float)(100 * b + 10 * r + k);
              tables[b].ref_inv_K[r][k] = -(float)(100 * b + 10 * r + k);
            }
          probs[b] = {&bases[b], &tables[b], poses[b]};
        }
        const SweepSchedule sch = PlanSweeps(o.num_iterations, 7, true, false, bases[0].sel_out_off, bases[0].sel_in_off);
        const RunShape shape = {1, 2};
        const std::vector<PmParams> blocks = FillParamBlocks(sch, probs.data(), n, shape, xcd_switch, fp_resource != 0);
        CHECK(blocks.size() == (size_t)(7 + 1) * n);
        const int xcd_map = xcd_switch == 2 ? 2 : (xcd_switch == 1 && n == 8) ? 1 : 0;
        for (int k = -1; k < 7; ++k)
          for (int b = 0; b < n; ++b) {
            const PmParams& p = blocks[(size_t)(k + 1) * n + b];
            const int rot = k < 0 ? 0 : k % 4;
            CHECK(p.rec == rec + b && p.W == 70 && p.S == S && p.ntaps == 121);
            CHECK(p.rot == rot && p.poses == poses[b] + (size_t)rot * S * 43);
            for (int j = 0; j < 4; ++j)
              CHECK(p.refK[j] == tables[b].ref_K[rot][j] && p.refInvK[j] == tables[b].ref_inv_K[rot][j]);
            CHECK(p.C == 1 && p.help == 2 && p.ablate == 0);
            CHECK(p.fp_base == (fp_resource ? fp + b : nullptr));
            if (k < 0) {  // the initial cost
              CHECK(p.perturbation == 0.0f && p.prev_sel_prob_weight == 0.0f && p.xcd_map == 0);
              CHECK(p.sel_out_off == 4 + S && p.sel_in_off == 4 + 2 * S);
            } else {
              const Sweep& s = sch.sweeps[k];
              CHECK(p.perturbation == s.perturbation && p.perturbation_pi == s.perturbation_pi);
              CHECK(p.prev_sel_prob_weight == s.prev_sel_prob_weight && p.xcd_map == xcd_map);
              CHECK(p.sel_out_off == s.sel_out_off && p.sel_in_off == s.sel_in_off);
            }
          }
      }
    }
  }
}

// ---- sub-batches ----

void test_sub_batches() {
  for (int n = 1; n <= 40; ++n) {
    CHECK(FirstSubBatch(n, 0) == n);
    const int first = FirstSubBatch(n, 1), second = n - first;
    CHECK(first + second == n && first >= 1 && second >= 0);
    if (n < 16) CHECK(second == 0);
    if (second > 0) CHECK(n >= 16 && first >= 8 && second >= 8 && first % 8 == 0);
    if (n >= 16) CHECK(second > 0);
  }
  CHECK(FirstSubBatch(16, 1) == 8 && FirstSubBatch(17, 1) == 8 && FirstSubBatch(23, 1) == 8 && FirstSubBatch(24, 1) == 16);
  CHECK(FirstSubBatch(32, 1) == 16 && FirstSubBatch(33, 1) == 16 && FirstSubBatch(40, 1) == 24);
}

}  // namespace

int main() {
  test_check_options();
  test_check_problem();
  test_pose_tables();
  test_shape_scalars();
  test_span();
  test_rehome_order();
  test_compatibility();
  test_run_shape();
  test_schedule();
  test_param_blocks();
  test_sub_batches();
  std::printf("pm host plan checks OK\n");
  return 0;
}
