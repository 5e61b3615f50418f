// The host plan of model alignment (colmap_amd/csrc/align_plan.h) against brute-force code of its own: input validation
// on exactly sized heap arrays (a read through a bad index before its check shows under the sanitizers), the wave-padded
// record layout, Sim3 algebra, ComputeNumTrials, the sample stream, and the search loop driven by a scripted scorer --
// compared, for several batch sizes, with a one-at-a-time loop written here. g++ alone, no HIP.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "align_plan.h"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

namespace {

namespace ap = align_plan;

struct Pair {  // owns exactly sized arrays
  std::unique_ptr<align_camera[]> sc, tc;
  std::unique_ptr<double[]> sp, tp, sxyz, txyz, sxy, txy;
  std::unique_ptr<int32_t[]> sn, tn, image;
  align_reproj_pair p{};
};

Pair make(int num_images, const std::vector<int>& counts, std::mt19937& rng) {
  Pair s;
  const int params[18] = {3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12, 16, 4, 5, 3, 4, 6, 2};
  s.sc.reset(new align_camera[num_images]());
  s.tc.reset(new align_camera[num_images]());
  for (int i = 0; i < num_images; ++i)
    for (align_camera* c : {&s.sc[i], &s.tc[i]}) {
      c->model_id = (int)(rng() % 18);
      c->num_params = params[c->model_id];
      c->width = 100;
      c->height = 50;
    }
  s.sp.reset(new double[7 * num_images]());
  s.tp.reset(new double[7 * num_images]());
  s.sn.reset(new int32_t[num_images]());
  s.tn.reset(new int32_t[num_images]());
  for (int i = 0; i < num_images; ++i) s.sp[7 * i + 3] = s.tp[7 * i + 3] = 1.0;
  int64_t N = 0;
  for (int c : counts) N += c;
  s.image.reset(new int32_t[N]);
  std::vector<int32_t> slots;
  for (size_t i = 0; i < counts.size(); ++i) slots.insert(slots.end(), (size_t)counts[i], (int32_t)i);
  std::shuffle(slots.begin(), slots.end(), rng);
  for (int64_t r = 0; r < N; ++r) s.image[r] = slots[(size_t)r];
  s.sxyz.reset(new double[3 * N]());
  s.txyz.reset(new double[3 * N]());
  s.sxy.reset(new double[2 * N]());
  s.txy.reset(new double[2 * N]());
  s.p.num_images = num_images;
  s.p.num_records = N;
  s.p.src_cameras = s.sc.get();
  s.p.tgt_cameras = s.tc.get();
  s.p.src_poses = s.sp.get();
  s.p.tgt_poses = s.tp.get();
  s.p.src_num_points2D = s.sn.get();
  s.p.tgt_num_points2D = s.tn.get();
  s.p.rec_image = s.image.get();
  s.p.rec_src_xyz = s.sxyz.get();
  s.p.rec_tgt_xyz = s.txyz.get();
  s.p.rec_src_xy = s.sxy.get();
  s.p.rec_tgt_xy = s.txy.get();
  return s;
}

template <typename F>
bool fails(F&& f, const char* needle) {
  try {
    f();
  } catch (const ap::Fail& e) {
    return std::string(e.what()).find(needle) != std::string::npos;
  }
  return false;
}

void test_validation() {
  std::mt19937 rng(1);
  const std::vector<int> counts = {3, 0, 70};
  {
    Pair s = make(3, counts, rng);
    ap::validate(s.p);
  }
  {
    Pair s = make(3, counts, rng);
    s.p.rec_image = nullptr;
    EXPECT(fails([&] { ap::validate(s.p); }, "null"));
  }
  {
    Pair s = make(3, counts, rng);
    s.p.tgt_poses = nullptr;
    EXPECT(fails([&] { ap::validate(s.p); }, "null"));
  }
  {
    Pair s = make(3, counts, rng);
    s.image[5] = 3;
    EXPECT(fails([&] { ap::validate(s.p); }, "out of range"));
    s.image[5] = -1;
    EXPECT(fails([&] { ap::validate(s.p); }, "out of range"));
  }
  {
    Pair s = make(3, counts, rng);
    s.tn[1] = 4;
    EXPECT(fails([&] { ap::validate(s.p); }, "NumPoints2D"));
  }
  {
    Pair s = make(3, counts, rng);
    s.tc[2].model_id = 18;
    EXPECT(fails([&] { ap::validate(s.p); }, "unknown camera model"));
    s.tc[2].model_id = 0;
    s.tc[2].num_params = 4;
    EXPECT(fails([&] { ap::validate(s.p); }, "parameters"));
  }
  {
    Pair s = make(3, counts, rng);
    s.p.num_records = -1;
    EXPECT(fails([&] { ap::validate(s.p); }, "negative"));
  }
  {
    Pair s = make(0, {}, rng);  // empty is fine, with null arrays too
    s.p.src_cameras = s.p.tgt_cameras = nullptr;
    s.p.rec_image = nullptr;
    ap::validate(s.p);
    EXPECT(ap::make_layout(s.p).num_rows == 0);
  }
  EXPECT(fails([&] { ap::validate_positions(nullptr, nullptr, 2); }, "null"));
  EXPECT(fails([&] { ap::validate_positions(nullptr, nullptr, -2); }, "negative"));
  ap::validate_positions(nullptr, nullptr, 0);
  align_options o{8.0, 0.3, 0.1, 0.99, 3.0, 0, 100, 0, 0};
  ap::validate_options(o, true);
  o.max_error = -1.0;
  EXPECT(fails([&] { ap::validate_options(o, true); }, "negative"));
  o.max_error = 0.0;
  ap::validate_options(o, true);
  EXPECT(fails([&] { ap::validate_options(o, false); }, "positive"));
  o.max_error = 1.0;
  o.min_num_trials = 101;
  EXPECT(fails([&] { ap::validate_options(o, false); }, "min_num_trials"));
  o.min_num_trials = 0;
  o.batch_size = ALIGN_MAX_BATCH + 1;
  EXPECT(fails([&] { ap::validate_options(o, false); }, "batch_size"));
  const double nan_sim[8] = {1, 1, 0, 0, 0, 0, 0, std::nan("")};
  EXPECT(fails([&] { ap::check_sim3(nan_sim, "h"); }, "finite"));
}

void test_layout() {
  std::mt19937 rng(2);
  const std::vector<int> counts = {0, 1, 2, 63, 64, 65, 127, 129, 300, 17, 0};
  Pair s = make((int)counts.size(), counts, rng);
  const ap::ReprojLayout L = ap::make_layout(s.p);
  int64_t waves = 0;
  for (int c : counts) waves += (c + 63) / 64;
  EXPECT(L.num_rows == 64 * waves);
  EXPECT((int64_t)L.wave_image.size() == waves && (int64_t)L.wave_count.size() == waves);
  std::vector<int> seen((size_t)s.p.num_records, 0);
  for (size_t i = 0; i < counts.size(); ++i) {
    EXPECT(L.common[i] == (uint32_t)counts[i]);
    EXPECT(L.image_wave_begin[i + 1] - L.image_wave_begin[i] == (counts[i] + 63) / 64);
    int32_t last = -1;
    int total = 0;
    for (int32_t w = L.image_wave_begin[i]; w < L.image_wave_begin[i + 1]; ++w) {
      EXPECT(L.wave_image[(size_t)w] == (int32_t)i);
      EXPECT(L.wave_count[(size_t)w] >= 1 && L.wave_count[(size_t)w] <= 64);
      for (int l = 0; l < 64; ++l) {
        const int32_t o = L.order[(size_t)w * 64 + (size_t)l];
        if (l < L.wave_count[(size_t)w]) {
          EXPECT(o >= 0 && s.image[o] == (int32_t)i);
          EXPECT(o > last);  // stable: the caller's order inside an image
          last = o;
          ++seen[(size_t)o];
          ++total;
        } else {
          EXPECT(o == -1);
        }
      }
      if (w + 1 < L.image_wave_begin[i + 1]) EXPECT(L.wave_count[(size_t)w] == 64);
    }
    EXPECT(total == counts[i]);
  }
  for (int v : seen) EXPECT(v == 1);
  EXPECT(ap::reproj_residual(0, 0) == 1.0 && ap::reproj_residual(3, 4) == 0.0625 && ap::reproj_residual(5, 5) == 0.0);
}

void test_sim3() {
  const double sim[8] = {1.7, 0.9, 0.1, -0.2, 0.3, 0.5, -1.0, 2.0};  // the quaternion is not normalised on purpose
  double inv[8], back[8], M[12], Mi[12];
  ap::sim3_inverse(sim, inv);
  ap::sim3_inverse(inv, back);
  ap::sim3_matrix(sim, M);
  ap::sim3_matrix(inv, Mi);
  const double x[3] = {0.3, -0.7, 1.1};
  double y[3], z[3];
  for (int r = 0; r < 3; ++r) y[r] = M[4 * r] * x[0] + M[4 * r + 1] * x[1] + M[4 * r + 2] * x[2] + M[4 * r + 3];
  for (int r = 0; r < 3; ++r) z[r] = Mi[4 * r] * y[0] + Mi[4 * r + 1] * y[1] + Mi[4 * r + 2] * y[2] + Mi[4 * r + 3];
  for (int r = 0; r < 3; ++r) EXPECT(std::abs(z[r] - x[r]) < 1e-14);
  EXPECT(std::abs(back[0] - sim[0]) < 1e-15);
  for (int k = 5; k < 8; ++k) EXPECT(std::abs(back[k] - sim[k]) < 1e-14);
  // Horn recovers a similarity from exact correspondences, through sim3_from_srt
  std::mt19937 rng(3);
  std::uniform_real_distribution<double> u(-2, 2);
  std::vector<double> a(30), b(30);
  for (int i = 0; i < 10; ++i) {
    for (int c = 0; c < 3; ++c) a[3 * i + c] = u(rng);
    for (int r = 0; r < 3; ++r)
      b[3 * i + r] = M[4 * r] * a[3 * i] + M[4 * r + 1] * a[3 * i + 1] + M[4 * r + 2] * a[3 * i + 2] + M[4 * r + 3];
  }
  size_t idx[10];
  for (size_t i = 0; i < 10; ++i) idx[i] = i;
  double est[8], Me[12];
  EXPECT(ap::estimate_sim3(a.data(), b.data(), idx, 10, est));
  ap::sim3_matrix(est, Me);
  for (int k = 0; k < 12; ++k) EXPECT(std::abs(Me[k] - M[k]) < 1e-12);
  const size_t same[3] = {1, 1, 1};
  EXPECT(!ap::estimate_sim3(a.data(), b.data(), same, 3, est));  // coincident
  const auto c = ap::projection_center(std::vector<double>{0, 0, 0, 1, -1.0, -2.0, -3.0}.data());
  EXPECT(c[0] == 1.0 && c[1] == 2.0 && c[2] == 3.0);
}

void test_num_trials() {
  // the three early returns of optim/ransac.h:179-210
  EXPECT(ap::ComputeNumTrials(50, 100, 1.0, 3.0) == ap::kNoLimit);   // prob_failure <= 0
  EXPECT(ap::ComputeNumTrials(100, 100, 0.99, 3.0) == 1);            // prob_outlier <= 0
  EXPECT(ap::ComputeNumTrials(0, 100, 0.99, 3.0) == ap::kNoLimit);   // prob_outlier == 1
  EXPECT(ap::ComputeNumTrials(2, 100, 0.99, 3.0) == ap::kNoLimit);   // fewer inliers than a sample: a factor is 0
  EXPECT(ap::ComputeNumTrials(50, 100, 0.99, 0.0) == 0);
  // 50 of 100: p = 50/100 * 49/99 * 48/98 = 0.121212..., ceil(log(0.01) / log(1 - p) * 3) = 107
  EXPECT(ap::ComputeNumTrials(50, 100, 0.99, 3.0) == 107);
  // 90 of 100: p = 0.726530..., ceil(3.5527 * 1) = 4
  EXPECT(ap::ComputeNumTrials(90, 100, 0.99, 1.0) == 4);
  align_options o{1.0, 0.3, 0.2, 0.99, 3.0, 0, INT32_MAX, 0, 0};
  // the clamp: 20000 of 100000, p = 0.2 * (19999/99999) * (19998/99998) = 0.00799880..., 3 * 573.4... -> 1721
  EXPECT(ap::clamped_max_num_trials(o) == 1721);
  o.max_num_trials = 100;
  EXPECT(ap::clamped_max_num_trials(o) == 100);
  o.min_inlier_ratio = 0.0;
  EXPECT(ap::clamped_max_num_trials(o) == 100);
}

void test_sample_stream() {
  // first values of the LCG of colmap_amd/estimators.py for seed 0 and n = 20, written out by hand from its definition
  ap::SampleStream s(0);
  uint64_t state = 0x9E3779B97F4A7C15ull * 6364136223846793005ull + 1442695040888963407ull;
  EXPECT(s.state == state);
  for (int rep = 0; rep < 50; ++rep) {
    size_t idx[3];
    s.draw(20, idx);
    size_t want[3];
    for (int k = 0; k < 3;) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      const size_t c = (size_t)((state >> 33) % 20);
      bool dup = false;
      for (int j = 0; j < k; ++j) dup = dup || want[j] == c;
      if (!dup) want[k++] = c;
    }
    for (int k = 0; k < 3; ++k) EXPECT(idx[k] == want[k] && idx[k] < 20);
    EXPECT(idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2]);
  }
}

// A scripted problem: samples are numbers; a model is the sorted index set it was estimated from, kept in a table and
// named by sim[5]; a sample's residual under a model is a fixed pseudo-random function of (model, sample) that favours
// the samples below `good`. Samples whose index sum is divisible by 7 have no model.
struct Scripted {
  size_t n, good;
  double max_residual;
  std::map<double, std::vector<size_t>> models;  // by the name a model carries in sim[5]: a hash of its index set
  std::vector<int> batch_sizes;
  int single_calls = 0;

  size_t num_samples() const { return n; }
  bool estimate(const size_t* idx, size_t count, double sim[8]) {
    std::vector<size_t> key(idx, idx + count);
    std::sort(key.begin(), key.end());
    size_t sum = 0;
    for (size_t v : key) sum += v;
    if (count == 3 && sum % 7 == 0) return false;
    uint64_t name = 1469598103934665603ull;
    for (size_t v : key) name = (name ^ (uint64_t)v) * 1099511628211ull;
    for (int k = 0; k < 8; ++k) sim[k] = 0.0;
    sim[0] = 1.0;
    sim[1] = 1.0;
    sim[5] = (double)(name >> 11);  // exact in a double, the same in whatever order the models are met
    const auto it = models.emplace(sim[5], key).first;
    EXPECT(it->second == key);
    return true;
  }
  double residual(double model, size_t sample) const {
    const std::vector<size_t>& key = models.at(model);
    size_t inside = 0;
    for (size_t v : key) inside += v < good ? 1 : 0;
    uint64_t h = 1469598103934665603ull ^ (uint64_t)sample;
    for (size_t v : key) h = (h ^ (uint64_t)v) * 1099511628211ull;
    const double noise = (double)(h >> 40) / (double)(1ull << 24);  // [0, 1)
    const bool clean = inside == key.size();
    if (clean && sample < good) return 0.5 * max_residual * noise * (key.size() > 3 ? 0.5 : 1.0);
    return max_residual * (0.6 + 3.0 * noise);  // some of these fall below max_residual
  }
  ap::Support support_of(double model, std::vector<uint8_t>* mask) const {
    ap::Support s;
    s.num_inliers = 0;
    s.residual_sum = 0.0;
    if (mask) mask->assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const double r = residual(model, i);
      if (r <= max_residual) {
        ++s.num_inliers;
        s.residual_sum += r;
        if (mask) (*mask)[i] = 1;
      }
    }
    return s;
  }
  void score(const double* sims, int B, ap::Support* supports) {
    batch_sizes.push_back(B);
    for (int h = 0; h < B; ++h) supports[h] = support_of(sims[8 * h + 5], nullptr);
  }
  void inliers(const double sim[8], std::vector<uint8_t>* mask, ap::Support* s) {
    ++single_calls;
    *s = support_of(sim[5], mask);
  }
};

// LORANSAC::Estimate one trial at a time, straight from optim/loransac.h:131-393
ap::Report sequential(Scripted& P, const align_options& opt) {
  ap::Report report;
  const size_t n = P.num_samples();
  if (n < 3) return report;
  const uint64_t max_num_trials = ap::clamped_max_num_trials(opt);
  ap::Support best;
  best.num_inliers = 0;
  bool have = false;
  std::array<double, 8> best_model{};
  ap::SampleStream stream(opt.random_seed);
  uint64_t counter = 0, dyn = max_num_trials;
  while (true) {
    const uint64_t curr = counter++;
    if (curr >= max_num_trials) break;
    size_t idx[3];
    stream.draw(n, idx);
    double sim[8];
    if (!P.estimate(idx, 3, sim)) continue;
    std::vector<uint8_t> mask, mask2;
    ap::Support support;
    P.inliers(sim, &mask, &support);
    if (ap::IsLeftBetter(support, best)) {
      ap::Support local_best = support;
      std::array<double, 8> local_model;
      std::copy(sim, sim + 8, local_model.begin());
      if (support.num_inliers > 3) {
        for (int it = 0; it < 10; ++it) {
          std::vector<size_t> in;
          for (size_t i = 0; i < n; ++i)
            if (mask[i]) in.push_back(i);
          double refit[8];
          bool improved = false;
          if (P.estimate(in.data(), in.size(), refit)) {
            ap::Support s2;
            P.inliers(refit, &mask2, &s2);
            if (ap::IsLeftBetter(s2, local_best)) {
              local_best = s2;
              std::copy(refit, refit + 8, local_model.begin());
              improved = true;
              mask.swap(mask2);
            }
          }
          if (!improved) break;
        }
      }
      if (ap::IsLeftBetter(local_best, best)) {
        best = local_best;
        best_model = local_model;
        have = true;
        dyn = ap::ComputeNumTrials(best.num_inliers, n, opt.confidence, opt.dyn_num_trials_multiplier);
      }
    }
    if (curr >= dyn && curr >= (uint64_t)opt.min_num_trials) break;
  }
  report.num_trials = counter;
  if (!have) return report;
  report.support = best;
  report.model = best_model;
  if (best.num_inliers < 3) return report;
  report.success = true;
  ap::Support s;
  P.inliers(best_model.data(), &report.inlier_mask, &s);
  return report;
}

void expect_same(const ap::Report& a, const ap::Report& b) {
  EXPECT(a.success == b.success);
  EXPECT(a.num_trials == b.num_trials);
  EXPECT(a.support.num_inliers == b.support.num_inliers);
  EXPECT(a.support.residual_sum == b.support.residual_sum);
  EXPECT(a.model == b.model);
  EXPECT(a.inlier_mask == b.inlier_mask);
}

void test_search() {
  int improved_late = 0;
  for (int seed = 0; seed < 40; ++seed) {
    for (int variant = 0; variant < 4; ++variant) {
      align_options opt{1.0, 0.3, 0.05, 0.99, 3.0, 0, INT32_MAX, seed, 0};
      size_t n = 30, good = 18;
      if (variant == 1) opt.min_num_trials = 90;
      if (variant == 2) opt.max_num_trials = 7;
      if (variant == 3) {
        good = 9;  // few inliers: many trials until the dynamic stop
        opt.dyn_num_trials_multiplier = 1.0;
      }
      Scripted ref{n, good, 0.25, {}, {}, 0};
      const ap::Report want = sequential(ref, opt);
      if (variant == 1) EXPECT(want.num_trials > 90);
      if (variant == 2) EXPECT(want.num_trials == 8);
      if (variant == 0 && want.num_trials > 10) ++improved_late;
      for (int B : {1, 2, 7, 64, 1000}) {
        Scripted P{n, good, 0.25, {}, {}, 0};
        opt.batch_size = B;
        const ap::Report got = ap::loransac(P, opt);
        expect_same(got, want);
        for (int b : P.batch_sizes) EXPECT(b >= 1 && b <= B);
        if (B == 1) EXPECT(got.num_launches == got.num_scored);
      }
    }
  }
  EXPECT(improved_late > 0);
  // fewer than three samples: no trial at all
  Scripted P{2, 2, 0.25, {}, {}, 0};
  align_options opt{1.0, 0.3, 0.1, 0.99, 3.0, 0, INT32_MAX, 0, 0};
  const ap::Report r = ap::loransac(P, opt);
  EXPECT(!r.success && r.num_trials == 0 && P.batch_sizes.empty());
}

}  // namespace

int main() {
  test_validation();
  test_layout();
  test_sim3();
  test_num_trials();
  test_sample_stream();
  test_search();
  std::printf("align plan checks OK\n");
  return 0;
}
