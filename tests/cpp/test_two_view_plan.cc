// The host-only plan of two-view geometry estimation (colmap_amd/csrc/two_view_plan.h) with a scripted backend: the
// LORANSAC walk against hand-written traces, the trial budget, the router on every branch, the option checks, the
// layout, the sample draw and the local estimators. `test_two_view_plan svd FILE` prints the Jacobi SVD of the m x 9
// matrix in FILE for tests/test_two_view_plan.py, which compares it with numpy.linalg.svd. No HIP, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>

#include "two_view_plan.h"

namespace tp = two_view_plan;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

template <typename F>
static bool fails_with(F&& f, const char* word) {
  try {
    f();
  } catch (const tp::Fail& e) {
    return std::strstr(e.what(), word) != nullptr;
  }
  return false;
}

// ---------------------------------------------------------------------------------------------------------------------
// the scripted backend: a sample model is tagged (set, trial, j); what a set asks to be scored after a tagged model,
// until its next tagged model, are that model's refits 0, 1, 2, ...
// ---------------------------------------------------------------------------------------------------------------------

constexpr double kTag = 12345.5;
using Sup = std::pair<uint64_t, double>;  // inliers, residual sum

struct Script : tp::Backend {
  std::vector<int64_t> counts;
  std::function<std::vector<Sup>(int set, int64_t trial)> sample;               // supports of a trial's models
  std::function<Sup(int set, int64_t trial, int j, int refit)> refit;           // support of a refit
  struct Cursor { int64_t trial = -1; int j = 0, refit = 0; };
  std::map<int, Cursor> cursor;
  int rounds = 0, scores = 0;
  std::vector<std::string> log;  // what was asked, in order

  void upload(const std::vector<int64_t>& offsets, const std::vector<double>&, const std::vector<uint64_t>&) override {
    counts.clear();
    for (size_t s = 0; s + 1 < offsets.size(); ++s) counts.push_back(offsets[s + 1] - offsets[s]);
  }
  void round(int, double, int32_t, const std::vector<tp::Item>& items, tp::RoundResult* out) override {
    ++rounds;
    out->num_models.clear();
    out->models.clear();
    out->supports.clear();
    for (const tp::Item& it : items)
      for (int64_t t = it.first_trial; t < it.first_trial + it.num_trials; ++t) {
        const std::vector<Sup> s = sample(it.set, t);
        out->num_models.push_back((int32_t)s.size());
        for (int j = 0; j < 3; ++j) {
          tp::Support sup;
          if (j < (int)s.size()) {
            sup.num_inliers = s[(size_t)j].first;
            sup.residual_sum = s[(size_t)j].second;
          }
          out->supports.push_back(sup);
          const double m[9] = {(double)it.set, (double)t, (double)j, kTag, 0, 0, 0, 0, 0};
          out->models.insert(out->models.end(), m, m + 9);
        }
      }
  }
  void score(int, double, const std::vector<tp::ScoreJob>& jobs, std::vector<tp::Support>* supports,
             std::vector<std::vector<uint8_t>>* masks) override {
    ++scores;
    supports->assign(jobs.size(), tp::Support());
    if (masks) masks->assign(jobs.size(), {});
    for (size_t k = 0; k < jobs.size(); ++k) {
      const tp::ScoreJob& job = jobs[k];
      Cursor& c = cursor[job.set];
      Sup s;
      if (job.model[3] == kTag) {
        c.trial = (int64_t)job.model[1];
        c.j = (int)job.model[2];
        c.refit = 0;
        s = sample(job.set, c.trial)[(size_t)c.j];
        log.push_back("s" + std::to_string(job.set) + " t" + std::to_string(c.trial) + " j" + std::to_string(c.j));
      } else {
        s = refit(job.set, c.trial, c.j, c.refit);
        log.push_back("s" + std::to_string(job.set) + " t" + std::to_string(c.trial) + " j" + std::to_string(c.j) + " r" +
                      std::to_string(c.refit));
        ++c.refit;
      }
      (*supports)[k].num_inliers = s.first;
      (*supports)[k].residual_sum = s.second;
      if (masks) {
        (*masks)[k].assign((size_t)counts[(size_t)job.set], 0);
        for (uint64_t i = 0; i < s.first; ++i) (*masks)[k][(size_t)i] = 1;
      }
    }
  }
};

static std::vector<double> random_points(size_t n, uint64_t seed) {
  std::vector<double> p(4 * n);
  for (size_t i = 0; i < 4 * n; ++i) p[i] = (double)(tvs::mix64(seed + i) % 100000) / 100.0;
  return p;
}

static tvg_ransac_options options(int min_trials, int max_trials, int per_round) {
  tvg_ransac_options o;
  o.max_error = 4.0;
  o.min_inlier_ratio = 0.1;
  o.confidence = 0.999;
  o.dyn_num_trials_multiplier = 3.0;
  o.min_num_trials = min_trials;
  o.max_num_trials = max_trials;
  o.random_seed = 0;
  o.trials_per_round = per_round;
  return o;
}

static bool tagged(const tp::Model& m, int set, int64_t trial, int j) {
  return m[3] == kTag && m[0] == set && m[1] == (double)trial && m[2] == j;
}

static void test_walk_traces() {
  const std::vector<int64_t> offsets = {0, 100};
  const std::vector<double> pts = random_points(100, 1);
  const Sup none(0, 0.0);
  for (int per_round : {1, 2, 64}) {
    // A. the stopping check sits inside the loop over a sample's models: trial 0 finds all 100 matches, so one trial is
    // enough; trial 1's first model is no better and the search stops THERE, before its second, better model.
    {
      Script dev;
      dev.upload(offsets, pts, {0});
      dev.sample = [&](int, int64_t t) -> std::vector<Sup> {
        if (t == 0) return {{5, 1.0}, {100, 50.0}};
        return {{100, 60.0}, {100, 1.0}, {100, 0.5}};
      };
      dev.refit = [&](int, int64_t, int, int) { return Sup(100, 70.0); };  // no improvement
      const tp::Report r = tp::estimate(dev, tvs::KIND_F, options(0, 1000, per_round), offsets, pts, nullptr, nullptr)[0];
      CHECK(r.success && r.num_trials == 2 && r.support.num_inliers == 100 && r.support.residual_sum == 50.0);
      CHECK(tagged(r.model, 0, 0, 1));
      // asked: the mask of (t0, j1), its first refit, and the winner's mask; (t0, j0) has too few inliers for a refit
      CHECK(dev.log.size() == 3 && dev.log[0] == "s0 t0 j1" && dev.log[1] == "s0 t0 j1 r0" && dev.log[2] == "s0 t0 j1");
      CHECK(r.inlier_mask.size() == 100 && r.inlier_mask[99] == 1);
    }
    // B. a sample without a model is not checked: trial 1 gives none, so the search goes on to trial 2, whose first
    // model is compared (and taken) before the check stops it.
    {
      Script dev;
      dev.upload(offsets, pts, {0});
      dev.sample = [&](int, int64_t t) -> std::vector<Sup> {
        if (t == 0) return {{100, 50.0}};
        if (t == 1) return {};
        return {{100, 40.0}, {100, 1.0}};
      };
      dev.refit = [&](int, int64_t, int, int) { return none; };
      const tp::Report r = tp::estimate(dev, tvs::KIND_F, options(0, 1000, per_round), offsets, pts, nullptr, nullptr)[0];
      CHECK(r.num_trials == 3 && r.support.residual_sum == 40.0 && tagged(r.model, 0, 2, 0));
    }
    // C. min_num_trials keeps a finished search going: it stops at trial 5, the counter reads 6
    {
      Script dev;
      dev.upload(offsets, pts, {0});
      dev.sample = [&](int, int64_t) -> std::vector<Sup> { return {{100, 50.0}}; };
      dev.refit = [&](int, int64_t, int, int) { return none; };
      const tp::Report r = tp::estimate(dev, tvs::KIND_F, options(5, 1000, per_round), offsets, pts, nullptr, nullptr)[0];
      CHECK(r.num_trials == 6 && tagged(r.model, 0, 0, 0));
    }
    // D. the clamp: nothing is ever found, the search runs out at the clamped maximum and the counter is one past it
    {
      Script dev;
      dev.upload(offsets, pts, {0});
      dev.sample = [&](int, int64_t) -> std::vector<Sup> { return {}; };
      dev.refit = [&](int, int64_t, int, int) { return none; };
      tvg_ransac_options o = options(0, 1000, per_round);
      o.min_inlier_ratio = 0.7;
      o.confidence = 0.99;
      const uint64_t clamp = tp::clamped_max_num_trials(o, 0.7, 7);
      CHECK(clamp == tp::compute_num_trials(70000, 100000, 0.99, 3.0, 7) && clamp > 100 && clamp < 1000);
      const tp::Report r = tp::estimate(dev, tvs::KIND_F, o, offsets, pts, nullptr, nullptr)[0];
      CHECK(!r.success && !r.has_model && r.num_trials == clamp + 1 && r.support.num_inliers == 0);
      o.max_num_trials = 7;
      CHECK(tp::estimate(dev, tvs::KIND_F, o, offsets, pts, nullptr, nullptr)[0].num_trials == 8);
    }
    // E. local refits stop at the first that does not improve, and at ten
    {
      Script dev;
      dev.upload(offsets, pts, {0});
      dev.sample = [&](int, int64_t t) -> std::vector<Sup> { return t == 0 ? std::vector<Sup>{{50, 9.0}} : std::vector<Sup>{}; };
      dev.refit = [&](int, int64_t, int, int k) { return k == 0 ? Sup(60, 9.0) : k == 1 ? Sup(70, 9.0) : Sup(65, 1.0); };
      tp::Report r = tp::estimate(dev, tvs::KIND_F, options(0, 3, per_round), offsets, pts, nullptr, nullptr)[0];
      CHECK(r.support.num_inliers == 70 && r.model[3] != kTag && r.num_trials == 4);
      CHECK(dev.log.size() == 5 && dev.log[3] == "s0 t0 j0 r2");  // mask, three refits, the winner (untagged: counted as r3)
      Script ten;
      ten.upload(offsets, pts, {0});
      ten.sample = dev.sample;
      ten.refit = [&](int, int64_t, int, int k) { return Sup(51 + (uint64_t)k, 9.0); };
      r = tp::estimate(ten, tvs::KIND_F, options(0, 3, per_round), offsets, pts, nullptr, nullptr)[0];
      CHECK(r.support.num_inliers == 60 && ten.log.size() == 12 && ten.log[10] == "s0 t0 j0 r9");
      // the same support again is not better: a sample with at most 7 inliers is never refitted
      Script few;
      few.upload(offsets, pts, {0});
      few.sample = [&](int, int64_t t) -> std::vector<Sup> { return t == 0 ? std::vector<Sup>{{7, 1.0}} : std::vector<Sup>{}; };
      few.refit = dev.refit;
      r = tp::estimate(few, tvs::KIND_F, options(0, 3, per_round), offsets, pts, nullptr, nullptr)[0];
      CHECK(r.success && r.support.num_inliers == 7 && few.log.size() == 1);
      few.sample = [&](int, int64_t t) -> std::vector<Sup> { return t == 0 ? std::vector<Sup>{{6, 1.0}} : std::vector<Sup>{}; };
      r = tp::estimate(few, tvs::KIND_F, options(0, 3, per_round), offsets, pts, nullptr, nullptr)[0];
      CHECK(!r.success && r.has_model && r.support.num_inliers == 6);
    }
  }
}

// several sets park and resume in the same launches; every set's report equals the one it gets alone, for every T
static void test_parking() {
  const int S = 5;
  std::vector<int64_t> offsets = {0};
  std::vector<double> pts;
  for (int s = 0; s < S; ++s) {
    const size_t n = s == 3 ? 5 : 40 + 10 * (size_t)s;  // set 3 is below the minimal sample
    const std::vector<double> p = random_points(n, 100 + (uint64_t)s);
    pts.insert(pts.end(), p.begin(), p.end());
    offsets.push_back(offsets.back() + (int64_t)n);
  }
  auto sample = [&](int set, int64_t t) -> std::vector<Sup> {
    const uint64_t h = tvs::mix64((uint64_t)set * 1000003ull + (uint64_t)t);
    const uint64_t n = (uint64_t)(offsets[(size_t)set + 1] - offsets[(size_t)set]);
    std::vector<Sup> out;
    for (uint64_t j = 0; j < h % 4; ++j) {
      const uint64_t g = tvs::mix64(h + j);
      out.push_back(Sup(std::min<uint64_t>(n, (g % n) * (uint64_t)(t + 1) / 40 + 1), (double)(g % 977)));
    }
    return out;
  };
  auto refit = [&](int set, int64_t t, int j, int k) {
    const uint64_t n = (uint64_t)(offsets[(size_t)set + 1] - offsets[(size_t)set]);
    const uint64_t g = tvs::mix64((uint64_t)set * 7919ull + (uint64_t)t * 31ull + (uint64_t)j * 7ull + (uint64_t)k);
    return Sup(std::min<uint64_t>(n, sample(set, t)[(size_t)j].first + g % 5 - 1), (double)(g % 100));
  };
  std::vector<tp::Report> base;
  for (int per_round : {64, 1, 3, 63, 65}) {
    Script dev;
    dev.upload(offsets, pts, std::vector<uint64_t>(S, 0));
    dev.sample = sample;
    dev.refit = refit;
    const std::vector<tp::Report> r = tp::estimate(dev, tvs::KIND_F, options(20, 200, per_round), offsets, pts, nullptr, nullptr);
    if (base.empty()) {
      base = r;
      CHECK(!r[3].success && r[3].num_trials == 0);
      int launches = 0;
      for (const tp::Report& x : r) launches = std::max<int>(launches, (int)x.num_launches);
      CHECK(dev.scores + dev.rounds >= launches && dev.scores < (int)dev.log.size());  // requests of several sets share launches
    }
    for (int s = 0; s < S; ++s) {
      CHECK(r[(size_t)s].success == base[(size_t)s].success && r[(size_t)s].num_trials == base[(size_t)s].num_trials);
      CHECK(r[(size_t)s].support.num_inliers == base[(size_t)s].support.num_inliers);
      CHECK(r[(size_t)s].support.residual_sum == base[(size_t)s].support.residual_sum && r[(size_t)s].model == base[(size_t)s].model);
    }
  }
  for (int s = 0; s < S; ++s) {  // alone
    const std::vector<int64_t> one = {0, offsets[(size_t)s + 1] - offsets[(size_t)s]};
    const std::vector<double> p(pts.begin() + 4 * offsets[(size_t)s], pts.begin() + 4 * offsets[(size_t)s + 1]);
    Script dev;
    dev.upload(one, p, {0});
    dev.sample = [&](int, int64_t t) { return sample(s, t); };
    dev.refit = [&](int, int64_t t, int j, int k) { return refit(s, t, j, k); };
    const tp::Report r = tp::estimate(dev, tvs::KIND_F, options(20, 200, 0), one, p, nullptr, nullptr)[0];
    tp::Model m = r.model;
    if (m[3] == kTag) m[0] = (double)s;  // the tag names the set's position in its batch
    CHECK(r.num_trials == base[(size_t)s].num_trials && r.support.num_inliers == base[(size_t)s].support.num_inliers &&
          r.support.residual_sum == base[(size_t)s].support.residual_sum && m == base[(size_t)s].model);
  }
}

static void test_num_trials() {
  CHECK(tp::compute_num_trials(100, 100, 0.999, 3.0, 7) == 1);
  CHECK(tp::compute_num_trials(0, 100, 0.999, 3.0, 7) == tp::kNoLimit);
  CHECK(tp::compute_num_trials(50, 100, 1.0, 3.0, 7) == tp::kNoLimit);
  // 1 point: log(0.001) / log(0.75) * 3 = 72.03...
  CHECK(tp::compute_num_trials(25000, 100000, 0.999, 3.0, 1) == 73);
  // 4 points, half inliers of 8: (4 3 2 1) / (8 7 6 5) = 1 / 70
  const double want = std::ceil(std::log(0.01) / std::log(1.0 - 1.0 / 70.0) * 2.0);
  CHECK(std::fabs((double)tp::compute_num_trials(4, 8, 0.99, 2.0, 4) - want) <= 1.0);
  tvg_ransac_options o = options(0, 50, 0);
  CHECK(tp::clamped_max_num_trials(o, 0.25, 1) == 50);
  CHECK(tp::clamped_max_num_trials(o, 1.0, 7) == 1);
}

static tvg_camera cam(int model, int id, int prior) { return tvg_camera{model, 1000, 800, id, prior}; }

static void test_router() {
  namespace cm = colmap_amd::camera_models;
  tvg_options o;
  std::memset(&o, 0, sizeof o);
  const int PIN = cm::PINHOLE, FISH = cm::OPENCV_FISHEYE, SPH = cm::EQUIRECTANGULAR;
  CHECK(tp::route(cam(PIN, 1, 0), cam(PIN, 2, 0), o) == TVG_ROUTE_UNCALIBRATED);
  CHECK(tp::route(cam(cm::SIMPLE_RADIAL, 1, 0), cam(cm::OPENCV, 2, 0), o) == TVG_ROUTE_UNCALIBRATED);
  CHECK(tp::route(cam(PIN, 1, 0), cam(PIN, 1, 0), o) == TVG_ROUTE_SHARED_FOCAL);
  CHECK(tp::route(cam(FISH, 1, 0), cam(FISH, 1, 0), o) == TVG_ROUTE_FISHEYE_DEGENERATE);  // a shared fisheye is no pinhole
  CHECK(tp::route(cam(PIN, 1, 1), cam(PIN, 1, 1), o) == TVG_ROUTE_CALIBRATED);
  CHECK(tp::route(cam(PIN, 1, 1), cam(FISH, 2, 1), o) == TVG_ROUTE_CALIBRATED);
  CHECK(tp::route(cam(PIN, 1, 1), cam(PIN, 2, 0), o) == TVG_ROUTE_ONE_SIDED_FOCAL);
  CHECK(tp::route(cam(PIN, 1, 0), cam(FISH, 2, 1), o) == TVG_ROUTE_ONE_SIDED_FOCAL);
  CHECK(tp::route(cam(SPH, 1, 0), cam(PIN, 2, 0), o) == TVG_ROUTE_ONE_SIDED_FOCAL);       // spherical counts as calibrated
  CHECK(tp::route(cam(FISH, 1, 0), cam(PIN, 2, 1), o) == TVG_ROUTE_FISHEYE_DEGENERATE);   // the unknown side is no pinhole
  CHECK(tp::route(cam(SPH, 1, 0), cam(SPH, 2, 0), o) == TVG_ROUTE_SPHERICAL);
  CHECK(tp::route(cam(SPH, 1, 0), cam(PIN, 2, 1), o) == TVG_ROUTE_SPHERICAL);
  CHECK(tp::route(cam(SPH, 1, 0), cam(FISH, 2, 0), o) == TVG_ROUTE_SPHERICAL);            // one-sided needs a pinhole there
  CHECK(tp::route(cam(FISH, 1, 0), cam(PIN, 2, 0), o) == TVG_ROUTE_FISHEYE_DEGENERATE);
  CHECK(tp::route(cam(PIN, 1, 0), cam(FISH, 2, 0), o) == TVG_ROUTE_FISHEYE_DEGENERATE);
  o.force_H_use = 1;
  CHECK(tp::route(cam(PIN, 1, 1), cam(PIN, 1, 1), o) == TVG_ROUTE_FORCED_H);
  CHECK(tp::route(cam(PIN, 1, 0), cam(FISH, 2, 0), o) == TVG_ROUTE_FORCED_H_DEGENERATE);
  CHECK(tp::route(cam(SPH, 1, 0), cam(PIN, 2, 0), o) == TVG_ROUTE_FORCED_H_DEGENERATE);
  std::set<std::string> names;
  int built = 0;
  for (int r = 0; r < TVG_NUM_ROUTES; ++r) {
    names.insert(tp::route_name(r));
    built += tp::route_is_built(r) ? 1 : 0;
  }
  CHECK(names.size() == TVG_NUM_ROUTES && built == 4);
}

static void test_checks() {
  tvg_ransac_options o = options(0, 10, 0);
  tp::validate_ransac(o);
  auto bad = [&](std::function<void(tvg_ransac_options&)> f, const char* word) {
    tvg_ransac_options b = o;
    f(b);
    return fails_with([&] { tp::validate_ransac(b); }, word);
  };
  CHECK(bad([](tvg_ransac_options& b) { b.max_error = 0.0; }, "max_error"));
  CHECK(bad([](tvg_ransac_options& b) { b.min_inlier_ratio = 1.5; }, "min_inlier_ratio"));
  CHECK(bad([](tvg_ransac_options& b) { b.confidence = -0.1; }, "confidence"));
  CHECK(bad([](tvg_ransac_options& b) { b.min_num_trials = 11; }, "min_num_trials"));
  CHECK(bad([](tvg_ransac_options& b) { b.random_seed = -2; }, "random_seed"));
  CHECK(bad([](tvg_ransac_options& b) { b.trials_per_round = 5000; }, "trials_per_round"));
  CHECK(bad([](tvg_ransac_options& b) { b.dyn_num_trials_multiplier = 0.0; }, "dyn_num_trials_multiplier"));
  CHECK(fails_with([] { tp::check_kind(3); }, "kind"));
  // offsets sit in exactly sized heap arrays: a read past a bad entry would be reported by the sanitizers
  std::vector<int64_t> off = {0, 5, 3};
  std::vector<double> p(20);
  CHECK(fails_with([&] { tp::validate_offsets(2, off.data(), p.data(), "sets"); }, "decrease"));
  off = {1, 5};
  CHECK(fails_with([&] { tp::validate_offsets(1, off.data(), p.data(), "sets"); }, "first offset"));
  off = {0, 5};
  CHECK(fails_with([&] { tp::validate_offsets(1, off.data(), nullptr, "sets"); }, "null"));
  CHECK(fails_with([&] { tp::validate_offsets(-1, off.data(), p.data(), "sets"); }, "negative"));
  CHECK(fails_with([&] { tp::validate_camera(cam(99, 1, 0), "camera"); }, "unknown camera model"));
  // the layout pads every set to whole waves
  off = {0, 7, 7, 71, 135};
  const tp::SetLayout L = tp::make_layout(4, off.data());
  CHECK(L.begin[0] == 0 && L.begin[1] == 64 && L.begin[2] == 64 && L.begin[3] == 128 && L.num_rows == 192);
  CHECK(L.count[0] == 7 && L.count[1] == 0 && L.count[2] == 64 && L.count[3] == 64);
}

static void test_draw_and_estimators() {
  for (int kind = 0; kind < 3; ++kind)
    for (uint32_t n : {7u, 8u, 9u, 1000u})
      for (uint64_t t = 0; t < 50; ++t) {
        uint32_t a[7] = {0, 0, 0, 0, 0, 0, 0}, b[7] = {0, 0, 0, 0, 0, 0, 0};
        tvs::draw_sample(-1, 99, kind, t, n, a);
        tvs::draw_sample(0, 99, kind, t, n, b);  // -1 is treated as 0
        std::set<uint32_t> seen;
        for (int k = 0; k < tvs::min_samples(kind); ++k) {
          CHECK(a[k] == b[k] && a[k] < n);
          seen.insert(a[k]);
        }
        CHECK((int)seen.size() == tvs::min_samples(kind));
      }
  uint32_t a[7], b[7];
  tvs::draw_sample(0, 1, 0, 0, 1000, a);
  tvs::draw_sample(0, 2, 0, 0, 1000, b);
  CHECK(std::memcmp(a, b, sizeof a) != 0);
  // the minimal and local solvers on exact data: x2 = H x1 and x2^T F x1 = 0
  const double Ht[9] = {1.1, 0.02, 30.0, -0.03, 0.95, -12.0, 1e-5, -2e-5, 1.0};
  std::vector<double> p;
  std::vector<uint32_t> idx;
  for (uint32_t i = 0; i < 40; ++i) {
    const double x = (double)(tvs::mix64(i) % 1000), y = (double)(tvs::mix64(i + 77) % 800);
    const double w = Ht[6] * x + Ht[7] * y + Ht[8];
    const double q[4] = {x, y, (Ht[0] * x + Ht[1] * y + Ht[2]) / w, (Ht[3] * x + Ht[4] * y + Ht[5]) / w};
    p.insert(p.end(), q, q + 4);
    idx.push_back(i);
  }
  tp::Model H, F, T;
  CHECK(tp::estimate_h_dlt(p.data(), idx, &H));
  for (int k = 0; k < 9; ++k) CHECK(std::fabs(H[(size_t)k] / H[8] - Ht[k]) < 1e-7 * std::max(1.0, std::fabs(Ht[k])));
  struct Host {
    double w[tvs::kWorkDoubles];
    double& operator()(int k) { return w[k]; }
  } W;
  double x1[7], y1[7], x2[7], y2[7], m[3][9];
  for (int k = 0; k < 7; ++k) {
    x1[k] = p[4 * (size_t)k];
    y1[k] = p[4 * (size_t)k + 1];
    x2[k] = p[4 * (size_t)k + 2];
    y2[k] = p[4 * (size_t)k + 3];
  }
  CHECK(tvs::solve_h4(W, x1, y1, x2, y2, m[0]) == 1);
  for (int k = 0; k < 9; ++k) CHECK(std::fabs(m[0][k] - Ht[k]) < 1e-7 * std::max(1.0, std::fabs(Ht[k])));
  for (uint32_t i = 0; i < 40; ++i) CHECK(tvs::homography_error(m[0], p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]) < 1e-12);
  // coplanar points leave the 8-point system with a three-dimensional null space; any vector of it has zero error
  CHECK(tp::estimate_f8(p.data(), idx, &F));
  for (uint32_t i = 0; i < 40; ++i) CHECK(tvs::sampson_error(F.data(), p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]) < 1e-10);
  const double det = F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
  double norm = 0.0;
  for (double v : F) norm += v * v;
  CHECK(std::fabs(det) < 1e-12 * std::pow(norm, 1.5));  // rank 2
  const int nm = tvs::solve_f7(W, x1, y1, x2, y2, m);
  CHECK(nm == 0 || nm == 1 || nm == 3);
  CHECK(tp::estimate_t_mean(p.data(), {0, 1}, &T));
  CHECK(T[0] == (p[2] + p[6]) / 2.0 - (p[0] + p[4]) / 2.0);
  CHECK(!tp::estimate_f8(p.data(), {0, 1, 2, 3, 4, 5, 6}, &F));
  // four collinear points: no homography
  const double cx[4] = {10, 200, 350, 700}, cy[4] = {0, 0, 0, 0}, dx[4] = {15, 205, 355, 705};
  CHECK(tvs::solve_h4(W, cx, cy, dx, cy, m[0]) == 0);
  std::vector<double> line;
  for (int k = 0; k < 6; ++k) {
    const double q[4] = {10.0 + 50 * k, 20.0 + 100 * k, 30.0 + 50 * k, 25.0 + 100 * k};
    line.insert(line.end(), q, q + 4);
  }
  CHECK(!tp::estimate_h_dlt(line.data(), {0, 1, 2, 3, 4, 5}, &H));  // rank < 8
}

// decisions of two_view_geometry.cc:292-320 and :216-226 on hand-made reports
static void test_decisions() {
  tvg_options o;
  std::memset(&o, 0, sizeof o);
  o.min_num_inliers = 15;
  o.max_H_inlier_ratio = 0.8;
  o.ransac = options(0, 10, 0);
  auto report = [](bool success, uint64_t n, uint8_t fill) {
    tp::Report r;
    r.success = r.has_model = success;
    r.support.num_inliers = n;
    r.inlier_mask.assign(4, fill);
    return r;
  };
  CHECK(tp::decide_uncalibrated(report(false, 0, 0), report(false, 0, 0), o).config == TVG_CONFIG_DEGENERATE);
  CHECK(tp::decide_uncalibrated(report(true, 14, 1), report(true, 14, 2), o).config == TVG_CONFIG_DEGENERATE);
  tp::Geometry g = tp::decide_uncalibrated(report(true, 100, 1), report(true, 80, 2), o);  // 0.8 is not above 0.8
  CHECK(g.config == TVG_CONFIG_UNCALIBRATED && g.inlier_mask[0] == 1 && g.num_inliers == 100);
  g = tp::decide_uncalibrated(report(true, 100, 1), report(true, 81, 2), o);
  CHECK(g.config == TVG_CONFIG_PLANAR_OR_PANORAMIC && g.inlier_mask[0] == 1 && g.num_inliers == 100);
  g = tp::decide_uncalibrated(report(true, 100, 1), report(true, 100, 2), o);
  CHECK(g.config == TVG_CONFIG_PLANAR_OR_PANORAMIC && g.inlier_mask[0] == 2);
  g = tp::decide_uncalibrated(report(false, 0, 1), report(true, 20, 2), o);  // 20 / 0 = inf
  CHECK(g.config == TVG_CONFIG_PLANAR_OR_PANORAMIC && g.inlier_mask[0] == 2 && g.num_inliers == 20);
  CHECK(tp::decide_forced_homography(report(true, 14, 2), o).config == TVG_CONFIG_DEGENERATE);
  CHECK(tp::decide_forced_homography(report(true, 15, 2), o).config == TVG_CONFIG_PLANAR_OR_PANORAMIC);
  CHECK(tp::homography_min_inlier_ratio(o, 50, 100) == 0.4 && tp::homography_min_inlier_ratio(o, 5, 100) == 0.1);
  CHECK(tp::iteration_stream(42, 0) == 42 && tp::iteration_stream(42, 1) != 42 && tp::iteration_stream(42, 1) != tp::iteration_stream(42, 2));
}

static int print_svd(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return 2;
  int m = 0;
  if (std::fscanf(f, "%d", &m) != 1 || m <= 0) return 2;
  tp::JacobiSvd svd;
  svd.n = 9;
  svd.a.assign(9, std::vector<double>((size_t)m));
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < 9; ++c)
      if (std::fscanf(f, "%lf", &svd.a[(size_t)c][(size_t)r]) != 1) return 2;
  std::fclose(f);
  svd.compute();
  for (int k = 0; k < 9; ++k) std::printf("%.17g ", svd.sigma[svd.order[k]]);
  std::printf("\n");
  for (int k = 0; k < 9; ++k) std::printf("%.17g ", svd.v[svd.order[8]][k]);
  std::printf("\n%d\n", svd.rank((size_t)m));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "svd") == 0) return print_svd(argv[2]);
  test_walk_traces();
  test_parking();
  test_num_trials();
  test_router();
  test_checks();
  test_draw_and_estimators();
  test_decisions();
  std::printf("two-view plan checks OK\n");
  return 0;
}
