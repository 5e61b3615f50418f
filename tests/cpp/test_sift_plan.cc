// The host plan of SIFT extraction (colmap_amd/csrc/sift_plan.h), with g++ alone: options, octave sizes (odd halves),
// sigmas and the `sa > sb` tests, the Gaussian taps, the exp(-x) table, the order key, the capacity and its growth, the
// cut to max_num_features with the reference's quirk, the UBC permutation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "sift_plan.h"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

namespace sp = sift_plan;

static void options() {
  sp::Options o;
  EXPECT(o.max_num_features == 8192 && o.first_octave == -1 && o.num_octaves == 4 && o.octave_resolution == 3);
  EXPECT(o.peak_threshold == 0.02 / 3.0 && o.edge_threshold == 10.0 && o.max_num_orientations == 2 && !o.upright);
  EXPECT(sp::check(o).empty());
  struct { int sp::Options::*field; int value; const char* word; } bad[] = {
      {&sp::Options::max_num_features, 0, "max_num_features"}, {&sp::Options::octave_resolution, 0, "octave_resolution"},
      {&sp::Options::max_num_orientations, 0, "max_num_orientations"}, {&sp::Options::normalization, 2, "normalization"},
      {&sp::Options::first_octave, -2, "first_octave"}, {&sp::Options::num_octaves, 0, "num_octaves"}};
  for (const auto& b : bad) {
    sp::Options p;
    p.*(b.field) = b.value;
    EXPECT(sp::check(p).find(b.word) != std::string::npos);
  }
  sp::Options p;
  p.peak_threshold = 0.0;
  EXPECT(sp::check(p).find("peak_threshold") != std::string::npos);
  p = sp::Options();
  p.edge_threshold = -1.0;
  EXPECT(sp::check(p).find("edge_threshold") != std::string::npos);
}

static void geometry() {
  sp::Options o;
  sp::Geometry g = sp::geometry(67, 45, o);
  EXPECT(g.O == 4 && g.S == 3 && g.o_min == -1 && g.s_min == -1 && g.s_max == 4);
  EXPECT(g.num_levels() == 6 && g.num_dog() == 5 && g.num_grad() == 3);
  const int ws[] = {134, 67, 33, 16}, hs[] = {90, 45, 22, 11};
  for (int k = 0; k < 4; ++k) EXPECT(g.octave_width(-1 + k) == ws[k] && g.octave_height(-1 + k) == hs[k]);
  EXPECT(sp::num_octaves_run(g) == 4);
  EXPECT(g.sigman == 0.5 && g.sigmak == pow(2.0, 1.0 / 3) && g.sigma0 == 1.6 * g.sigmak);
  EXPECT(g.dsigma0 == g.sigma0 * sqrt(1.0 - 1.0 / (g.sigmak * g.sigmak)));
  EXPECT(sp::seed_level(g) == 2);
  // first octave at o_min = -1: sa = 1.6, sb = 1 -> sqrt(1.56); later octaves: sa == sb, no smoothing
  sp::Smoothing s = sp::base_smoothing(g, true);
  EXPECT(s.apply && std::fabs(s.sigma - sqrt(1.6 * 1.6 - 1.0)) < 1e-12);
  EXPECT(!sp::base_smoothing(g, false).apply);
  o.first_octave = 0;
  s = sp::base_smoothing(sp::geometry(67, 45, o), true);
  EXPECT(s.apply && std::fabs(s.sigma - sqrt(1.6 * 1.6 - 0.25)) < 1e-12);
  o.first_octave = 2;  // sb = 0.125
  EXPECT(sp::geometry(67, 45, o).octave_width(2) == 16 && sp::base_smoothing(sp::geometry(67, 45, o), true).apply);
  const int want_w[] = {5, 7, 8, 10, 13};  // ceil(4 dsigma0 sigmak^s), s = 0..4: up to 27 taps
  for (int i = 0; i < 5; ++i) {
    EXPECT(sp::level_sigma(g, i) == g.dsigma0 * pow(g.sigmak, (double)i));
    EXPECT(sp::gaussian_half_width(sp::level_sigma(g, i)) == want_w[i]);
  }
  // a 1 x 1 image: octave -1 is 2 x 2, octave 0 is below 2 x 2 and ends the walk
  EXPECT(sp::num_octaves_run(sp::geometry(1, 1, sp::Options())) == 1);
  // num_octaves < 0: floor(log2(min(w, h))) - o_min - 3, at least 1
  sp::Options n;
  n.num_octaves = -1;
  EXPECT(sp::geometry(640, 480, n).O == 8 - (-1) - 3 && sp::geometry(9, 9, n).O == 1);
  // octave_resolution 1 needs 45 taps a side at its last level: above the halo limit
  sp::Options r1;
  r1.octave_resolution = 1;
  EXPECT(sp::gaussian_half_width(sp::level_sigma(sp::geometry(64, 64, r1), 2)) == 45 && 45 > sp::kHaloLimit);
  sp::Options r2;
  r2.octave_resolution = 2;
  EXPECT(sp::gaussian_half_width(sp::level_sigma(sp::geometry(64, 64, r2), 3)) <= sp::kHaloLimit);
}

static void taps() {
  for (double sigma : {0.1, 0.25, 1.2489995996796797, 1.2262734984654078, 3.09, 7.9}) {
    const int W = sp::gaussian_half_width(sigma);
    EXPECT(W == (int)std::max(std::ceil(4.0 * sigma), 1.0));
    const std::vector<float> f = sp::gaussian_taps(sigma);
    EXPECT((int)f.size() == 2 * W + 1);
    float acc = 0;  // the stated recipe, once more
    std::vector<float> e(f.size());
    for (int j = 0; j < 2 * W + 1; ++j) {
      const float d = ((float)(j - W)) / ((float)sigma);
      e[j] = (float)exp(-0.5 * (d * d));
      acc += e[j];
    }
    double sum = 0;
    for (int j = 0; j < 2 * W + 1; ++j) {
      EXPECT(f[j] == e[j] / acc);
      EXPECT(f[j] == f[2 * W - j]);  // symmetric bit for bit: d * d is
      sum += f[j];
    }
    EXPECT(std::fabs(sum - 1.0) < 1e-6);
  }
  const std::vector<double> t = sp::expn_table();
  EXPECT(t.size() == 258 && t[0] == 1.0 && t[256] == exp(-25.0) && t[128] == exp(-12.5) && t[257] == 0.0);
}

static void order_and_capacity() {
  int x, y, s;
  sp::candidate_unkey(sp::candidate_key(1048575, 7, 5), &x, &y, &s);
  EXPECT(x == 1048575 && y == 7 && s == 5);
  EXPECT(sp::candidate_key(9, 9, 1) < sp::candidate_key(0, 0, 2));   // DoG level first
  EXPECT(sp::candidate_key(9, 3, 1) < sp::candidate_key(0, 4, 1));   // then rows
  EXPECT(sp::candidate_key(3, 4, 1) < sp::candidate_key(4, 4, 1));   // then columns
  EXPECT(sp::candidate_capacity(16, 11, 3) == 1024 && sp::candidate_capacity(320, 240, 3) == 3600);
  EXPECT(sp::candidate_capacity(6400, 4800, 3) == 1440000);
  EXPECT(sp::grown_capacity(1) == 1024 && sp::grown_capacity(1024) == 1024 && sp::grown_capacity(1025) == 2048);
  EXPECT(sp::grown_capacity(3000000) == 4194304);
}

static void cut_and_permutation() {
  // levels from fine to coarse: detections {19, 33, 6}, rows with orientations {22, 38, 8}
  const std::vector<int> nf = {10, 9, 20, 13, 4, 2}, nr = {12, 10, 25, 13, 6, 2};
  sp::Cut c = sp::cut_levels(nf, nr, 8192);
  EXPECT(c.first_level == 0 && c.num_out == 68);
  c = sp::cut_levels(nf, nr, 58);  // exactly all: not exceeded
  EXPECT(c.first_level == 0 && c.num_out == 68);
  c = sp::cut_levels(nf, nr, 25);  // 2 + 4 + 13 = 19 <= 25 < 39: the level that crosses is kept whole
  EXPECT(c.first_level == 2 && c.num_out == 2 + 6 + 13 + 25);
  c = sp::cut_levels(nf, nr, 1);   // the coarsest level alone already crosses
  EXPECT(c.first_level == 5 && c.num_out == 2);
  c = sp::cut_levels({}, {}, 10);
  EXPECT(c.first_level == 0 && c.num_out == 0);
  std::set<int> seen;
  const int q[8] = {0, 7, 6, 5, 4, 3, 2, 1};
  for (int k = 0; k < 128; ++k) {
    EXPECT(sp::ubc_index(k) == (k / 8) * 8 + q[k % 8]);
    EXPECT(sp::ubc_index(sp::ubc_index(k)) == k);
    seen.insert(sp::ubc_index(k));
  }
  EXPECT(seen.size() == 128);
  sp::Geometry g = sp::geometry(64, 48, sp::Options());
  EXPECT(sp::keypoint_sigma(g, 1.25, -1) == (float)(g.sigma0 * pow(2.0, 1.25 / 3) * 0.5));
}

int main() {
  options();
  geometry();
  taps();
  order_and_capacity();
  cut_and_permutation();
  std::printf("sift plan checks OK\n");
  return 0;
}
