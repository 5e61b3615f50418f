// sift_plan.h -- the host plan of SIFT extraction (sift.hip): options and their check, the geometry of the scale space,
// the smoothing of every level, the Gaussian taps and the exp(-x) table the device reads, the order of the detections and
// the assembly of the result. Plain C++17, no HIP: tests/cpp/test_sift_plan.cc drives it on its own.
//
// The arithmetic is the reference's VLFeat route (SiftCPUFeatureExtractor::Extract, feature/sift.cc:138-341, over
// thirdparty/VLFeat/sift.c): every double and every float below stands where the C code has it, and exp / pow / sqrt are
// the C library's, called here on the host and never on the device.
#ifndef COLMAP_AMD_SIFT_PLAN_H_
#define COLMAP_AMD_SIFT_PLAN_H_

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace sift_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

constexpr int kNormL1Root = 0, kNormL2 = 1;

// SiftExtractionOptions (feature/sift.h:41-101), the members of the built route
struct Options {
  int max_num_features = 8192;
  int first_octave = -1;
  int num_octaves = 4;
  int octave_resolution = 3;
  double peak_threshold = 0.02 / 3.0;
  double edge_threshold = 10.0;
  int max_num_orientations = 2;
  int upright = 0;
  int normalization = kNormL1Root;
};

// Sizes of the kernels (exported by sift.hip as functions for the tests).
constexpr int kColTileX = 64, kColTileY = 32;   // column pass: outputs of one workgroup
constexpr int kRowTileX = 128, kRowTileY = 8;   // row pass
constexpr int kHaloLimit = 32;                  // largest half-width W of a Gaussian the convolution kernels stage
constexpr int kMinCandidateCapacity = 1024;

// SiftExtractionOptions::Check (sift.cc:72-84) and what the kernels add: empty, or what is wrong
inline std::string check(const Options& o) {
  if (!(o.max_num_features > 0)) return "max_num_features must be > 0";
  if (!(o.octave_resolution > 0)) return "octave_resolution must be > 0";
  if (!(o.peak_threshold > 0.0)) return "peak_threshold must be > 0";
  if (!(o.edge_threshold > 0.0)) return "edge_threshold must be > 0";
  if (!(o.max_num_orientations > 0)) return "max_num_orientations must be > 0";
  if (o.normalization != kNormL1Root && o.normalization != kNormL2) return "normalization must be L1_ROOT (0) or L2 (1)";
  if (o.first_octave < -1) return "first_octave below -1 is not built (one doubling of the image only)";
  if (o.first_octave > 8) return "first_octave above 8 is not built";
  if (o.num_octaves == 0 || o.num_octaves > 32) return "num_octaves must be in 1..32, or negative for the largest number";
  if (o.octave_resolution > 16) return "octave_resolution above 16 is not built";
  return "";
}

inline int shift_left(int x, int n) { return n >= 0 ? x << n : x >> -n; }  // VL_SHIFT_LEFT

// vl_sift_new (sift.c:874-934)
struct Geometry {
  int width = 0, height = 0, O = 0, S = 0, o_min = 0, s_min = -1, s_max = 0;
  double sigman = 0.5, sigma0 = 0, sigmak = 0, dsigma0 = 0;
  int num_levels() const { return s_max - s_min + 1; }  // Gaussian levels of an octave
  int num_dog() const { return s_max - s_min; }         // DoG levels of an octave
  int num_grad() const { return S; }                    // gradient planes: levels s_min+1 .. s_max-2
  int octave_width(int o) const { return shift_left(width, -o); }
  int octave_height(int o) const { return shift_left(height, -o); }
};

inline Geometry geometry(int width, int height, const Options& o) {
  Geometry g;
  int noctaves = o.num_octaves;
  if (noctaves < 0) noctaves = (int)std::max(floor(log((double)std::min(width, height)) / 0.693147180559945) - o.first_octave - 3, 1.0);
  g.width = width;
  g.height = height;
  g.O = noctaves;
  g.S = o.octave_resolution;
  g.o_min = o.first_octave;
  g.s_min = -1;
  g.s_max = o.octave_resolution + 1;
  g.sigman = 0.5;
  g.sigmak = pow(2.0, 1.0 / o.octave_resolution);
  g.sigma0 = 1.6 * g.sigmak;
  g.dsigma0 = g.sigma0 * sqrt(1.0 - 1.0 / (g.sigmak * g.sigmak));
  return g;
}

// The octaves that are processed: VLFeat reads outside an octave narrower or lower than 2 pixels (update_gradient,
// "the minimum octave size is 2x2xS"), so the octaves end before the first such one.
inline int num_octaves_run(const Geometry& g) {
  int n = 0;
  while (n < g.O && g.octave_width(g.o_min + n) >= 2 && g.octave_height(g.o_min + n) >= 2) ++n;
  return n;
}

// The smoothing applied to level s_min of an octave after it was made (up-/down-sampled image, or decimated level
// s_best of the octave before): vl_sift_process_first_octave / _next_octave, with the `sa > sb` test and the powf of the
// latter.
struct Smoothing {
  bool apply = false;
  double sigma = 0.0;
};

inline Smoothing base_smoothing(const Geometry& g, bool first) {
  double sa, sb;
  if (first) {
    sa = g.sigma0 * pow(g.sigmak, (double)g.s_min);
    sb = g.sigman * pow(2.0, (double)-g.o_min);
  } else {
    const int s_best = std::min(g.s_min + g.S, g.s_max);
    sa = g.sigma0 * powf((float)g.sigmak, (float)g.s_min);
    sb = g.sigma0 * powf((float)g.sigmak, (float)(s_best - g.S));
  }
  Smoothing r;
  if (sa > sb) {
    r.apply = true;
    r.sigma = sqrt(sa * sa - sb * sb);
  }
  return r;
}

inline int seed_level(const Geometry& g) { return std::min(g.s_min + g.S, g.s_max); }  // s_best: seeds the next octave

inline double level_sigma(const Geometry& g, int s) { return g.dsigma0 * pow(g.sigmak, (double)s); }  // s_min < s <= s_max

// _vl_sift_smooth's filter (sift.c:782-797): half-width and 2 W + 1 normalised float taps
inline int gaussian_half_width(double sigma) { return (int)std::max(ceil(4.0 * sigma), 1.0); }

inline std::vector<float> gaussian_taps(double sigma) {
  const int W = gaussian_half_width(sigma);
  std::vector<float> f(2 * W + 1);
  float acc = 0;
  for (int j = 0; j < 2 * W + 1; ++j) {
    const float d = ((float)(j - W)) / ((float)sigma);
    f[j] = (float)exp(-0.5 * (d * d));
    acc += f[j];
  }
  for (int j = 0; j < 2 * W + 1; ++j) f[j] /= acc;
  return f;
}

// fast_expn's table (sift.c:671-720)
constexpr int kExpnSize = 256;
constexpr double kExpnMax = 25.0;
// VLFeat's 257 entries and one more, 0: x == 25 exactly passes the `x > 25` test and reads entry 257 with weight 0, which
// lies past the end of VLFeat's own table
inline std::vector<double> expn_table() {
  std::vector<double> t(kExpnSize + 2, 0.0);
  for (int k = 0; k < kExpnSize + 1; ++k) t[k] = exp(-(double)k * (kExpnMax / kExpnSize));
  return t;
}

// The order of vl_sift_detect's list: DoG level, then raster order. One key per candidate, sorted ascending.
constexpr uint64_t candidate_key(int x, int y, int s_index) { return ((uint64_t)s_index << 40) | ((uint64_t)y << 20) | (uint64_t)x; }
constexpr void candidate_unkey(uint64_t k, int* x, int* y, int* s_index) {
  *x = (int)(k & 0xfffffu);
  *y = (int)((k >> 20) & 0xfffffu);
  *s_index = (int)(k >> 40);
}
constexpr int kMaxOctaveDim = 1 << 20;

// Candidate capacity of an octave and how it grows after an overflow: to the next power of two that holds the count
inline int candidate_capacity(int w, int h, int S) {
  const long long guess = (long long)w * h * S / 64;
  return (int)std::min<long long>(std::max<long long>(guess, kMinCandidateCapacity), 1 << 28);
}
inline int grown_capacity(int count) {
  int c = kMinCandidateCapacity;
  while (c < count) c *= 2;
  return c;
}

// k->sigma of vl_sift_detect (sift.c:1422), from the refined scale index the device returns
inline float keypoint_sigma(const Geometry& g, double sn, int o) { return (float)(g.sigma0 * pow(2.0, sn / g.S) * pow(2.0, (double)o)); }

// sift.cc:294-305: the DoG levels (runs of equal `is` within an octave, octaves without a detection left out) are
// visited from the last to the first; the first level kept is the one at which the number of detections (not of
// orientations) exceeds max_num_features, and the output holds the orientations of every level visited, that one included.
struct Cut {
  int first_level = 0;
  int num_out = 0;
};
inline Cut cut_levels(const std::vector<int>& level_num_features, const std::vector<int>& level_num_rows, int max_num_features) {
  Cut c;
  int num_features = 0;
  for (int i = (int)level_num_rows.size() - 1; i >= 0; --i) {
    num_features += level_num_features[i];
    c.num_out += level_num_rows[i];
    if (num_features > max_num_features) {
      c.first_level = i;
      break;
    }
  }
  return c;
}

// TransformVLFeatToUBCFeatureDescriptors (sift.cc:120-136): UBC position of VLFeat bin k
constexpr int ubc_index(int k) { return (k & ~7) | ((8 - (k & 7)) & 7); }  // q = {0, 7, 6, 5, 4, 3, 2, 1}

}  // namespace sift_plan

#endif  // COLMAP_AMD_SIFT_PLAN_H_
