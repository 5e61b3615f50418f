// The C++ surface of descriptor matching (include/colmap_amd/feature_matching.hpp) from g++, linked against the library:
//   nodevice  creating a matcher without a GPU fails loudly (exit 2)
//   known     on the GPU: a set and its permuted copy match row for row, one pair and a batch of three
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>

#include "colmap_amd/feature_matching.hpp"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

using namespace colmap_amd;

static void known() {
  const int n = 300;
  std::mt19937 rng(5);
  std::vector<uint8_t> a(n * 128), b(n * 128), c(n * 128);
  // uniform 0..39: |a|^2 is near 66 600 and a dot of two rows near 48 700, so the copy is the one best column and
  // both stay below 512^2 (distances above 0)
  for (auto& v : a) v = (uint8_t)(rng() % 40);
  std::vector<int> perm(n);
  std::iota(perm.begin(), perm.end(), 0);
  for (int i = n - 1; i > 0; --i) std::swap(perm[i], perm[rng() % (i + 1)]);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 128; ++k) {
      b[perm[i] * 128 + k] = a[i * 128 + k];
      c[i * 128 + k] = a[(n - 1 - i) * 128 + k];
    }
  SiftMatchingOptions options;
  options.max_ratio = 1.0;    // a copy has distance acos(|a|^2 / 512^2); only the ordering is under test here
  options.max_distance = 2.0;
  FeatureMatcher matcher(options);
  matcher.SetDescriptors(1, n, a.data());
  matcher.SetDescriptors(2, n, b.data());
  matcher.SetDescriptors(3, n, c.data());
  EXPECT(matcher.HasDescriptors(2) && !matcher.HasDescriptors(9));
  FeatureMatches m;
  matcher.Match(1, 2, &m);
  EXPECT((int)m.size() == n);
  for (int i = 0; i < n; ++i) EXPECT(m[i] == FeatureMatch(i, perm[i]));
  const auto all = matcher.Match({{1, 2}, {1, 3}, {3, 2}});
  EXPECT(all.size() == 3 && all[0] == m && (int)all[1].size() == n && (int)all[2].size() == n);
  for (int i = 0; i < n; ++i) {
    EXPECT(all[1][i] == FeatureMatch(i, n - 1 - i));
    EXPECT(all[2][i] == FeatureMatch(i, perm[n - 1 - i]));
  }
  try {
    matcher.Match(1, 9, &m);
    EXPECT(false);
  } catch (const std::runtime_error& e) {
    EXPECT(std::string(e.what()).find("image 9 has no descriptors") != std::string::npos);
  }
  std::printf("known OK\n");
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "nodevice";
  if (mode == "known") known();
  if (mode == "nodevice") {
    try {
      FeatureMatcher matcher;
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 2;
    }
  }
  return 0;
}
