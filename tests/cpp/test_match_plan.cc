// The host plan of descriptor matching (colmap_amd/csrc/match_plan.h) without a GPU: the finish on scripted
// (idx, best, second) triples, the tile table, the device image of a set, and the argument checks. Stand-alone: g++
// alone, also under -fsanitize=address,undefined (tests/test_match_plan.py) -- the arrays are exactly sized on the heap.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "match_plan.h"

namespace mp = match_plan;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

template <typename F>
static bool fails(F&& f, const char* needle) {
  try {
    f();
  } catch (const mp::Fail& e) {
    return std::string(e.what()).find(needle) != std::string::npos;
  }
  return false;
}

static match_options defaults() {
  match_options o;
  mp::options_init(&o);
  return o;
}

// a dot whose distance acos(dot / 262144) is `angle`
static int32_t dot_at(double angle) { return (int32_t)std::lround(262144.0 * std::cos(angle)); }

static std::vector<uint32_t> run(const std::vector<int32_t>& s12, const std::vector<int32_t>& s21, const match_options& o) {
  // exactly sized heap copies: a read past the end is the sanitizer's
  std::unique_ptr<int32_t[]> a(new int32_t[s12.size()]), b(new int32_t[s21.size()]);
  std::copy(s12.begin(), s12.end(), a.get());
  std::copy(s21.begin(), s21.end(), b.get());
  std::vector<uint32_t> m;
  mp::finish(a.get(), (int64_t)s12.size() / 3, b.get(), (int64_t)s21.size() / 3, o, &m);
  return m;
}

static void test_options() {
  const match_options o = defaults();
  EXPECT(o.max_ratio == 0.8f && o.max_distance == 0.7f && o.cross_check == 1 && o.min_num_inliers == 15);
  mp::check_options(&o);
  EXPECT(fails([] { mp::check_options(nullptr); }, "options is null"));
  match_options bad = o;
  bad.max_ratio = 0.0f;
  EXPECT(fails([&] { mp::check_options(&bad); }, "max_ratio"));
  bad = o;
  bad.max_distance = -1.0f;
  EXPECT(fails([&] { mp::check_options(&bad); }, "max_distance"));
  bad = o;
  bad.min_num_inliers = -1;
  EXPECT(fails([&] { mp::check_options(&bad); }, "min_num_inliers"));
}

static void test_decide() {
  const int32_t good = dot_at(0.3), far = dot_at(0.9), weak = dot_at(0.65);
  const int32_t none[3] = {-1, 0, 0};
  EXPECT(mp::decide(none, 0.8f, 0.7f) == -1);                       // all-zero row
  const int32_t accept[3] = {4, good, far};
  EXPECT(mp::decide(accept, 0.8f, 0.7f) == 4);
  const int32_t tie[3] = {4, good, good};
  EXPECT(mp::decide(tie, 0.8f, 0.7f) == -1);                        // best == second: d1 >= 0.8 d1
  EXPECT(mp::decide(tie, 1.5f, 0.7f) == 4);                         // visible with a ratio above 1
  const int32_t too_far[3] = {4, far, 0};
  EXPECT(mp::decide(too_far, 0.8f, 0.7f) == -1);                    // d1 = 0.9 > 0.7
  EXPECT(mp::decide(too_far, 0.8f, 2.0f) == 4);
  const int32_t single[3] = {0, good, 0};                           // a single column: second = 0, d2 = pi / 2
  EXPECT(mp::decide(single, 0.8f, 0.7f) == 0);
  const int32_t ratio[3] = {2, weak, dot_at(0.7)};                  // 0.65 >= 0.8 * 0.7
  EXPECT(mp::decide(ratio, 0.8f, 0.7f) == -1);
  const int32_t above_norm[3] = {1, 128 * 255 * 255, 0};            // min(., 1): acos(1) = 0
  EXPECT(mp::decide(above_norm, 0.8f, 0.7f) == 1);
  // exactly on the distance threshold: `>` keeps it
  const int32_t v = dot_at(0.5);
  const float d = acosf((float)v * (float)(1.0 / 262144.0));
  const int32_t edge[3] = {7, v, 0};
  EXPECT(mp::decide(edge, 0.8f, d) == 7);
  EXPECT(mp::decide(edge, 0.8f, std::nextafterf(d, 0.0f)) == -1);
}

static void test_finish() {
  match_options o = defaults();
  o.min_num_inliers = 0;
  const int32_t g = dot_at(0.3), f = dot_at(0.9);
  // 4 rows against 3 columns: row 0 -> col 1 (mutual), row 1 -> col 1 (not mutual), row 2 all zero, row 3 -> col 0 (mutual)
  const std::vector<int32_t> s12 = {1, g, f, 1, g - 5, f, -1, 0, 0, 0, g, f};
  const std::vector<int32_t> s21 = {3, g, f, 0, g, f, -1, 0, 0};
  EXPECT((run(s12, s21, o) == std::vector<uint32_t>{0, 1, 3, 0}));
  o.cross_check = 0;
  EXPECT((run(s12, s21, o) == std::vector<uint32_t>{0, 1, 1, 1, 3, 0}));
  // the column direction rejects its own match by ratio: the cross check drops the pair
  o.cross_check = 1;
  const std::vector<int32_t> s21_tie = {3, g, g, 0, g, f, -1, 0, 0};
  EXPECT((run(s12, s21_tie, o) == std::vector<uint32_t>{0, 1}));
  // min_num_inliers: 2 matches stay at 2, vanish at 3
  o.min_num_inliers = 2;
  EXPECT(run(s12, s21, o).size() == 4);
  o.min_num_inliers = 3;
  EXPECT(run(s12, s21, o).empty());
  // empty sides
  o.min_num_inliers = 0;
  EXPECT(run({}, s21, o).empty());
  EXPECT(run({}, {}, defaults()).empty());
  EXPECT(run({-1, 0, 0, -1, 0, 0}, {}, o).empty());
  // a single column
  EXPECT((run({0, g, 0}, {0, g, 0}, o) == std::vector<uint32_t>{0, 0}));
  // a column beyond the other set is refused, not read
  o.cross_check = 0;
  EXPECT(fails([&] { run({5, g, f}, s21, o); }, "beyond the other set"));
  std::vector<uint32_t> m;
  EXPECT(fails([&] { mp::finish(nullptr, 2, nullptr, 0, o, &m); }, "selection of direction 0 is null"));
}

static void test_device_image() {
  EXPECT(mp::padded_rows(0) == 0 && mp::padded_rows(1) == 64 && mp::padded_rows(64) == 64 && mp::padded_rows(65) == 128);
  EXPECT(mp::device_bytes(65) == 128 * 132);
  const int rows = 3;
  std::unique_ptr<uint8_t[]> data(new uint8_t[rows * 128]);
  for (int k = 0; k < 128; ++k) {
    data[k] = 0;
    data[128 + k] = 255;
    data[256 + k] = (uint8_t)(k * 2);
  }
  std::vector<int8_t> desc;
  std::vector<int32_t> corr;
  mp::build_device_image(data.get(), rows, &desc, &corr);
  EXPECT(desc.size() == 64 * 128 && corr.size() == 64);
  EXPECT(desc[0] == -128 && desc[128] == 127 && desc[256 + 5] == 10 - 128 && desc[256 + 100] == 200 - 128);
  EXPECT(corr[0] == -mp::kRowBias && corr[1] == 128 * 128 * 255 - mp::kRowBias);
  for (int r = rows; r < 64; ++r) {
    EXPECT(corr[r] == mp::kAbsent);
    for (int k = 0; k < 128; ++k) EXPECT(desc[r * 128 + k] == 0);
  }
  // the biased product plus the corrections is the unsigned dot, 255 included
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < rows; ++j) {
      int32_t acc = 0, dot = 0, sum_j = 0;
      for (int k = 0; k < 128; ++k) {
        acc += (int32_t)desc[i * 128 + k] * (int32_t)desc[j * 128 + k];
        dot += (int32_t)data[i * 128 + k] * (int32_t)data[j * 128 + k];
        sum_j += data[j * 128 + k];
      }
      EXPECT(acc + corr[i] + 128 * sum_j == dot);
      EXPECT(acc + corr[i] > -(1 << 22) && acc + corr[i] < (1 << 23));  // the key of the kernel cannot overflow
    }
  EXPECT((int64_t)mp::kAbsent * 256 == INT32_MIN);
  mp::build_device_image(nullptr, 0, &desc, &corr);
  EXPECT(desc.empty() && corr.empty());
}

static void test_checks() {
  bool truncated = true;
  uint8_t byte = 0;
  EXPECT(mp::check_descriptors(0, 128, nullptr, 100, &truncated) == 0 && !truncated);
  EXPECT(mp::check_descriptors(100, 128, &byte, 100, &truncated) == 100 && !truncated);
  EXPECT(mp::check_descriptors(150, 128, &byte, 100, &truncated) == 100 && truncated);
  EXPECT(fails([&] { mp::check_descriptors(3, 64, &byte, 100, &truncated); }, "128 columns"));
  EXPECT(fails([&] { mp::check_descriptors(3, 128, nullptr, 100, &truncated); }, "data is null"));
  EXPECT(fails([&] { mp::check_descriptors(-1, 128, &byte, 100, &truncated); }, "negative"));
  EXPECT(mp::effective_max_num_matches(0) == 32768 && mp::effective_max_num_matches(7) == 7);
  EXPECT(fails([] { mp::effective_max_num_matches(-1); }, "max_num_matches"));
  EXPECT(mp::effective_cache_bytes(0, 32768) == mp::kDefaultCacheBytes);
  EXPECT(mp::effective_cache_bytes(1, 100) == 2 * mp::device_bytes(100));  // never less than one pair
  EXPECT(mp::effective_cache_bytes(1 << 20, 100) == (1 << 20));
}

static void test_tiles() {
  const int T = mp::kTileRows;
  // sizes 0, 1, 16, 17, a whole tile, a tile and one, two tiles and a bit
  const std::vector<int32_t> rows = {0, 1, 16, 17, T, T + 1, 2 * T + 5};
  for (size_t a = 0; a < rows.size(); ++a)
    for (size_t b = 0; b < rows.size(); ++b) {
      const mp::PairSlots p{(int32_t)a, (int32_t)b};
      const mp::Launch L = mp::build_launch(rows, &p, 1);
      const size_t ta = (rows[a] + T - 1) / T, tb = (rows[b] + T - 1) / T;
      EXPECT(L.tiles.size() == ta + tb);
      EXPECT(L.out_rows == rows[a] + rows[b] && L.out_row0[0] == 0 && L.out_row0[1] == rows[a]);
      for (size_t t = 0; t < L.tiles.size(); ++t) {
        const bool first = t < ta;
        EXPECT(L.tiles[t].query_set == (int32_t)(first ? a : b) && L.tiles[t].stream_set == (int32_t)(first ? b : a));
        EXPECT(L.tiles[t].query_row0 == (int32_t)((first ? t : t - ta) * T));
        EXPECT(L.tiles[t].out_row0 == (first ? 0 : rows[a]));
      }
    }
  // a mixed batch: every output row is owned by exactly one (tile, row)
  const std::vector<mp::PairSlots> batch = {{6, 1}, {0, 3}, {3, 3}, {5, 2}, {1, 0}, {4, 6}, {2, 5}};
  const mp::Launch L = mp::build_launch(rows, batch.data(), (int)batch.size());
  std::vector<int> owner(L.out_rows, 0);
  for (const mp::Tile& t : L.tiles)
    for (int r = t.query_row0; r < std::min(rows[t.query_set], t.query_row0 + T); ++r) ++owner[t.out_row0 + r];
  for (int c : owner) EXPECT(c == 1);
  int64_t expect = 0;
  for (size_t p = 0; p < batch.size(); ++p) {
    EXPECT(L.out_row0[2 * p] == expect);
    expect += rows[batch[p].set1];
    EXPECT(L.out_row0[2 * p + 1] == expect);
    expect += rows[batch[p].set2];
  }
  EXPECT(L.out_rows == expect);
  // a pair's tiles do not depend on the batch: the same (query, stream, row0) sequence alone and inside
  const mp::Launch alone = mp::build_launch(rows, &batch[3], 1);
  size_t at = 0;
  while (at < L.tiles.size() && L.tiles[at].out_row0 != L.out_row0[6]) ++at;
  for (size_t t = 0; t < alone.tiles.size(); ++t) {
    EXPECT(L.tiles[at + t].query_set == alone.tiles[t].query_set && L.tiles[at + t].query_row0 == alone.tiles[t].query_row0);
    EXPECT(L.tiles[at + t].out_row0 - L.out_row0[6] == alone.tiles[t].out_row0);
  }
  // refusals
  EXPECT(mp::build_launch(rows, nullptr, 0).tiles.empty());
  EXPECT(fails([&] { mp::build_launch(rows, nullptr, 1); }, "pairs is null"));
  EXPECT(fails([&] { mp::build_launch(rows, batch.data(), -1); }, "negative"));
  const mp::PairSlots unknown{0, 7}, negative{-1, 0};
  EXPECT(fails([&] { mp::build_launch(rows, &unknown, 1); }, "unknown descriptor slot"));
  EXPECT(fails([&] { mp::build_launch(rows, &negative, 1); }, "unknown descriptor slot"));
}

int main() {
  test_options();
  test_decide();
  test_finish();
  test_device_image();
  test_checks();
  test_tiles();
  std::printf("match plan checks OK\n");
  return 0;
}
