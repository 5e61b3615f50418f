// The host plan of the model statistics (colmap_amd/csrc/model_plan.h) against brute-force code of its own: input
// validation on exactly sized heap arrays (a read through a bad offset or index before its check shows under the
// sanitizers), the by-image order of the depth pass, the lane-group and selection classes, the pair totals, the cell
// index, the segments and rows made of a count table, and the limits. g++ alone, no HIP.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "model_plan.h"

#define EXPECT(cond)                                                                 \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

namespace {

namespace mp = model_plan;

struct Model {  // owns exactly sized arrays
  std::unique_ptr<float[]> R, T, points;
  std::unique_ptr<int64_t[]> offsets;
  std::unique_ptr<int32_t[]> track_image;
  model_flat m{};
};

Model make(int num_images, const std::vector<int>& lengths, std::mt19937& rng) {
  Model s;
  const size_t P = lengths.size();
  s.R.reset(new float[9 * (size_t)num_images]());
  s.T.reset(new float[3 * (size_t)num_images]());
  s.points.reset(new float[3 * P]());
  s.offsets.reset(new int64_t[P + 1]);
  s.offsets[0] = 0;
  for (size_t p = 0; p < P; ++p) s.offsets[p + 1] = s.offsets[p] + lengths[p];
  const int64_t O = s.offsets[P];
  s.track_image.reset(new int32_t[(size_t)O]);
  for (int64_t o = 0; o < O; ++o) s.track_image[o] = (int32_t)(rng() % (unsigned)num_images);
  s.m.num_images = num_images;
  s.m.num_points = (int64_t)P;
  s.m.num_observations = O;
  s.m.R = s.R.get();
  s.m.T = s.T.get();
  s.m.points = s.points.get();
  s.m.track_offsets = s.offsets.get();
  s.m.track_image = s.track_image.get();
  return s;
}

bool rejected(const model_flat& m, const char* what) {
  try {
    mp::validate(m);
  } catch (const mp::Fail& e) {
    const std::string msg = e.what();
    if (msg.rfind("Check failed: ", 0) != 0 || msg.find(what) == std::string::npos) {
      std::fprintf(stderr, "expected \"%s\", got \"%s\"\n", what, msg.c_str());
      return false;
    }
    return true;
  }
  std::fprintf(stderr, "expected \"%s\", but the model was accepted\n", what);
  return false;
}

template <typename F>
bool fails_with(F&& f, const char* what) {
  try {
    f();
  } catch (const mp::Fail& e) {
    return std::string(e.what()).rfind("Check failed: ", 0) == 0 && std::string(e.what()).find(what) != std::string::npos;
  }
  return false;
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  std::vector<int> lengths = {0, 1, 2, 3, 16, 17, 64, 65, 130, 2, 0, 5};
  for (int k = 0; k < 400; ++k) lengths.push_back((int)(rng() % 24));

  {  // validation: each rejected input sits in exactly sized arrays
    Model s = make(9, lengths, rng);
    mp::validate(s.m);
    { Model b = make(9, lengths, rng); b.m.num_points = -1; EXPECT(rejected(b.m, "must not be negative")); }
    { Model b = make(9, lengths, rng); b.m.num_images = mp::kMaxImages + 1; EXPECT(rejected(b.m, "exceeds the limit of the dense pair table, 8192 images")); }
    { Model b = make(9, lengths, rng); b.m.num_points = (int64_t)1 << 31; EXPECT(rejected(b.m, "num_points must fit a 32-bit index")); }
    { Model b = make(9, lengths, rng); b.m.num_observations = (int64_t)1 << 31; EXPECT(rejected(b.m, "num_observations must fit a 32-bit index")); }
    { Model b = make(9, lengths, rng); b.m.track_offsets = nullptr; EXPECT(rejected(b.m, "track_offsets is null")); }
    { Model b = make(9, lengths, rng); b.m.R = nullptr; EXPECT(rejected(b.m, "image arrays are null")); }
    { Model b = make(9, lengths, rng); b.m.points = nullptr; EXPECT(rejected(b.m, "points is null")); }
    { Model b = make(9, lengths, rng); b.m.track_image = nullptr; EXPECT(rejected(b.m, "track_image is null")); }
    { Model b = make(9, lengths, rng); b.offsets[0] = 1; EXPECT(rejected(b.m, "track_offsets must start at 0")); }
    { Model b = make(9, lengths, rng); b.offsets[5] = b.offsets[4] - 1; EXPECT(rejected(b.m, "track_offsets decreases at point 4")); }
    { Model b = make(9, lengths, rng); b.offsets[lengths.size()] += 3; EXPECT(rejected(b.m, "track_offsets must end at num_observations")); }
    { Model b = make(9, lengths, rng); b.offsets[3] = (int64_t)1 << 40; EXPECT(rejected(b.m, "track_offsets")); }  // never used as an index
    { Model b = make(9, lengths, rng); b.track_image[7] = 9; EXPECT(rejected(b.m, "observation 7: image index 9 out of range")); }
    { Model b = make(9, lengths, rng); b.track_image[0] = -1; EXPECT(rejected(b.m, "observation 0: image index -1 out of range")); }
    Model none = make(0, {}, rng);
    mp::validate(none.m);
    mp::validate_percentile(0.0);
    mp::validate_percentile(100.0);
    EXPECT(fails_with([] { mp::validate_percentile(-1e-9); }, "percentile must lie in [0, 100]"));
    EXPECT(fails_with([] { mp::validate_percentile(100.0001); }, "percentile must lie in [0, 100]"));
    EXPECT(fails_with([] { mp::validate_percentile(std::nan("")); }, "percentile must lie in [0, 100]"));
  }

  {  // the depth plan: a stable counting sort by image, the point of every observation, the selection classes
    Model s = make(9, lengths, rng);
    for (int64_t o = 0; o < s.m.num_observations; ++o)
      if (s.track_image[o] == 4) s.track_image[o] = 5;  // image 4 has no observation
    const mp::DepthPlan plan = mp::make_depth_plan(s.m);
    const int64_t O = s.m.num_observations;
    EXPECT((int64_t)plan.obs_order.size() == O && (int64_t)plan.obs_point.size() == O && plan.image_offsets.size() == 10);
    EXPECT(plan.image_offsets[0] == 0 && plan.image_offsets[9] == O && plan.image_offsets[4] == plan.image_offsets[5]);
    std::vector<char> seen((size_t)O, 0);
    for (int i = 0; i < 9; ++i)
      for (int64_t t = plan.image_offsets[i]; t < plan.image_offsets[i + 1]; ++t) {
        const int32_t o = plan.obs_order[(size_t)t];
        EXPECT(o >= 0 && o < O && !seen[(size_t)o] && s.track_image[o] == i);
        seen[(size_t)o] = 1;
        if (t > plan.image_offsets[i]) EXPECT(plan.obs_order[(size_t)t - 1] < o);
      }
    for (int64_t p = 0; p < s.m.num_points; ++p)
      for (int64_t o = s.offsets[p]; o < s.offsets[p + 1]; ++o) EXPECT(plan.obs_point[(size_t)o] == p);
    size_t listed = 0;
    for (int k = 0; k < 2; ++k) {
      listed += plan.select_ids[k].size();
      EXPECT(std::is_sorted(plan.select_ids[k].begin(), plan.select_ids[k].end()));
      for (int32_t i : plan.select_ids[k]) EXPECT(((plan.image_offsets[(size_t)i + 1] - plan.image_offsets[(size_t)i]) > 64) == (k == 1));
    }
    EXPECT(listed == 9);
    EXPECT(mp::select_class(0) == 0 && mp::select_class(64) == 0 && mp::select_class(65) == 1);
    EXPECT(mp::device_bytes_depth(s.m) >= O * 16);
  }

  {  // the pair plan: classes, totals in 64 bits, limits
    Model s = make(9, lengths, rng);
    const mp::PairPlan plan = mp::make_pair_plan(s.m);
    EXPECT(mp::length_class(16) == 0 && mp::length_class(17) == 1 && mp::length_class(64) == 1 && mp::length_class(65) == 2);
    int64_t total = 0;
    size_t listed = 0, want_listed = 0;
    for (size_t p = 0; p < lengths.size(); ++p) {
      for (int i = 0; i < lengths[p]; ++i) total += i;
      want_listed += lengths[p] >= 2;
    }
    for (int k = 0; k < mp::kNumClasses; ++k) {
      listed += plan.class_points[k].size();
      EXPECT(std::is_sorted(plan.class_points[k].begin(), plan.class_points[k].end()));
      for (int32_t p : plan.class_points[k]) EXPECT(lengths[(size_t)p] >= 2 && mp::length_class(lengths[(size_t)p]) == k);
    }
    EXPECT(listed == want_listed && plan.total_pairs == total && plan.num_cells == 36);
    EXPECT(mp::num_cells(0) == 0 && mp::num_cells(1) == 0 && mp::num_cells(2) == 1 && mp::num_cells(8192) == 33550336);
    EXPECT(mp::device_bytes_pairs(s.m, plan, 10) == mp::device_bytes_pairs(s.m, plan, 0) + 40);
    EXPECT(fails_with([] { mp::check_device_memory(11, 10); }, "bytes of device memory"));
    mp::check_device_memory(10, 10);
    // limits without the arrays: validate() is what reads them, the plan only reads the offsets
    int64_t big[3] = {0, 70000, 140000};  // one image pair could hold 2 * 35000^2 > 2^31 - 1 pairs
    model_flat m{};
    m.num_images = 2;
    m.num_points = 2;
    m.num_observations = 140000;
    m.track_offsets = big;
    EXPECT(fails_with([&] { mp::make_pair_plan(m); }, "more than 2^31 - 1 track pairs"));
    int64_t huge[2] = {0, 2000000000};  // L (L - 1) / 2 = 2e18 fits 64 bits and is refused by name
    m.num_points = 1;
    m.num_observations = 2000000000;
    m.track_offsets = huge;
    EXPECT(fails_with([&] { mp::make_pair_plan(m); }, "more than 2^40 pairs"));
  }

  {  // cell_index enumerates the upper triangle row by row; segments and rows of a count table
    const int I = 13;
    int64_t next = 0;
    for (int a = 0; a < I; ++a)
      for (int b = a + 1; b < I; ++b) EXPECT(mp::cell_index(a, b, I) == next++);
    EXPECT(next == mp::num_cells(I));
    EXPECT(mp::cell_index(8190, 8191, 8192) == mp::num_cells(8192) - 1);
    std::vector<int32_t> counts((size_t)next);
    std::vector<float> angles((size_t)next);
    int64_t pairs = 0;
    for (size_t c = 0; c < counts.size(); ++c) {
      const unsigned r = rng() % 5;
      counts[c] = r == 0 ? 0 : r == 1 ? 64 : r == 2 ? 65 : (int32_t)(rng() % 200);
      angles[c] = (float)c;
      pairs += counts[c];
    }
    const mp::CellSegments seg = mp::make_cell_segments(counts.data(), next);
    EXPECT(seg.pairs == pairs);
    size_t nonempty = 0;
    for (int32_t c : counts) nonempty += c > 0;
    EXPECT(seg.select_ids[0].size() + seg.select_ids[1].size() == nonempty);
    for (int k = 0; k < 2; ++k) {
      EXPECT(std::is_sorted(seg.select_ids[k].begin(), seg.select_ids[k].end()));
      for (int32_t c : seg.select_ids[k]) EXPECT(counts[(size_t)c] > 0 && (counts[(size_t)c] > 64) == (k == 1));
    }
    std::vector<int64_t> row_offsets;
    std::vector<int32_t> other, count;
    std::vector<float> angle;
    mp::make_rows(counts.data(), angles.data(), I, &row_offsets, &other, &count, &angle);
    std::vector<std::map<int, std::pair<int, float>>> want((size_t)I);
    for (int a = 0; a < I; ++a)
      for (int b = a + 1; b < I; ++b) {
        const size_t c = (size_t)mp::cell_index(a, b, I);
        if (counts[c] > 0) want[(size_t)a][b] = want[(size_t)b][a] = {counts[c], angles[c]};
      }
    EXPECT(row_offsets.size() == (size_t)I + 1 && row_offsets[0] == 0);
    for (int i = 0; i < I; ++i) {
      int64_t e = row_offsets[(size_t)i];
      for (const auto& kv : want[(size_t)i]) {
        EXPECT(e < row_offsets[(size_t)i + 1] && other[(size_t)e] == kv.first && count[(size_t)e] == kv.second.first && angle[(size_t)e] == kv.second.second);
        ++e;
      }
      EXPECT(e == row_offsets[(size_t)i + 1]);
    }
    mp::make_rows(nullptr, nullptr, 1, &row_offsets, &other, &count, &angle);  // one image: no cell is read
    EXPECT(row_offsets.size() == 2 && row_offsets[1] == 0 && other.empty());
  }

  std::printf("model plan checks OK\n");
  return 0;
}
