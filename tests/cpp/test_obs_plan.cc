// The host plan of observation filtering (colmap_amd/csrc/obs_plan.h) against brute-force code of its own: input
// validation on exactly sized heap arrays (a read through a bad index before its check shows under the sanitizers), the
// model-sorted order of the per-observation pass, the lane-group classes and the count reduction. g++ alone, no HIP.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "obs_plan.h"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

namespace {

struct Model {  // owns exactly sized arrays
  std::unique_ptr<obs_camera[]> cameras;
  std::unique_ptr<double[]> poses, points, xy;
  std::unique_ptr<int32_t[]> image_camera, obs_image;
  std::unique_ptr<int64_t[]> offsets;
  obs_model m{};
};

Model make(int num_cameras, int num_images, const std::vector<int>& lengths, std::mt19937& rng) {
  Model s;
  const int params[18] = {3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12, 16, 4, 5, 3, 4, 6, 2};
  s.cameras.reset(new obs_camera[num_cameras]());
  for (int c = 0; c < num_cameras; ++c) {
    s.cameras[c].model_id = (int)(rng() % 18);
    s.cameras[c].num_params = params[s.cameras[c].model_id];
    s.cameras[c].width = 100;
    s.cameras[c].height = 50;
  }
  s.poses.reset(new double[7 * num_images]());
  s.image_camera.reset(new int32_t[num_images]);
  for (int i = 0; i < num_images; ++i) s.image_camera[i] = (int32_t)(rng() % num_cameras);
  const size_t P = lengths.size();
  s.points.reset(new double[3 * P]());
  s.offsets.reset(new int64_t[P + 1]);
  s.offsets[0] = 0;
  for (size_t p = 0; p < P; ++p) s.offsets[p + 1] = s.offsets[p] + lengths[p];
  const int64_t O = s.offsets[P];
  s.obs_image.reset(new int32_t[O]);
  s.xy.reset(new double[2 * O]());
  for (int64_t o = 0; o < O; ++o) s.obs_image[o] = (int32_t)(rng() % num_images);
  s.m.num_cameras = num_cameras;
  s.m.num_images = num_images;
  s.m.num_points = (int64_t)P;
  s.m.num_observations = O;
  s.m.cameras = s.cameras.get();
  s.m.image_poses = s.poses.get();
  s.m.image_camera = s.image_camera.get();
  s.m.points = s.points.get();
  s.m.obs_offsets = s.offsets.get();
  s.m.obs_image = s.obs_image.get();
  s.m.obs_xy = s.xy.get();
  return s;
}

bool rejected(const obs_model& m, const char* what) {
  try {
    obs_plan::validate(m);
  } catch (const obs_plan::Fail& e) {
    if (std::string(e.what()).find(what) == std::string::npos) {
      std::fprintf(stderr, "rejected with \"%s\", expected \"%s\"\n", e.what(), what);
      return false;
    }
    return true;
  }
  std::fprintf(stderr, "accepted, expected \"%s\"\n", what);
  return false;
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  const std::vector<int> lengths = {0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 200, 5, 0, 33};
  Model s = make(5, 40, lengths, rng);
  obs_plan::validate(s.m);

  // ---- validation: each defect alone, on the exactly sized arrays
  { Model b = make(5, 40, lengths, rng); b.offsets[0] = 1; EXPECT(rejected(b.m, "start at 0")); }
  { Model b = make(5, 40, lengths, rng); b.offsets[6] = b.offsets[5] - 1; EXPECT(rejected(b.m, "decreases")); }
  { Model b = make(5, 40, lengths, rng); b.offsets[lengths.size()] += 1000000; EXPECT(rejected(b.m, "end at num_observations")); }
  { Model b = make(5, 40, lengths, rng); b.m.num_observations += 7; EXPECT(rejected(b.m, "end at num_observations")); }
  { Model b = make(5, 40, lengths, rng); b.obs_image[3] = 40; EXPECT(rejected(b.m, "image index 40 out of range")); }
  { Model b = make(5, 40, lengths, rng); b.obs_image[b.m.num_observations - 1] = -1; EXPECT(rejected(b.m, "image index -1")); }
  { Model b = make(5, 40, lengths, rng); b.image_camera[39] = 5; EXPECT(rejected(b.m, "camera index 5 out of range")); }
  { Model b = make(5, 40, lengths, rng); b.cameras[2].model_id = 18; EXPECT(rejected(b.m, "unknown camera model id 18")); }
  { Model b = make(5, 40, lengths, rng); b.cameras[2].model_id = -1; EXPECT(rejected(b.m, "unknown camera model")); }
  { Model b = make(5, 40, lengths, rng); b.cameras[4].num_params += 1; EXPECT(rejected(b.m, "parameters, got")); }
  { Model b = make(5, 40, lengths, rng); b.cameras[0].width = 0; EXPECT(rejected(b.m, "width and height")); }
  { Model b = make(5, 40, lengths, rng); b.m.num_points = -1; EXPECT(rejected(b.m, "negative")); }
  { Model b = make(5, 40, lengths, rng); b.m.num_observations = (int64_t)1 << 31; EXPECT(rejected(b.m, "32-bit")); }
  { Model b = make(5, 40, lengths, rng); b.m.num_points = (int64_t)1 << 31; EXPECT(rejected(b.m, "32-bit")); }
  { Model b = make(5, 40, lengths, rng); b.m.obs_offsets = nullptr; EXPECT(rejected(b.m, "obs_offsets is null")); }
  { Model b = make(5, 40, lengths, rng); b.m.obs_xy = nullptr; EXPECT(rejected(b.m, "observation arrays are null")); }
  { Model b = make(5, 40, lengths, rng); b.m.points = nullptr; EXPECT(rejected(b.m, "points is null")); }
  {  // the empty model is a model
    const int64_t zero = 0;
    obs_model e{};
    e.obs_offsets = &zero;
    obs_plan::validate(e);
    const obs_plan::Plan plan = obs_plan::make_plan(e, true);
    EXPECT(plan.obs_point.empty() && plan.eval_order.empty());
    for (int k = 0; k < obs_plan::kNumClasses; ++k) EXPECT(plan.class_points[k].empty());
  }

  // ---- the plan against brute force, on several random models
  for (int round = 0; round < 20; ++round) {
    std::vector<int> len(1 + rng() % 300);
    for (int& l : len) l = (rng() % 8 == 0) ? (int)(rng() % 140) : (int)(rng() % 12);
    Model t = make(1 + (int)(rng() % 20), 1 + (int)(rng() % 50), len, rng);
    obs_plan::validate(t.m);
    const obs_plan::Plan plan = obs_plan::make_plan(t.m, true);
    const int64_t O = t.m.num_observations;
    EXPECT((int64_t)plan.obs_point.size() == O && (int64_t)plan.eval_order.size() == O);
    for (int64_t o = 0; o < O; ++o) {  // the point of an observation: the one whose range holds it
      int64_t p = 0;
      while (!(t.offsets[p] <= o && o < t.offsets[p + 1])) ++p;
      EXPECT(plan.obs_point[o] == p);
    }
    auto model_of = [&](int32_t o) { return t.cameras[t.image_camera[t.obs_image[o]]].model_id; };
    std::vector<char> seen(O, 0);
    for (int64_t k = 0; k < O; ++k) {  // a permutation, sorted by model, stable within a model
      const int32_t o = plan.eval_order[k];
      EXPECT(o >= 0 && o < O && !seen[o]);
      seen[o] = 1;
      if (k > 0) {
        const int32_t prev = plan.eval_order[k - 1];
        EXPECT(model_of(prev) < model_of(o) || (model_of(prev) == model_of(o) && prev < o));
      }
    }
    size_t total = 0;
    for (int k = 0; k < obs_plan::kNumClasses; ++k) {
      total += plan.class_points[k].size();
      for (size_t i = 0; i < plan.class_points[k].size(); ++i) {
        const int32_t p = plan.class_points[k][i];
        const int64_t L = t.offsets[p + 1] - t.offsets[p];
        const int want = L <= 16 ? 0 : L <= 64 ? 1 : 2;
        EXPECT(k == want);
        EXPECT(i == 0 || plan.class_points[k][i - 1] < p);
      }
    }
    EXPECT(total == len.size());
    EXPECT(obs_plan::make_plan(t.m, false).eval_order.empty());
  }
  EXPECT(obs_plan::length_class(16) == 0 && obs_plan::length_class(17) == 1 && obs_plan::length_class(64) == 1 &&
         obs_plan::length_class(65) == 2 && obs_plan::length_class(0) == 0);
  EXPECT(obs_plan::kClassWidth[0] == 1 && obs_plan::kClassWidth[1] == 16 && obs_plan::kClassWidth[2] == 64);

  // ---- the count reduction: 64-bit, beyond what 32 bits hold
  std::vector<uint32_t> counts(5, 0xffffffffu);
  EXPECT(obs_plan::sum_counts(counts.data(), 5) == 5ll * 0xffffffffll);
  EXPECT(obs_plan::sum_counts(nullptr, 0) == 0);
  std::printf("obs plan checks OK\n");
  return 0;
}
