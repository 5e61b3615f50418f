// The C++ surface of the model statistics (include/colmap_amd/model.hpp) from g++ against the C ABI.
//   test_model_host host      what needs no device: names, flattening, a rejected model
//   test_model_host known     the reference's own expectations (mvs/model_test.cc:82-190)
//   test_model_host nodevice  a statistic without a device
#include <cmath>
#include <cstdio>
#include <string>

#include "colmap_amd/model.hpp"

#define EXPECT(cond)                                                                 \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

using colmap_amd::mvs::Image;
using colmap_amd::mvs::Model;

static const float K[9] = {100, 0, 50, 0, 100, 50, 0, 0, 1};
static const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

static Model Cameras(int n) {  // projection centres (0, 0, 0), (1, 0, 0), (2, 0, 0): -R^T T = -T
  Model model;
  for (int i = 0; i < n; ++i) {
    const float T[3] = {-(float)i, 0, 0};
    model.AddImage("img" + std::to_string(i) + ".jpg", Image("img" + std::to_string(i) + ".jpg", 100, 100, K, R, T));
  }
  return model;
}

static int Host() {
  Model model = Cameras(3);
  EXPECT(model.GetImageIdx("img2.jpg") == 2 && model.GetImageName(1) == "img1.jpg");
  int thrown = 0;
  try { model.GetImageIdx("nonexistent"); } catch (const std::exception&) { ++thrown; }
  try { model.GetImageName(-1); } catch (const std::exception&) { ++thrown; }
  try { model.GetImageName(3); } catch (const std::exception&) { ++thrown; }
  EXPECT(thrown == 3);
  model.points.push_back({5.0f, 0.0f, 10.0f, {0, 1}});
  model.points.push_back({6.0f, 0.0f, 10.0f, {}});
  model.points.push_back({7.0f, 0.0f, 10.0f, {2, 1, 2}});
  const Model::Flat f(model);
  EXPECT(f.model.num_images == 3 && f.model.num_points == 3 && f.model.num_observations == 5);
  EXPECT(f.offsets.size() == 4 && f.offsets[1] == 2 && f.offsets[2] == 2 && f.offsets[3] == 5);
  EXPECT(f.track_image[2] == 2 && f.track_image[3] == 1 && f.T[3] == -1.0f && f.xyz[6] == 7.0f);
  // a model the library must reject before it touches a device
  model.points.push_back({0.0f, 0.0f, 1.0f, {0, 3}});
  try {
    model.ComputeSharedPoints();
    EXPECT(false);
  } catch (const std::runtime_error& e) {
    EXPECT(std::string(e.what()).find("image index 3 out of range") != std::string::npos);
  }
  std::printf("host OK\n");
  return 0;
}

static int Known() {
  {  // ComputeSharedPoints (:82-106)
    Model model = Cameras(3);
    model.points.push_back({5.0f, 0.0f, 10.0f, {0, 1}});
    model.points.push_back({6.0f, 0.0f, 10.0f, {0, 1, 2}});
    const auto shared = model.ComputeSharedPoints();
    EXPECT(shared.size() == 3 && shared[0].at(1) == 2 && shared[1].at(0) == 2 && shared[0].at(2) == 1);
    EXPECT(shared[2].at(0) == 1 && shared[1].at(2) == 1 && shared[2].at(1) == 1 && shared[0].count(0) == 0);
  }
  {  // ComputeDepthRanges, ComputeDepthRangesNoPoints (:108-143)
    Model model = Cameras(1);
    EXPECT(model.ComputeDepthRanges() == (std::vector<std::pair<float, float>>{{-1.0f, -1.0f}}));
    for (int i = 1; i <= 100; ++i) model.points.push_back({0.0f, 0.0f, (float)i, {0}});
    const auto ranges = model.ComputeDepthRanges();
    EXPECT(ranges.size() == 1 && ranges[0].first == 1.5f && ranges[0].second == 125.0f);
  }
  {  // ComputeTriangulationAngles (:145-166)
    Model model = Cameras(2);
    model.points.push_back({0.5f, 0.0f, 10.0f, {0, 1}});
    const auto angles = model.ComputeTriangulationAngles(50);
    EXPECT(angles.size() == 2 && std::fabs(angles[0].at(1) - 2.0f * std::atan(0.5f / 10.0f)) <= 1e-5f);
    EXPECT(angles[0].at(1) == angles[1].at(0));
  }
  {  // GetMaxOverlappingImages (:168-190)
    Model model = Cameras(3);
    for (int i = 0; i < 10; ++i) model.points.push_back({0.5f, 0.0f, 5.0f + i, {0, 1}});
    model.points.push_back({1.0f, 0.0f, 10.0f, {0, 2}});
    const auto overlapping = model.GetMaxOverlappingImages(2, 0.0);
    EXPECT(overlapping.size() == 3 && !overlapping[0].empty() && overlapping[0][0] == 1);
    EXPECT(overlapping[0] == (std::vector<int>{1, 2}) && overlapping[1] == (std::vector<int>{0}));
    EXPECT(model.GetMaxOverlappingImages(1, 0.0)[0] == (std::vector<int>{1}));
    EXPECT(model.GetMaxOverlappingImages(2, 89.0)[0].empty());
  }
  std::printf("known OK\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc > 1 && std::string(argv[1]) == "host") return Host();
    if (argc > 1 && std::string(argv[1]) == "known") return Known();
    if (argc > 1 && std::string(argv[1]) == "nodevice") {
      Model model = Cameras(2);
      model.points.push_back({0.5f, 0.0f, 10.0f, {0, 1}});
      model.ComputeDepthRanges();
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  std::fprintf(stderr, "usage: test_model_host host|known|nodevice\n");
  return 1;
}
