// Prints the camera model table of include/colmap_amd/camera_models.hpp as JSON, for ids -1 .. kNumModels (the two
// ends are not models); tests/test_camera_models.py compares it with tests/golden/camera_models.json.
#include <cstdio>

#include "colmap_amd/camera_models.hpp"

namespace cm = colmap_amd::camera_models;

static void print_range(const char* key, int first, int count) {
  std::printf("\"%s\": [", key);
  for (int i = 0; i < count; ++i) std::printf("%s%d", i ? ", " : "", first + i);
  std::printf("]");
}

int main() {
  std::printf("{\"num_models\": %d, \"max_params\": %d, \"models\": [\n", cm::kNumModels, cm::kMaxParams);
  for (int m = -1; m <= cm::kNumModels; ++m) {
    const cm::ModelInfo* k = cm::model_info(m);
    std::printf("{\"id\": %d, \"num_params\": %d, ", m, cm::num_params(m));
    if (!k) {
      std::printf("\"name\": null");
    } else {
      std::printf("\"name\": \"%s\", ", k->name);
      std::printf("\"focal_length_idxs\": [");
      if (k->num_focal() >= 1) std::printf("%d", k->fx);
      if (k->num_focal() == 2) std::printf(", %d", k->fy);
      std::printf("], \"principal_point_idxs\": [");
      if (k->cx >= 0) std::printf("%d, %d", k->cx, k->cy);
      std::printf("], ");
      print_range("extra_params_idxs", k->first_extra, k->num_extra());
    }
    std::printf(", \"one_focal\": %s, \"is_fisheye\": %s, \"is_spherical\": %s, \"is_perspective\": %s}%s\n",
                cm::one_focal(m) ? "true" : "false", cm::is_fisheye(m) ? "true" : "false",
                cm::is_spherical(m) ? "true" : "false", cm::is_perspective(m) ? "true" : "false",
                m < cm::kNumModels ? "," : "");
  }
  std::printf("]}\n");
  return 0;
}
