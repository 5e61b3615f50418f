// camera.hpp -- colmap_amd::Camera (reference scene/camera.h), the one camera type of the C++ headers: bundle
// adjustment, image undistortion and observation filtering all take it. Header-only, standard library only.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "camera_models.hpp"

namespace colmap_amd {

struct Camera {
  // camera_id stands last so that Camera{model_id, width, height, {params...}} initialises what it names
  int model_id = CameraModelId::SIMPLE_RADIAL;
  int width = 0, height = 0;
  std::vector<double> params;
  uint32_t camera_id = 0;

  bool IsSpherical() const { return camera_models::is_spherical(model_id); }
  bool IsUndistorted() const {  // scene/camera.cc:98-111
    if (IsSpherical()) return true;
    const camera_models::ModelInfo* info = camera_models::model_info(model_id);
    if (!info) return false;  // not a model: nothing is known about its parameters
    for (size_t i = static_cast<size_t>(info->first_extra); i < params.size(); ++i)
      if (std::abs(params[i]) > 1e-8) return false;
    return true;
  }
};

}  // namespace colmap_amd
