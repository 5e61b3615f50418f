// camera_models.hpp -- the camera models, once, for device code, host code and the C++ API: ids, names, parameter
// counts, which parameters are focal length / principal point / extra, and the families (reference sensor/models.h).
// The functions are host/device when the HIP header (or its CPU stand-in) came first and plain inline otherwise.
// An id outside 0 .. kNumModels - 1 is not a model: model_info() gives null and num_params() gives -1.
#pragma once

#if defined(__device__) && defined(__host__)
#define COLMAP_AMD_MODELS_HD __host__ __device__ __forceinline__
#else
#define COLMAP_AMD_MODELS_HD inline
#endif

namespace colmap_amd {
namespace camera_models {

// colmap::CameraModelId (sensor/models.h:90-111)
enum CameraModelId : int {
  SIMPLE_PINHOLE = 0, PINHOLE = 1, SIMPLE_RADIAL = 2, RADIAL = 3, OPENCV = 4, OPENCV_FISHEYE = 5, FULL_OPENCV = 6,
  FOV = 7, SIMPLE_RADIAL_FISHEYE = 8, RADIAL_FISHEYE = 9, THIN_PRISM_FISHEYE = 10, RAD_TAN_THIN_PRISM_FISHEYE = 11,
  SIMPLE_DIVISION = 12, DIVISION = 13, SIMPLE_FISHEYE = 14, FISHEYE = 15, EUCM = 16, EQUIRECTANGULAR = 17
};
constexpr int kNumModels = 18;
constexpr int kMaxParams = 16;

// The parameters of a model are (f | fx fy) cx cy extra..., except EQUIRECTANGULAR's (width, height), which are
// metadata: no focal length, no principal point, nothing to refine (MetaDataParamsIdxs, models.h:2839-2842).
struct ModelInfo {
  const char* name;
  int num_params;
  int fx, fy, cx, cy;  // parameter indices; fx == fy: one shared focal length; -1: the model has none
  int first_extra;     // the extra parameters are first_extra .. num_params - 1
  constexpr int num_focal() const { return fx < 0 ? 0 : (fx == fy ? 1 : 2); }
  constexpr int num_extra() const { return num_params - first_extra; }
};

constexpr ModelInfo kModels[kNumModels] = {
    {"SIMPLE_PINHOLE", 3, 0, 0, 1, 2, 3},
    {"PINHOLE", 4, 0, 1, 2, 3, 4},
    {"SIMPLE_RADIAL", 4, 0, 0, 1, 2, 3},
    {"RADIAL", 5, 0, 0, 1, 2, 3},
    {"OPENCV", 8, 0, 1, 2, 3, 4},
    {"OPENCV_FISHEYE", 8, 0, 1, 2, 3, 4},
    {"FULL_OPENCV", 12, 0, 1, 2, 3, 4},
    {"FOV", 5, 0, 1, 2, 3, 4},
    {"SIMPLE_RADIAL_FISHEYE", 4, 0, 0, 1, 2, 3},
    {"RADIAL_FISHEYE", 5, 0, 0, 1, 2, 3},
    {"THIN_PRISM_FISHEYE", 12, 0, 1, 2, 3, 4},
    {"RAD_TAN_THIN_PRISM_FISHEYE", 16, 0, 1, 2, 3, 4},
    {"SIMPLE_DIVISION", 4, 0, 0, 1, 2, 3},
    {"DIVISION", 5, 0, 1, 2, 3, 4},
    {"SIMPLE_FISHEYE", 3, 0, 0, 1, 2, 3},
    {"FISHEYE", 4, 0, 1, 2, 3, 4},
    {"EUCM", 6, 0, 1, 2, 3, 4},
    {"EQUIRECTANGULAR", 2, -1, -1, -1, -1, 2},
};

COLMAP_AMD_MODELS_HD constexpr const ModelInfo* model_info(int m) { return m >= 0 && m < kNumModels ? &kModels[m] : nullptr; }
COLMAP_AMD_MODELS_HD constexpr int num_params(int m) { return m >= 0 && m < kNumModels ? kModels[m].num_params : -1; }

// one shared focal length (f, cx, cy, extra...) or two (fx, fy, cx, cy, extra...)
COLMAP_AMD_MODELS_HD constexpr bool one_focal(int m) {
  return m == SIMPLE_PINHOLE || m == SIMPLE_RADIAL || m == RADIAL || m == SIMPLE_RADIAL_FISHEYE || m == RADIAL_FISHEYE ||
         m == SIMPLE_DIVISION || m == SIMPLE_FISHEYE;
}
COLMAP_AMD_MODELS_HD constexpr bool is_spherical(int m) { return m == EQUIRECTANGULAR; }
COLMAP_AMD_MODELS_HD constexpr bool is_perspective(int m) { return m >= 0 && m < EQUIRECTANGULAR; }
// BasePerspectiveFisheyeCameraModel (models.h:425-456)
COLMAP_AMD_MODELS_HD constexpr bool is_fisheye(int m) {
  return m == OPENCV_FISHEYE || m == SIMPLE_RADIAL_FISHEYE || m == RADIAL_FISHEYE || m == THIN_PRISM_FISHEYE ||
         m == RAD_TAN_THIN_PRISM_FISHEYE || m == SIMPLE_FISHEYE || m == FISHEYE;
}

struct Intrinsics {
  double f1, f2, c1, c2;
  const double* extra;
};
COLMAP_AMD_MODELS_HD Intrinsics intrinsics(int m, const double* p) {
  if (one_focal(m)) return Intrinsics{p[0], p[0], p[1], p[2], p + 3};
  return Intrinsics{p[0], p[1], p[2], p[3], p + 4};
}

}  // namespace camera_models

using camera_models::CameraModelId;

}  // namespace colmap_amd
#undef COLMAP_AMD_MODELS_HD
