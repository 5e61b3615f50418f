// colmap_amd/csrc/camera_projection.h compiled for the host alone, as a stand-alone program: reads cases from a text
// file (tests/test_camera_projection_cpp.py writes the cases of tests/camera_edge_cases.py), evaluates the header's
// functions at every point and prints the results with 17 significant digits, which round-trip a double.
//
//   input : per case one line  "<name> <kind: 0 inverse, 1 forward> <model id> <num params> <num points>", the parameters
//           on one line, then one point per line
//   output: per case one line  "<name> <num points>", then per point
//             ok a b          cam_from_img (kind 0) or img_from_normalized (kind 1); a = b = nan when !ok
//             du dv J0..J3    distortion() and its Jacobian at the point (kind 0: at the normalized pixel)
//             it_ok it_u it_v iterative_undistortion() from the normalized pixel (kind 0, iterative models; else 0 nan nan)
#define __host__
#define __device__
#define __forceinline__ inline
#include "camera_projection.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace {

bool is_iterative(int m) {
  using namespace camera;
  switch (m) {
    case SIMPLE_RADIAL: case RADIAL: case OPENCV: case OPENCV_FISHEYE: case FULL_OPENCV: case SIMPLE_RADIAL_FISHEYE:
    case RADIAL_FISHEYE: case THIN_PRISM_FISHEYE: case RAD_TAN_THIN_PRISM_FISHEYE:
      return true;
    default:
      return false;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  char name[128];
  int kind, model, num_params;
  long num_points;
  while (std::fscanf(in, "%127s %d %d %d %ld", name, &kind, &model, &num_params, &num_points) == 5) {
    if (model < 0 || model >= camera::kNumModels || num_params != camera::num_params(model) || num_points < 0) {
      std::fprintf(stderr, "%s: bad header\n", name);
      return 2;
    }
    std::vector<double> p(camera::kMaxParams, 0.0);
    for (int i = 0; i < num_params; ++i)
      if (std::fscanf(in, "%lf", &p[i]) != 1) return 2;
    std::printf("%s %ld\n", name, num_points);
    const camera::Intrinsics k = camera::intrinsics(model, p.data());
    for (long i = 0; i < num_points; ++i) {
      double x, y;
      if (std::fscanf(in, "%lf %lf", &x, &y) != 2) return 2;
      double a = nan, b = nan;
      const bool ok = kind == 0 ? camera::cam_from_img(model, p.data(), x, y, &a, &b)
                                : camera::img_from_normalized(model, p.data(), x, y, &a, &b);
      if (!ok) a = b = nan;
      const double u = kind == 0 ? (x - k.c1) / k.f1 : x, v = kind == 0 ? (y - k.c2) / k.f2 : y;
      double du, dv, J[4];
      camera::distortion(model, k.extra, u, v, &du, &dv, J);
      bool it_ok = false;
      double iu = nan, iv = nan;
      if (kind == 0 && is_iterative(model)) {
        iu = u;
        iv = v;
        it_ok = camera::iterative_undistortion(model, k.extra, &iu, &iv);
      }
      std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g %.17g\n", ok ? 1 : 0, a, b, du, dv, J[0], J[1],
                  J[2], J[3], it_ok ? 1 : 0, iu, iv);
    }
  }
  std::fclose(in);
  std::printf("camera projection dump OK\n");
  return 0;
}
