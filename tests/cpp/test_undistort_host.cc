// Host program of tests/test_undistort_cpp.py: include/colmap_amd/undistortion.hpp from g++.
//   test_undistort_host known            the known answers of the reference's UndistortCamera tests (no GPU needed)
//   test_undistort_host image OUT.txt    one UndistortImage + UndistortReconstruction on the GPU, results as text
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "colmap_amd/undistortion.hpp"

using namespace colmap_amd;

#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: EXPECT(%s)\n", __FILE__, __LINE__, #c); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static Camera SimpleRadial(double f, int w, int h, double k) {
  Camera c;
  c.model_id = 2;
  c.width = w;
  c.height = h;
  c.params = {f, w / 2.0, h / 2.0, k};
  return c;
}

static int Known() {  // image/undistortion_test.cc:78-179
  UndistortCameraOptions options;
  Camera u = UndistortCamera(options, SimpleRadial(1, 1, 1, 0));
  EXPECT(u.model_id == 1 && u.params[0] == 1 && u.params[1] == 1 && u.width == 1 && u.height == 1);
  const Camera cam = SimpleRadial(100, 100, 100, 0.5);
  u = UndistortCamera(options, cam);
  EXPECT(u.model_id == 1 && u.params[0] == 100 && u.params[1] == 100 && u.params[2] == 42.0 && u.params[3] == 42.0);
  EXPECT(u.width == 84 && u.height == 84);
  options.blank_pixels = 1;
  u = UndistortCamera(options, cam);
  EXPECT(u.width == 90 && u.height == 90 && u.params[2] == 45.0);
  options.max_scale = 0.75;
  u = UndistortCamera(options, cam);
  EXPECT(u.width == 75 && u.height == 75);
  options.max_scale = 1.0;
  options.roi_min_x = 0.1;
  options.roi_min_y = 0.2;
  options.roi_max_x = 0.9;
  options.roi_max_y = 0.8;
  u = UndistortCamera(options, cam);
  EXPECT(u.width == 80 && u.height == 60 && u.params[2] == 40 && u.params[3] == 30 && u.params[0] == 100);
  Camera fisheye;
  fisheye.model_id = 14;
  fisheye.width = 200;
  fisheye.height = 100;
  fisheye.params = {130, 10, 50};
  UndistortCameraOptions fo;
  fo.blank_pixels = 1.0;
  const Camera unbounded = UndistortCamera(fo, fisheye);
  EXPECT(unbounded.width == 400 && unbounded.height == 200);
  fo.max_cam_point_norm = 2.0;
  const Camera bounded = UndistortCamera(fo, fisheye);
  EXPECT(bounded.width < unbounded.width && bounded.height < unbounded.height);
  fo.max_cam_point_norm = 0;
  bool threw = false;
  try {
    UndistortCamera(fo, fisheye);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "max_cam_point_norm") != nullptr;
  }
  EXPECT(threw);
  EXPECT(!cam.IsUndistorted() && SimpleRadial(1, 1, 1, 0).IsUndistorted());
  std::printf("known OK\n");
  return 0;
}

static int Image(const char* out_path) {
  const Camera cam = SimpleRadial(100, 100, 100, 0.5);
  Bitmap in;
  in.width = in.height = 100;
  in.channels = 3;
  in.data.resize(100 * 100 * 3);
  for (int y = 0; y < 100; ++y)
    for (int x = 0; x < 100; ++x) {  // image/undistortion_test.cc:269-279
      in.data[(y * 100 + x) * 3 + 0] = static_cast<uint8_t>(x);
      in.data[(y * 100 + x) * 3 + 1] = static_cast<uint8_t>(y);
      in.data[(y * 100 + x) * 3 + 2] = static_cast<uint8_t>((x + y) / 2);
    }
  UndistortCameraOptions options;
  Bitmap out;
  Camera out_cam;
  UndistortImage(options, in, cam, &out, &out_cam);
  EXPECT(out_cam.model_id == 1 && out.width == 84 && out.height == 84 && out.channels == 3);
  EXPECT(out.data.size() == 84u * 84u * 3u);
  std::vector<Camera> cameras = {cam};
  std::vector<std::vector<double>> xy = {{10.0, 20.0, 50.0, 50.0, 90.5, 12.25}};
  UndistortReconstruction(options, &cameras, {0}, &xy);
  EXPECT(cameras[0].model_id == 1 && cameras[0].width == 84);
  std::FILE* f = std::fopen(out_path, "w");
  EXPECT(f != nullptr);
  std::fprintf(f, "%d %d %d\n", out.width, out.height, out.channels);
  for (size_t i = 0; i < out.data.size(); ++i) std::fprintf(f, "%d ", out.data[i]);
  std::fprintf(f, "\n");
  for (double v : xy[0]) std::fprintf(f, "%.17g ", v);
  std::fprintf(f, "\n");
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && std::string(argv[1]) == "known") return Known();
    if (argc >= 3 && std::string(argv[1]) == "image") return Image(argv[2]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 2;
  }
  std::fprintf(stderr, "usage: test_undistort_host known | image OUT.txt\n");
  return 64;
}
