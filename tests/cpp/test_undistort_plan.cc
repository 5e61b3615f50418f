// The host plan of image undistortion (colmap_amd/csrc/undistort_plan.h) without a GPU: UndistortCamera and
// RectifyStereoCameras against the known answers of the reference's tests, the route of an image, the mid camera and the
// conjugated homography of the indirect route, sizes and grids, and every refusal with its message. Stand-alone: g++
// alone, also under -fsanitize=address,undefined (tests/test_undistort_plan.py) -- the arrays are exactly sized on the
// heap. Every expected value is a literal: the reference's own, or exact by construction.
#define __host__
#define __device__
#define __forceinline__ inline
#include "undistort_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace up = undistort_plan;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// f throws a Fail whose message is exactly `message`
template <typename F>
static bool fails(F&& f, const std::string& message) {
  try {
    f();
  } catch (const up::Fail& e) {
    if (message == e.what()) return true;
    std::fprintf(stderr, "expected \"%s\", got \"%s\"\n", message.c_str(), e.what());
  }
  return false;
}

static undistort_options defaults() {
  undistort_options o;
  up::options_init(&o);
  return o;
}

static undistort_cam make_cam(int model, int w, int h, std::initializer_list<double> params) {
  undistort_cam c = {};
  c.model_id = model;
  c.width = w;
  c.height = h;
  int i = 0;
  for (double p : params) c.params[i++] = p;
  return c;
}

static undistort_cam simple_radial(double f, int w, int h, double k) {
  return make_cam(camera::SIMPLE_RADIAL, w, h, {f, w / 2.0, h / 2.0, k});
}

static undistort_cam undistorted(const undistort_options& o, const undistort_cam& c) {
  undistort_cam u;
  up::undistort_camera_impl(o, c, &u);
  return u;
}

static bool params_are(const undistort_cam& c, std::initializer_list<double> params) {
  int i = 0;
  for (double p : params)
    if (c.params[i++] != p) return false;
  return true;
}

static bool equal9(const double* a, std::initializer_list<double> b) { return std::equal(b.begin(), b.end(), a); }

// an image of the camera with exactly sized heap buffers (a plan never reads them)
struct Image {
  std::unique_ptr<uint8_t[]> data, out;
  undistort_image im = {};
  Image(const undistort_cam& cam, int channels, size_t out_bytes)
      : data(new uint8_t[(size_t)cam.width * cam.height * channels]()), out(new uint8_t[out_bytes]()) {
    im.camera = cam;
    im.data = data.get();
    im.channels = channels;
    im.out = out.get();
    im.out_capacity = out_bytes;
  }
};

static void test_undistort_camera() {  // image/undistortion_test.cc:78-179
  undistort_options o = defaults();
  undistort_cam u = undistorted(o, simple_radial(1, 1, 1, 0));
  EXPECT(u.model_id == camera::PINHOLE && u.width == 1 && u.height == 1 && u.params[0] == 1 && u.params[1] == 1);
  const undistort_cam cam = simple_radial(100, 100, 100, 0.5);
  u = undistorted(o, cam);
  EXPECT(u.model_id == camera::PINHOLE && u.width == 84 && u.height == 84 && params_are(u, {100, 100, 42, 42}));
  o.blank_pixels = 1;
  u = undistorted(o, cam);
  EXPECT(u.width == 90 && u.height == 90 && params_are(u, {100, 100, 45, 45}));
  o.max_scale = 0.75;
  u = undistorted(o, cam);
  EXPECT(u.width == 75 && u.height == 75);
  o.max_scale = 1.0;
  o.roi_min_x = 0.1;
  o.roi_min_y = 0.2;
  o.roi_max_x = 0.9;
  o.roi_max_y = 0.8;
  u = undistorted(o, cam);
  EXPECT(u.width == 80 && u.height == 60 && params_are(u, {100, 100, 40, 30}));
  const undistort_cam fisheye = make_cam(camera::SIMPLE_FISHEYE, 200, 100, {130, 10, 50});
  undistort_options fo = defaults();
  fo.blank_pixels = 1.0;
  const undistort_cam unbounded = undistorted(fo, fisheye);
  EXPECT(unbounded.width == 400 && unbounded.height == 200);
  fo.max_cam_point_norm = 2.0;
  const undistort_cam bounded = undistorted(fo, fisheye);
  EXPECT(bounded.width < unbounded.width && bounded.height < unbounded.height);
  fo.max_cam_point_norm = 0;
  EXPECT(fails([&] { undistorted(fo, fisheye); }, "Check failed: options.max_cam_point_norm != 0"));
  // a failed call leaves its output alone
  undistort_cam untouched = make_cam(7, 7, 7, {7});
  EXPECT(fails([&] { up::undistort_camera_impl(fo, fisheye, &untouched); }, "Check failed: options.max_cam_point_norm != 0"));
  EXPECT(untouched.model_id == 7 && untouched.width == 7 && untouched.params[0] == 7);
  EXPECT(fails([&] { undistorted(defaults(), make_cam(camera::EQUIRECTANGULAR, 500, 250, {500, 250})); },
               "Check failed: camera.IsPerspective()"));
  EXPECT(fails([&] { undistorted(defaults(), make_cam(99, 10, 10, {})); }, "unknown camera model id 99"));
  EXPECT(fails([&] { undistorted(defaults(), make_cam(camera::PINHOLE, 0, 10, {1, 1, 0, 0})); },
               "camera width and height must be positive"));
}

static void test_cam_from_img() {
  const undistort_cam cam = make_cam(camera::PINHOLE, 4, 8, {2, 4, 1, 1});
  std::unique_ptr<double[]> xy(new double[4]{3, 5, 1, 1}), uv(new double[4]);
  up::cam_from_img(cam, xy.get(), 2, uv.get());
  EXPECT(uv[0] == 1 && uv[1] == 1 && uv[2] == 0 && uv[3] == 0);
  up::cam_from_img(cam, nullptr, 0, nullptr);
  EXPECT(fails([&] { up::cam_from_img(make_cam(-1, 4, 8, {}), xy.get(), 2, uv.get()); }, "unknown camera model id -1"));
}

static void test_rectify_cameras() {
  // image/undistortion_test.cc:482-513, which prints the matrices transposed; cam2_from_cam1 = Rz(0.3) Ry(0.2) Rx(0.1)
  const double cx = std::cos(0.1), sx = std::sin(0.1), cy = std::cos(0.2), sy = std::sin(0.2), cz = std::cos(0.3),
               sz = std::sin(0.3);
  const double R[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                       sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                       -sy,     cy * sx,                cy * cx};
  const double t[3] = {0.1, 0.2, 0.3};
  const undistort_cam unit = make_cam(camera::PINHOLE, 1, 1, {1, 1, 0.5, 0.5});
  std::unique_ptr<double[]> H1(new double[9]), H2(new double[9]), Q(new double[16]);
  up::rectify_cameras_impl(unit, unit, R, t, H1.get(), H2.get(), Q.get());
  const double H1_t[9] = {-0.202759, -0.815848, -0.897034, 0.416329, 0.733069, -0.199657, 0.910839, -0.175408, 0.942638};
  const double H2_t[9] = {-0.082173, -1.01288, -0.698868, 0.301854, 0.472844, -0.465336, 0.963533, 0.292411, 1.12528};
  const double Q_ref[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2.67261, -0.5, -0.5, 1, 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      EXPECT(std::fabs(H1[3 * i + j] - H1_t[3 * j + i]) <= 1e-5);
      EXPECT(std::fabs(H2[3 * i + j] - H2_t[3 * j + i]) <= 1e-5);
    }
  for (int i = 0; i < 16; ++i) EXPECT(std::fabs(Q[i] - Q_ref[i]) <= 1e-5);

  // A baseline along x needs no rotation: H = K K_i^-1 with K = (min mean focal, cx of camera 1, mean cy). Dyadic
  // intrinsics make every product exact: K = (512, 512, 320, 236).
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const undistort_cam cam1 = make_cam(camera::PINHOLE, 640, 480, {512, 512, 320, 240});
  const undistort_cam cam2 = make_cam(camera::SIMPLE_PINHOLE, 640, 480, {1024, 336, 232});
  for (double tx : {1.0, -1.0}) {  // -x takes the flipped unit vector (image/undistortion.cc:405-408): still no rotation
    const double along_x[3] = {tx, 0, 0};
    up::rectify_cameras_impl(cam1, cam2, I, along_x, H1.get(), H2.get(), Q.get());
    EXPECT(equal9(H1.get(), {1, 0, 0, 0, 1, -4, 0, 0, 1}));
    EXPECT(equal9(H2.get(), {0.5, 0, 152, 0, 0.5, 120, 0, 0, 1}));
    const double Q_x[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -tx, -236, -320, 512, 0};
    for (int i = 0; i < 16; ++i) EXPECT(Q[i] == Q_x[i]);
  }

  const undistort_cam radial = simple_radial(500, 640, 480, 0.1);
  const double along_x[3] = {1, 0, 0};
  EXPECT(fails([&] { up::rectify_cameras_impl(radial, cam1, I, along_x, H1.get(), H2.get(), Q.get()); },
               "Check failed: camera1.model_id == SimplePinholeCameraModel::model_id || camera1.model_id == "
               "PinholeCameraModel::model_id"));
  EXPECT(fails([&] { up::rectify_cameras_impl(cam1, radial, I, along_x, H1.get(), H2.get(), Q.get()); },
               "Check failed: camera2.model_id == SimplePinholeCameraModel::model_id || camera2.model_id == "
               "PinholeCameraModel::model_id"));
  const undistort_cam flat = make_cam(camera::PINHOLE, 640, 480, {0, 512, 320, 240});
  EXPECT(fails([&] { up::rectify_cameras_impl(cam1, flat, I, along_x, H1.get(), H2.get(), Q.get()); },
               "a calibration matrix is singular"));
  EXPECT(Q[11] == 1 && Q[14] == 512);  // of the last good call: a refused one writes nothing
}

static void test_routes() {
  undistort_options o = defaults();
  const undistort_cam src = make_cam(camera::PINHOLE, 100, 100, {100, 100, 50, 50});
  up::PairPlan pp = {};
  const Image im(src, 1, 100 * 100);
  auto side_route = [&](int w, int h) {
    pp.target = make_cam(camera::PINHOLE, w, h, {100, 100, 50, 50});
    return up::plan_pair_side(o, pp, im.im, 0).route;
  };
  EXPECT(side_route(50, 100) == up::kDirect);  // 0.5 >= 0.5
  EXPECT(side_route(49, 100) == up::kIndirect);
  EXPECT(side_route(100, 49) == up::kIndirect);
  o.direct_warp_min_scale = 3;
  EXPECT(side_route(100, 100) == up::kDirect);  // equal sizes warp directly whatever the bound
  EXPECT(side_route(200, 200) == up::kIndirect);
  o.direct_warp_min_scale = -1;
  EXPECT(fails([&] { side_route(100, 100); }, "Check failed: options.direct_warp_min_scale >= 0"));
  EXPECT(fails([&] { up::plan_image(o, im.im, 0); }, "Check failed: options.direct_warp_min_scale >= 0"));

  // the same through plan_image: a PINHOLE camera is only rescaled to max_image_size
  o = defaults();
  o.max_image_size = 50;
  up::ImagePlan p = up::plan_image(o, im.im, 0);
  EXPECT(p.route == up::kDirect && p.target.width == 50 && p.target.height == 50 && params_are(p.target, {50, 50, 25, 25}));
  EXPECT(!p.has_homography && p.channels == 1 && p.interpolation == UNDISTORT_BILINEAR && p.in_bytes == 10000);
  o.max_image_size = 49;
  p = up::plan_image(o, im.im, 0);
  EXPECT(p.route == up::kIndirect && p.target.width == 49 && p.target.height == 49);
  EXPECT(p.mid.model_id == camera::PINHOLE && p.mid.width == 100 && p.mid.height == 100 && p.mid_words == 25 * 100);

  // spherical images: clone or resize, and direct_warp_min_scale is never looked at
  const undistort_cam sphere = make_cam(camera::EQUIRECTANGULAR, 200, 100, {200, 100});
  const Image pano(sphere, 3, 200 * 100 * 3);
  o = defaults();
  o.direct_warp_min_scale = -1;
  p = up::plan_image(o, pano.im, 0);
  EXPECT(p.route == up::kClone && p.in_bytes == 60000 && p.target.model_id == camera::EQUIRECTANGULAR);
  EXPECT(p.target.width == 200 && p.target.height == 100 && params_are(p.target, {200, 100}));
  o.max_image_size = 50;
  p = up::plan_image(o, pano.im, 0);
  EXPECT(p.route == up::kResize && p.target.model_id == camera::EQUIRECTANGULAR && p.target.width == 50 &&
         p.target.height == 25 && params_are(p.target, {50, 25}));
  EXPECT(p.out_words == 39 * 25 && p.grid.x == 1 && p.grid.y == 7 && p.mid_words == 0);
}

static void test_mid_camera_and_conjugation() {
  const undistort_cam tgt = make_cam(camera::PINHOLE, 64, 16, {30, 31, 20, 9});
  const undistort_cam src = make_cam(camera::OPENCV, 128, 64, {100, 100, 64, 32, 0.1, 0, 0, 0});
  const double Hinv[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  up::ImagePlan p = up::make_plan(up::kIndirect, src, tgt, 3, UNDISTORT_NEAREST, Hinv);  // sx = 2, sy = 4
  EXPECT(p.mid.model_id == camera::PINHOLE && p.mid.width == 128 && p.mid.height == 64);
  EXPECT(params_are(p.mid, {60, 124, 40, 36}));
  EXPECT(p.has_homography && equal9(p.hinv, {1, 1, 6, 8, 5, 24, 3.5, 2, 9}));
  EXPECT(p.in_bytes == 128 * 64 * 3 && p.out_words == 48 * 16 && p.mid_words == 96 * 64);
  EXPECT(p.grid.x == 1 && p.grid.y == 4 && p.mid_grid.x == 1 && p.mid_grid.y == 16);
  EXPECT(p.interpolation == UNDISTORT_NEAREST && p.channels == 3 && params_are(p.target, {30, 31, 20, 9}));
  p = up::make_plan(up::kDirect, src, tgt, 3, UNDISTORT_NEAREST, Hinv);  // in front of the target camera: as given
  EXPECT(p.has_homography && equal9(p.hinv, {1, 2, 3, 4, 5, 6, 7, 8, 9}) && p.mid_words == 0);
  p = up::make_plan(up::kIndirect, src, tgt, 1, UNDISTORT_BILINEAR, nullptr);
  EXPECT(!p.has_homography && params_are(p.mid, {60, 124, 40, 36}) && p.mid_words == 32 * 64);
}

static void test_sizes_and_grids() {
  EXPECT(up::padded_pitch(61, 3) == 192 && up::padded_pitch(64, 1) == 64 && up::padded_pitch(1, 3) == 12);
  const undistort_cam c = make_cam(camera::PINHOLE, 61, 47, {80, 81, 30, 23});
  EXPECT(up::make_plan(up::kDirect, c, c, 3, UNDISTORT_BILINEAR, nullptr).out_words == 48 * 47);
  EXPECT(up::image_grid(257, 5).x == 2 && up::image_grid(257, 5).y == 2);
  EXPECT(up::image_grid(256, 4).x == 1 && up::image_grid(256, 4).y == 1);
  EXPECT(up::image_grid(1, 1).x == 1 && up::image_grid(1, 1).y == 1);
  EXPECT(up::kBlockX == 64 && up::kBlockY == 4 && up::kPixelsPerLane == 4);
}

static void test_option_refusals() {  // image/undistortion.cc:60-70, each with the reference's wording
  const undistort_cam cam = simple_radial(100, 100, 100, 0.5);
  struct Case {
    void (*set)(undistort_options*);
    const char* message;
  };
  const Case cases[] = {
      {[](undistort_options* o) { o->blank_pixels = -0.1; }, "Check failed: options.blank_pixels >= 0"},
      {[](undistort_options* o) { o->blank_pixels = 1.1; }, "Check failed: options.blank_pixels <= 1"},
      {[](undistort_options* o) { o->min_scale = 0.0; }, "Check failed: options.min_scale > 0.0"},
      {[](undistort_options* o) { o->min_scale = 3.0; }, "Check failed: options.min_scale <= options.max_scale"},
      {[](undistort_options* o) { o->max_image_size = 0; }, "Check failed: options.max_image_size != 0"},
      {[](undistort_options* o) { o->roi_min_x = -0.1; }, "Check failed: options.roi_min_x >= 0.0"},
      {[](undistort_options* o) { o->roi_min_y = -0.1; }, "Check failed: options.roi_min_y >= 0.0"},
      {[](undistort_options* o) { o->roi_max_x = 1.1; }, "Check failed: options.roi_max_x <= 1.0"},
      {[](undistort_options* o) { o->roi_max_y = 1.1; }, "Check failed: options.roi_max_y <= 1.0"},
      {[](undistort_options* o) { o->roi_min_x = 0.6, o->roi_max_x = 0.5; }, "Check failed: options.roi_min_x < options.roi_max_x"},
      {[](undistort_options* o) { o->roi_min_y = 0.6, o->roi_max_y = 0.6; }, "Check failed: options.roi_min_y < options.roi_max_y"},
  };
  for (const Case& c : cases) {
    undistort_options o = defaults();
    c.set(&o);
    EXPECT(fails([&] { undistorted(o, cam); }, c.message));
    EXPECT(fails([&] { up::check_batch(&o, 0, nullptr); }, c.message));
  }
  undistort_options o = defaults();
  up::check_batch(&o, 0, nullptr);
  EXPECT(fails([&] { up::check_batch(nullptr, 0, nullptr); }, "null argument"));
  EXPECT(fails([&] { up::check_batch(&o, 1, nullptr); }, "null argument"));
  EXPECT(fails([&] { up::check_batch(&o, -1, &o); }, "null argument"));
  o.interpolation = 7;
  EXPECT(fails([&] { up::check_batch(&o, 0, nullptr); }, "Invalid warp image interpolation mode: 7"));
}

// plans a batch the way undistort_images does: image after image, stopping at the first refusal
static void plan_batch(const undistort_options& o, const undistort_image* images, int n) {
  for (int i = 0; i < n; ++i) up::plan_image(o, images[i], i);
}

static void test_image_refusals() {
  // Image 1 is wrong in the way under test, image 2 in another: the message names image 1, so image 2 was not examined.
  const undistort_options o = defaults();
  const undistort_cam cam = make_cam(camera::PINHOLE, 10, 10, {8, 8, 4, 4});  // its target is itself: 100 bytes of grey
  const Image good(cam, 1, 100);
  std::unique_ptr<undistort_image[]> batch(new undistort_image[3]);
  auto reset = [&] {
    batch[0] = batch[1] = batch[2] = good.im;
    batch[2].camera.model_id = 99;
  };
  reset();
  EXPECT(fails([&] { plan_batch(o, batch.get(), 3); }, "unknown camera model id 99"));
  batch[1].data = nullptr;
  EXPECT(fails([&] { plan_batch(o, batch.get(), 3); }, "image 1: null pixel buffer"));
  reset();
  batch[1].out = nullptr;
  EXPECT(fails([&] { plan_batch(o, batch.get(), 3); }, "image 1: null pixel buffer"));
  reset();
  batch[1].channels = 2;
  EXPECT(fails([&] { plan_batch(o, batch.get(), 3); }, "image 1: channels must be 1 (grey) or 3 (RGB)"));
  reset();
  batch[1].out_capacity = 99;
  EXPECT(fails([&] { plan_batch(o, batch.get(), 3); }, "image 1: output buffer of 99 bytes, 100 needed"));
  reset();
  plan_batch(o, batch.get(), 2);  // and the first two are fine as they stand

  // the same for pairs: the second image of pair 1 is spherical, pair 2 has an unknown model
  std::unique_ptr<undistort_stereo_pair[]> pairs(new undistort_stereo_pair[3]());
  auto reset_pairs = [&] {
    for (int i = 0; i < 3; ++i) {
      pairs[i].image1 = pairs[i].image2 = good.im;
      for (int k = 0; k < 9; ++k) pairs[i].R[k] = k % 4 == 0;
      pairs[i].t[0] = 1;
    }
    pairs[2].image1.camera.model_id = 99;
  };
  auto plan_pairs = [&](int n) {
    for (int i = 0; i < n; ++i) up::plan_pair(o, pairs[i], i);
  };
  reset_pairs();
  EXPECT(fails([&] { plan_pairs(3); }, "unknown camera model id 99"));
  pairs[1].image2.camera = make_cam(camera::EQUIRECTANGULAR, 10, 10, {10, 10});
  EXPECT(fails([&] { plan_pairs(3); }, "pair 1: Check failed: camera.IsPerspective()"));
  reset_pairs();
  pairs[1].image2.out = nullptr;
  EXPECT(fails([&] { plan_pairs(3); }, "pair 1: null pixel buffer"));
  reset_pairs();
  pairs[1].image1.channels = 2;
  EXPECT(fails([&] { plan_pairs(3); }, "pair 1: channels must be 1 (grey) or 3 (RGB)"));
  reset_pairs();
  pairs[1].image2.out_capacity = 99;
  EXPECT(fails([&] { plan_pairs(3); }, "pair 1: output buffer of 99 bytes, 100 needed"));
  reset_pairs();
  const up::PairPlan pp = up::plan_pair(o, pairs[1], 1);  // R = I, t = (1, 0, 0), one camera: H1 = H2 = I
  EXPECT(pp.target.width == 10 && equal9(pp.Hinv[0], {1, 0, 0, 0, 1, 0, 0, 0, 1}) && equal9(pp.Hinv[1], {1, 0, 0, 0, 1, 0, 0, 0, 1}));
  EXPECT(pp.Q[11] == -1 && pp.Q[12] == -4 && pp.Q[13] == -4 && pp.Q[14] == 8 && pairs[1].Q[11] == 0);
  const up::ImagePlan side = up::plan_pair_side(o, pp, pairs[1].image2, 1);
  EXPECT(side.route == up::kDirect && side.has_homography && equal9(side.hinv, {1, 0, 0, 0, 1, 0, 0, 0, 1}));
}

static void test_single_image_planners() {
  const undistort_options o = defaults();
  const undistort_cam src = make_cam(camera::OPENCV, 64, 48, {80, 80, 32, 24, 0.1, 0, 0, 0});
  const undistort_cam tgt = make_cam(camera::PINHOLE, 61, 47, {80, 81, 30.25, 23.5});
  const double Hinv[9] = {1, 0, 0.5, 0, 1, 0.25, 0, 0, 1};
  Image im(src, 3, 61 * 47 * 3);
  up::ImagePlan p = up::plan_warp_homography(&o, Hinv, &tgt, &im.im);
  EXPECT(p.route == up::kDirect && p.has_homography && equal9(p.hinv, {1, 0, 0.5, 0, 1, 0.25, 0, 0, 1}));
  EXPECT(p.in_bytes == 64 * 48 * 3 && p.out_words == 48 * 47 && p.grid.x == 1 && p.grid.y == 12 && p.target.width == 61);
  EXPECT(fails([&] { up::plan_warp_homography(&o, nullptr, &tgt, &im.im); }, "null argument"));
  EXPECT(fails([&] { up::plan_warp_homography(&o, Hinv, &src, &im.im); }, "the warp target is a PINHOLE camera"));
  im.im.out_capacity -= 1;
  EXPECT(fails([&] { up::plan_warp_homography(&o, Hinv, &tgt, &im.im); }, "output buffer of 8600 bytes, 8601 needed"));
  im.im.channels = 2;
  EXPECT(fails([&] { up::plan_warp_homography(&o, Hinv, &tgt, &im.im); }, "channels must be 1 (grey) or 3 (RGB)"));
  im.im.camera = make_cam(camera::EQUIRECTANGULAR, 64, 48, {64, 48});
  EXPECT(fails([&] { up::plan_warp_homography(&o, Hinv, &tgt, &im.im); }, "Check failed: camera.IsPerspective()"));

  std::unique_ptr<uint8_t[]> a(new uint8_t[160 * 120 * 3]()), b(new uint8_t[61 * 47 * 3]());
  p = up::plan_resize(a.get(), 160, 120, 3, b.get(), 61, 47);
  EXPECT(p.route == up::kResize && !p.has_homography && p.channels == 3 && p.in_bytes == 160 * 120 * 3);
  EXPECT(p.source.width == 160 && p.source.height == 120 && p.target.width == 61 && p.target.height == 47);
  EXPECT(p.out_words == 48 * 47 && p.grid.x == 1 && p.grid.y == 12);
  EXPECT(up::plan_resize(a.get(), 64, 48, 1, b.get(), 64, 48).route == up::kResize);  // the filter's identity, not a clone
  EXPECT(fails([&] { up::plan_resize(nullptr, 160, 120, 3, b.get(), 61, 47); }, "null argument"));
  EXPECT(fails([&] { up::plan_resize(a.get(), 160, 120, 3, b.get(), 0, 47); }, "image sizes must be positive"));
  EXPECT(fails([&] { up::plan_resize(a.get(), 160, 120, 4, b.get(), 61, 47); }, "channels must be 1 (grey) or 3 (RGB)"));
}

int main() {
  test_undistort_camera();
  test_cam_from_img();
  test_rectify_cameras();
  test_routes();
  test_mid_camera_and_conjugation();
  test_sizes_and_grids();
  test_option_refusals();
  test_image_refusals();
  test_single_image_planners();
  std::printf("undistort plan checks OK\n");
  return 0;
}
