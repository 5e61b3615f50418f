// The C++ surface of model alignment (include/colmap_amd/alignment.hpp) from g++, linked against the library.
//   host      what runs without a GPU: Sim3d files, Inverse, ComputeImageAlignmentError and the association step
//   nodevice  an alignment without a GPU fails loudly (exit 2)
//   known     on the GPU: a model and its copy under a known similarity are aligned three ways and transformed
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "colmap_amd/alignment.hpp"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

namespace al = colmap_amd::align;
namespace obs = colmap_amd::obs;

static al::Sim3d known_sim() {
  al::Sim3d t;
  t.scale = 1.7;
  const double n = std::sqrt(0.81 + 0.01 + 0.04 + 0.09);
  t.rotation = {{0.9 / n, 0.1 / n, -0.2 / n, 0.3 / n}};
  t.translation = {{0.5, -1.0, 2.0}};
  return t;
}

// `tgt`: 12 pinhole images on a ring looking along +z, 60 points seen by all; `src`: the same model under Inverse(sim)
static void make_models(obs::Reconstruction* src, obs::Reconstruction* tgt) {
  std::mt19937 rng(7);
  std::uniform_real_distribution<double> u(-1, 1);
  const al::Sim3d sim = known_sim(), inv = al::Inverse(sim);
  for (obs::Reconstruction* r : {src, tgt}) r->cameras[1] = obs::Camera{1 /* PINHOLE */, 640, 480, {500, 500, 320, 240}};
  for (int i = 1; i <= 12; ++i) {
    obs::Image img;
    img.camera_id = 1;
    img.cam_from_world = {{0, 0, 0, 1, u(rng), u(rng), 6.0 + u(rng)}};
    tgt->images[i] = img;
    src->images[i] = img;
  }
  for (int p = 0; p < 60; ++p) {
    const std::array<double, 3> X{{u(rng), u(rng), u(rng)}};
    std::vector<obs::TrackElement> track;
    for (int i = 1; i <= 12; ++i) {
      obs::Image& img = tgt->images[i];
      obs::Point2D p2;
      const double x = X[0] + img.cam_from_world[4], y = X[1] + img.cam_from_world[5], z = X[2] + img.cam_from_world[6];
      p2.xy[0] = 500 * x / z + 320;
      p2.xy[1] = 500 * y / z + 240;
      img.points2D.push_back(p2);
      src->images[i].points2D.push_back(p2);
      track.push_back({i, p});
    }
    tgt->AddPoint3D(X[0], X[1], X[2], track);
    src->AddPoint3D(X[0], X[1], X[2], track);
  }
  for (auto& kv : src->points3D) {  // move src by hand: points and poses, as Transform does with the device
    const std::array<double, 3> y = inv * std::array<double, 3>{{kv.second.xyz[0], kv.second.xyz[1], kv.second.xyz[2]}};
    for (int c = 0; c < 3; ++c) kv.second.xyz[c] = y[(size_t)c];
  }
  for (auto& kv : src->images) {
    auto& p = kv.second.cam_from_world;  // identity rotation: R' = R^T of inv = rotation of sim, t' = s_inv t_c - R' t_inv
    double Rs[9];
    al::QuatToRotation(sim.rotation.data(), Rs);
    double t[3];
    for (int r = 0; r < 3; ++r)
      t[r] = inv.scale * p[4 + (size_t)r] - (Rs[3 * r] * inv.translation[0] + Rs[3 * r + 1] * inv.translation[1] + Rs[3 * r + 2] * inv.translation[2]);
    p = {{sim.rotation[1], sim.rotation[2], sim.rotation[3], sim.rotation[0], t[0], t[1], t[2]}};
  }
}

static double distance(const al::Sim3d& a, const al::Sim3d& b) {
  double d = 0;
  for (const std::array<double, 3>& x : {std::array<double, 3>{{1, 0, 0}}, {{0, 1, 0}}, {{0, 0, 1}}, {{0, 0, 0}}}) {
    const auto p = a * x, q = b * x;
    for (int c = 0; c < 3; ++c) d = std::max(d, std::abs(p[(size_t)c] - q[(size_t)c]));
  }
  return d;
}

static void host(const std::string& dir) {
  const al::Sim3d sim = known_sim();
  sim.ToFile(dir + "/sim.txt");
  const al::Sim3d back = al::Sim3d::FromFile(dir + "/sim.txt");
  EXPECT(back.params() == sim.params());  // 17 digits round-trip a double
  EXPECT(distance(al::Inverse(al::Inverse(sim)), sim) < 1e-15);
  const auto x = al::Inverse(sim) * (sim * std::array<double, 3>{{0.3, -0.7, 1.1}});
  EXPECT(std::abs(x[0] - 0.3) < 1e-15 && std::abs(x[1] + 0.7) < 1e-15 && std::abs(x[2] - 1.1) < 1e-15);

  obs::Reconstruction src, tgt;
  make_models(&src, &tgt);
  EXPECT(al::FindCommonRegImageIds(src, tgt).size() == 12);
  for (const al::ImageAlignmentError& e : al::ComputeImageAlignmentError(src, tgt, sim))
    EXPECT(e.rotation_error_deg < 1e-6 && e.proj_center_error < 1e-12);
  // by hand: identity similarity, tgt camera 2 turned by 90 degrees about z and its centre moved by (3, 4, 0)
  obs::Reconstruction a, b;
  a.images[2].cam_from_world = {{0, 0, 0, 1, 0, 0, 0}};
  b.images[2].cam_from_world = {{0, 0, std::sqrt(0.5), std::sqrt(0.5), -4, 3, 0}};  // centre = -R^T t = (3, 4, 0)
  const auto errors = al::ComputeImageAlignmentError(a, b, al::Sim3d());
  EXPECT(errors.size() == 1 && std::abs(errors[0].rotation_error_deg - 90.0) < 1e-12 && std::abs(errors[0].proj_center_error - 5.0) < 1e-14);

  // association: every src point meets its tgt point in all 12 images; the count starts at 0, so it reaches 11, not 12
  std::vector<std::array<double, 3>> pa, pb;
  al::AssociatePoints(src, tgt, 11, &pa, &pb);
  EXPECT(pa.size() == 60);  // 12 votes count 11
  pa.clear();
  pb.clear();
  al::AssociatePoints(src, tgt, 12, &pa, &pb);
  EXPECT(pa.empty());
  std::printf("host OK\n");
}

static void known() {
  obs::Reconstruction src, tgt;
  make_models(&src, &tgt);
  const al::Sim3d sim = known_sim();
  al::Sim3d got;
  EXPECT(al::AlignReconstructionsViaReprojections(src, tgt, 0.3, 8.0, &got) && distance(got, sim) < 1e-9);
  EXPECT(al::AlignReconstructionsViaProjCenters(src, tgt, 0.01, &got) && distance(got, sim) < 1e-9);
  EXPECT(al::AlignReconstructionsViaPoints(src, tgt, 3, 0.005, 0.9, &got) && distance(got, sim) < 1e-9);
  al::Transform(&src, sim);
  for (const auto& kv : src.points3D)
    for (int c = 0; c < 3; ++c) EXPECT(std::abs(kv.second.xyz[c] - tgt.points3D.at(kv.first).xyz[c]) < 1e-12);
  for (const al::ImageAlignmentError& e : al::ComputeImageAlignmentError(src, tgt, al::Sim3d()))
    EXPECT(e.rotation_error_deg < 1e-6 && e.proj_center_error < 1e-12);
  std::printf("known OK\n");
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  if (mode == "host") host(argc > 2 ? argv[2] : ".");
  if (mode == "known") known();
  if (mode == "nodevice") {
    obs::Reconstruction src, tgt;
    make_models(&src, &tgt);
    al::Sim3d got;
    try {
      al::AlignReconstructionsViaProjCenters(src, tgt, 0.01, &got);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 2;
    }
    return 0;
  }
  return 0;
}
