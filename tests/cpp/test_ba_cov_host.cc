// Exercises include/colmap_amd/ba_covariance.hpp (the C++ host side of the covariance estimate).
//   test_ba_cov_host api                       host-only: options, Rigid3d adjoints, relative-pose propagation
//   test_ba_cov_host run FILE PARAMS OUT        flatten FILE (tests/test_cpp_host.py spec format), solve on the GPU,
//                                               EstimateBACovariance(PARAMS = BA_COV_*), write every result to OUT
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "colmap_amd/ba_covariance.hpp"

using namespace colmap_amd;

#define EXPECT(cond)                                                                 \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

static Rigid3d ReadPose(std::istream& f) {
  Rigid3d p;
  for (auto& v : p.params) f >> v;
  return p;
}

struct Spec {
  Reconstruction rec;
  BundleAdjustmentConfig config;
  BundleAdjustmentOptions options;
};

static void ReadSpec(const std::string& path, Spec* s) {
  std::ifstream f(path);
  if (!f.is_open()) throw std::runtime_error("cannot open " + path);
  std::string tag;
  size_t n;
  f >> tag >> n;  // cameras
  for (size_t i = 0; i < n; ++i) {
    Camera c;
    size_t np;
    f >> c.camera_id >> c.model_id >> c.width >> c.height >> np;
    c.params.resize(np);
    for (auto& v : c.params) f >> v;
    s->rec.cameras[c.camera_id] = c;
  }
  f >> tag >> n;  // rigs
  for (size_t i = 0; i < n; ++i) {
    Rig r;
    size_t ns;
    f >> r.rig_id >> r.ref_camera_id >> ns;
    for (size_t j = 0; j < ns; ++j) {
      camera_t cid;
      f >> cid;
      r.sensors_from_rig[cid] = ReadPose(f);
    }
    s->rec.rigs[r.rig_id] = r;
  }
  f >> tag >> n;  // frames
  for (size_t i = 0; i < n; ++i) {
    Frame fr;
    size_t ni;
    f >> fr.frame_id >> fr.rig_id;
    fr.rig_from_world = ReadPose(f);
    f >> ni;
    fr.image_ids.resize(ni);
    for (auto& v : fr.image_ids) f >> v;
    s->rec.frames[fr.frame_id] = fr;
  }
  f >> tag >> n;  // images
  for (size_t i = 0; i < n; ++i) {
    Image im;
    long long frame;
    size_t np;
    f >> im.image_id >> im.camera_id >> frame;
    if (frame >= 0) im.frame_id = static_cast<frame_t>(frame);
    im.cam_from_world = ReadPose(f);
    f >> np;
    im.points2D.resize(np);
    for (auto& p : im.points2D) {
      long long pid;
      f >> p.xy[0] >> p.xy[1] >> pid;
      p.point3D_id = pid < 0 ? kInvalidPoint3DId : static_cast<point3D_t>(pid);
    }
    s->rec.images[im.image_id] = im;
  }
  f >> tag >> n;  // points
  for (size_t i = 0; i < n; ++i) {
    point3D_t pid;
    Point3D p;
    size_t nt;
    f >> pid >> p.xyz[0] >> p.xyz[1] >> p.xyz[2] >> nt;
    p.track.resize(nt);
    for (auto& el : p.track) f >> el.image_id >> el.point2D_idx;
    s->rec.points3D[pid] = p;
  }
  int gauge;
  f >> tag >> gauge;  // gauge
  s->config.FixGauge(static_cast<BundleAdjustmentGauge>(gauge));
  auto read_ids = [&](auto&& fn) {
    f >> tag >> n;
    for (size_t i = 0; i < n; ++i) {
      unsigned long long id;
      f >> id;
      fn(id);
    }
  };
  read_ids([&](auto id) { s->config.AddImage(static_cast<image_t>(id)); });
  read_ids([&](auto id) { s->config.SetConstantCamIntrinsics(static_cast<camera_t>(id)); });
  read_ids([&](auto id) { s->config.SetConstantRigFromWorldPose(static_cast<frame_t>(id)); });
  read_ids([&](auto id) { s->config.SetConstantSensorFromRigPose(static_cast<camera_t>(id)); });
  read_ids([&](auto id) { s->config.AddVariablePoint(id); });
  read_ids([&](auto id) { s->config.AddConstantPoint(id); });
  read_ids([&](auto id) { s->config.IgnorePoint(id); });
  int b[7], loss, max_iter;
  double loss_scale, grad_tol;
  f >> tag;
  for (int& v : b) f >> v;
  f >> s->options.min_track_length >> loss >> loss_scale >> max_iter >> grad_tol;
  if (!f.good()) throw std::runtime_error("malformed spec " + path);
  s->options.refine_focal_length = b[0];
  s->options.refine_principal_point = b[1];
  s->options.refine_extra_params = b[2];
  s->options.refine_sensor_from_rig = b[3];
  s->options.refine_rig_from_world = b[4];
  s->options.refine_points3D = b[5];
  s->options.constant_rig_from_world_rotation = b[6];
  s->options.gpu_index = "0";
  s->options.mi355x->loss_function_type = static_cast<Mi355xBundleAdjustmentOptions::LossFunctionType>(loss);
  s->options.mi355x->loss_function_scale = loss_scale;
  s->options.mi355x->solver_options.max_num_iterations = max_iter;
  s->options.mi355x->solver_options.gradient_tolerance = grad_tol;
}

static int Api() {
  BACovarianceOptions o;
  EXPECT(o.params == BACovarianceOptions::Params::ALL && o.damping == 1e-8);
  ba_covariance_options co;
  ba_covariance_options_init(&co);
  EXPECT(co.params == BA_COV_ALL && co.damping == 1e-8);
  Rigid3d t;
  t.params = {0.1, -0.2, 0.3, 0.0, 0.5, -1.0, 2.0};
  double n = 0.0;
  for (int k = 0; k < 4; ++k) n += t.params[k] * t.params[k];
  for (int k = 0; k < 4; ++k) t.params[k] /= std::sqrt(n);
  const auto A = Rigid3dAdjoint(t, false), Ai = Rigid3dAdjoint(t, true);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      double m = 0.0;
      for (int k = 0; k < 6; ++k) m += A[6 * r + k] * Ai[6 * k + c];
      EXPECT(std::fabs(m - (r == c ? 1.0 : 0.0)) < 1e-12);
    }
  // perfectly correlated poses (rigid3_test.cc:184-208, with a = b): the relative pose has no uncertainty
  MatrixXd cov(12, 12);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      const double v = (r == c ? 2.0 : 0.0) + 0.1 * (r + c);
      cov(r, c) = cov(r + 6, c + 6) = cov(r, c + 6) = cov(r + 6, c) = v;
    }
  const MatrixXd rel = GetCovarianceForRelativeRigid3d(t, t, cov);
  for (double v : rel.values) EXPECT(std::fabs(v) < 1e-12);
  bool threw = false;
  try {
    (void)GetCovarianceForRelativeRigid3d(t, t, MatrixXd(6, 6));
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  std::printf("api OK\n");
  return 0;
}

static void Put(std::ofstream& f, const std::string& head, const std::optional<MatrixXd>& m) {
  if (!m) return;
  f << head << " " << m->rows << " " << m->cols;
  for (double v : m->values) f << " " << v;
  f << "\n";
}

static int Run(const std::string& path, int params, const std::string& out) {
  Spec s;
  ReadSpec(path, &s);
  auto ba = CreateDefaultBundleAdjuster(s.options, s.config, s.rec);
  if (!ba->Solve()->IsSolutionUsable()) return 4;
  BACovarianceOptions o;
  o.params = static_cast<BACovarianceOptions::Params>(params);
  const std::optional<BACovariance> cov = EstimateBACovariance(o, s.rec, *ba);
  std::ofstream f(out);
  f << std::setprecision(17);
  if (!cov) {
    f << "none " << ba_last_error() << "\n";
    return 0;
  }
  std::vector<image_t> ids;
  for (const auto& kv : s.rec.images) ids.push_back(kv.first);
  for (image_t a : ids) {
    Put(f, "pose " + std::to_string(a), cov->GetCamCovFromWorld(a));
    for (image_t b : ids) Put(f, "cross " + std::to_string(a) + " " + std::to_string(b), cov->GetCamCrossCovFromWorld(a, b));
  }
  if (ids.size() >= 2)
    Put(f, "rel " + std::to_string(ids[0]) + " " + std::to_string(ids[1]),
        cov->GetCam2CovFromCam1(ids[0], s.rec.images.at(ids[0]).cam_from_world, ids[1], s.rec.images.at(ids[1]).cam_from_world));
  for (const auto& kv : s.rec.points3D) Put(f, "point " + std::to_string(kv.first), cov->GetPointCov(kv.first));
  for (const auto& kv : s.rec.cameras) {
    Put(f, "camera " + std::to_string(kv.first), cov->GetOtherParamsCov(kv.second.params.data()));
    const std::vector<double> copy = kv.second.params;  // lookup by identity, not by value
    EXPECT(!cov->GetOtherParamsCov(copy.data()));
  }
  EXPECT(!cov->GetPointCov(kInvalidPoint3DId - 1) && !cov->GetCamCovFromWorld(0xfffffff0u));
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && std::string(argv[1]) == "api") return Api();
    if (argc >= 5 && std::string(argv[1]) == "run") return Run(argv[2], std::stoi(argv[3]), argv[4]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
  std::fprintf(stderr, "usage: test_ba_cov_host api | run FILE PARAMS OUT\n");
  return 2;
}
