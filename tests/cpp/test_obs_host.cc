// The C++ surface of observation filtering (include/colmap_amd/observation_manager.hpp) from g++ against the C ABI.
//   test_obs_host host     what needs no device: defaults, flattening, the statistics, "no HIP device available"
//   test_obs_host known    the reference's own expectations (sfm/observation_manager_test.cc) on the GPU
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "colmap_amd/observation_manager.hpp"

#define EXPECT(cond)                                                                 \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

using namespace colmap_amd::obs;

static Reconstruction Generate(int num_images, const Camera& camera, double x, double y) {
  Reconstruction rec;
  rec.cameras[1] = camera;
  for (int i = 1; i <= num_images; ++i) {
    Image img;
    img.camera_id = 1;
    img.points2D.resize(10);
    for (Point2D& p : img.points2D) {
      p.xy[0] = x;
      p.xy[1] = y;
    }
    rec.images[i] = img;
  }
  return rec;
}

static int Host() {
  obs_filter_options o;
  std::memset(&o, 0xff, sizeof(o));
  obs_filter_options_init(&o);
  EXPECT(o.max_reproj_error == 4.0 && o.min_tri_angle == 1.5 && o.min_track_len == 2 && o.error_type == OBS_ERROR_PIXEL);
  EXPECT(o.rules == (OBS_RULE_REPROJ_ERROR | OBS_RULE_TRI_ANGLE));
  Reconstruction rec = Generate(3, Camera{1, 1, 1, {1.0, 1.0, 0.5, 0.5}}, 0.0, 0.0);
  const int64_t a = rec.AddPoint3D(0.1, 0.2, 1.0, {{1, 0}, {2, 0}, {3, 0}});
  const int64_t b = rec.AddPoint3D(0.3, 0.1, 2.0, {{1, 1}});
  EXPECT(rec.ComputeNumObservations() == 4 && rec.ComputeMeanTrackLength() == 2.0 && rec.ComputeMeanReprojectionError() == 0.0);
  rec.points3D[a].error = 3.0;
  EXPECT(rec.ComputeMeanReprojectionError() == 3.0);
  detail::Flat f;
  const std::vector<int64_t> ids = {b, 77, b, a};
  detail::Flatten(rec, &ids, &f);
  EXPECT(f.ids.size() == 2 && f.ids[0] == b && f.ids[1] == a && f.model.num_observations == 4);
  EXPECT(f.offsets[1] == 1 && f.offsets[2] == 4 && f.model.num_images == 3 && f.cameras[0].num_params == 4);
  rec.DeletePoint3D(b);
  EXPECT(rec.NumPoints3D() == 1 && !rec.images[1].points2D[1].HasPoint3D());
  // a model the library must reject before it touches a device
  Reconstruction bad = Generate(2, Camera{2, 1, 1, {1.0, 0.5}}, 0.0, 0.0);  // SIMPLE_RADIAL with two parameters
  bad.AddPoint3D(0, 0, 1, {{1, 0}, {2, 0}});
  try {
    ObservationManager(bad).FilterAllPoints3D(4.0, 1.5);
    EXPECT(false);
  } catch (const std::runtime_error& e) {
    EXPECT(std::string(e.what()).find("takes 4 parameters") != std::string::npos);
  }
  std::printf("host OK\n");
  return 0;
}

static int Known() {
  const Camera unit{1, 1, 1, {1.0, 1.0, 0.5, 0.5}};
  {  // FilterAllPoints (:322) and FilterPoints3D (:85)
    Reconstruction rec = Generate(2, unit, 0.0, 0.0);
    ObservationManager om(rec);
    const int64_t p1 = rec.AddPoint3D(0.3, -0.7, 0.4, {{1, 0}, {2, 0}});
    EXPECT(om.FilterPoints3D(0.0, 0.0, {}) == 0 && om.FilterPoints3D(0.0, 0.0, {p1 + 1}) == 0 && rec.NumPoints3D() == 1);
    EXPECT(om.FilterAllPoints3D(0.0, 0.0) == 2 && rec.NumPoints3D() == 0);
    rec.AddPoint3D(0.3, -0.7, 0.4, {{1, 0}});
    EXPECT(om.FilterAllPoints3D(0.0, 0.0) == 1 && rec.NumPoints3D() == 0);
    rec.AddPoint3D(-0.5, -0.5, 1, {{1, 0}, {2, 0}});
    EXPECT(om.FilterAllPoints3D(0.0, 0.0) == 0 && rec.NumPoints3D() == 1);
    EXPECT(om.FilterPoints3DInImages(0.0, 1e-3, {1}) == 2 && rec.NumPoints3D() == 0);
    const int64_t p4 = rec.AddPoint3D(-0.6, -0.5, 1, {{1, 0}, {2, 0}});
    EXPECT(om.FilterAllPoints3D(0.1, 0.0) == 0 && rec.NumPoints3D() == 1);
    EXPECT(std::fabs(rec.points3D[p4].error - 0.1) < 1e-12);
    EXPECT(om.FilterPoints3D(0.09, 0.0, {p4}) == 2 && rec.NumPoints3D() == 0);
  }
  {  // FilterPoints3DWithLargeReprojectionErrorTypes (:137)
    Reconstruction rec = Generate(2, Camera{1, 100, 100, {100.0, 100.0, 50.0, 50.0}}, 50.0, 50.0);
    ObservationManager om(rec);
    const ReprojectionErrorType types[3] = {ReprojectionErrorType::PIXEL, ReprojectionErrorType::NORMALIZED,
                                            ReprojectionErrorType::ANGULAR};
    const double passes[3] = {1.0, 0.01, 0.6}, filters[3] = {0.9, 0.009, 0.5};
    for (int t = 0; t < 3; ++t) {
      const int64_t id = rec.AddPoint3D(0.02, 0, 2, {{1, 0}, {2, 0}});
      EXPECT(om.FilterPoints3DWithLargeReprojectionError(passes[t], {id}, types[t]) == 0);
      EXPECT(om.FilterPoints3DWithLargeReprojectionError(filters[t], {id}, types[t]) == 2);
    }
  }
  {  // FilterPoints3DSphericalSeam (:215)
    Reconstruction rec = Generate(2, Camera{17, 1000, 500, {1000.0, 500.0}}, 0.0, 250.0);
    const int64_t id = rec.AddPoint3D(0, 0, -2, {{1, 0}, {2, 0}});
    EXPECT(ObservationManager(rec).FilterPoints3DWithLargeReprojectionError(1.0, {id}) == 0 && rec.NumPoints3D() == 1);
  }
  {  // FilterPoints3DWithShortTracks (:356)
    Reconstruction rec = Generate(4, unit, 0.0, 0.0);
    ObservationManager om(rec);
    rec.AddPoint3D(0.1, 0.2, 0.3, {{1, 0}});
    rec.AddPoint3D(0.1, 0.2, 0.3, {{1, 1}, {2, 1}});
    rec.AddPoint3D(0.1, 0.2, 0.3, {{1, 2}, {2, 2}, {3, 2}});
    EXPECT(om.FilterPoints3DWithShortTracks(2) == 1 && rec.NumPoints3D() == 2);
    EXPECT(om.FilterPoints3DWithShortTracks(3) == 2 && rec.NumPoints3D() == 1);
    EXPECT(om.FilterPoints3DWithShortTracks(4) == 3 && rec.NumPoints3D() == 0);
  }
  {  // FilterObservationsWithNegativeDepth (:388), UpdatePoint3DErrors
    Reconstruction rec = Generate(2, unit, 0.0, 0.0);
    ObservationManager om(rec);
    const int64_t id = rec.AddPoint3D(0, 0, 1);
    EXPECT(om.FilterObservationsWithNegativeDepth() == 0 && rec.NumPoints3D() == 1);
    rec.AddObservation(id, {1, 0});
    rec.points3D[id].xyz[2] = 0.001;
    EXPECT(om.FilterObservationsWithNegativeDepth() == 0 && rec.NumPoints3D() == 1);
    rec.UpdatePoint3DErrors();
    EXPECT(std::fabs(rec.points3D[id].error - std::sqrt(0.5)) < 1e-12);  // (0.5, 0.5) against (0, 0)
    rec.points3D[id].xyz[2] = 0.0;
    EXPECT(om.FilterObservationsWithNegativeDepth() == 1 && rec.NumPoints3D() == 0);
  }
  std::printf("known OK\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc > 1 && std::string(argv[1]) == "host") return Host();
    if (argc > 1 && std::string(argv[1]) == "known") return Known();
    if (argc > 1 && std::string(argv[1]) == "nodevice") {
      Reconstruction rec = Generate(2, Camera{1, 1, 1, {1.0, 1.0, 0.5, 0.5}}, 0.0, 0.0);
      rec.AddPoint3D(0, 0, 1, {{1, 0}, {2, 0}});
      ObservationManager(rec).FilterAllPoints3D(4.0, 1.5);
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  std::fprintf(stderr, "usage: test_obs_host host|known|nodevice\n");
  return 1;
}
