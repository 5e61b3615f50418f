// The host-only layout of a bundle-adjustment solve (colmap_amd/csrc/ba_layout.h: make_layout) on small problems built
// in memory, against brute-force code written here. No GPU, nothing linked from the library.
#include "ba_layout.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>

using ba_layout::Incidences;
using ba_layout::Layout;
using ba_layout::LayoutParams;
using ba_layout::make_layout;

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

namespace {

// parameters of the camera models the cases use (sensor/models.h of the reference: the documented counts)
int npar(int model) {
  switch (model) {
    case BA_PINHOLE: case BA_SIMPLE_RADIAL: return 4;
    case BA_OPENCV: return 8;
    case BA_FULL_OPENCV: return 12;
    default: std::abort();
  }
}

struct Prob {
  std::vector<double> poses, cams, points, xy, sensors, prior_pos, prior_A;
  std::vector<int32_t> model, op, oc, ox, os, prior_pose, prior_sensor;
  std::vector<uint8_t> pose_const, cam_const, point_const, sensor_const;
  std::vector<int8_t> fixed_t;
  bool rigs = false;
  ba_problem p{};

  int pose(bool constant = false, int fixed = -1) {
    poses.insert(poses.end(), {0, 0, 0, 1, 0, 0, 0});
    pose_const.push_back(constant); fixed_t.push_back((int8_t)fixed);
    return (int)pose_const.size() - 1;
  }
  int cam(int m, const std::vector<int>& variable) {  // indices of the variable parameters
    model.push_back(m);
    cams.resize(cams.size() + BA_CAM_STRIDE, 1.0);
    cam_const.resize(cam_const.size() + BA_CAM_STRIDE, 1);
    for (int j : variable) cam_const[(model.size() - 1) * BA_CAM_STRIDE + j] = 0;
    return (int)model.size() - 1;
  }
  int point(bool constant = false) {
    points.insert(points.end(), {0, 0, 1});
    point_const.push_back(constant);
    return (int)point_const.size() - 1;
  }
  int sensor(bool constant) {
    rigs = true;
    sensors.insert(sensors.end(), {0, 0, 0, 1, 0, 0, 0});
    sensor_const.push_back(constant);
    return (int)sensor_const.size() - 1;
  }
  void obs(int pi, int ci, int xi, int si = -1) {
    op.push_back(pi); oc.push_back(ci); ox.push_back(xi); os.push_back(si);
    xy.push_back(0.25 * (double)op.size()); xy.push_back(-0.5 * (double)op.size());
  }
  void prior(int pi, int si) {
    prior_pose.push_back(pi); prior_sensor.push_back(si);
    for (int c = 0; c < 3; ++c) prior_pos.push_back((double)prior_pose.size() + 0.1 * c);
    for (int c = 0; c < 9; ++c) prior_A.push_back(100.0 * (double)prior_pose.size() + c);
  }
  const ba_problem& get() {
    p.num_poses = (int)pose_const.size(); p.num_cams = (int)model.size(); p.num_points = (int)point_const.size();
    p.num_obs = (int64_t)op.size();
    p.poses = poses.data(); p.cams = cams.data(); p.cam_model = model.data(); p.points = points.data();
    p.obs_pose = op.data(); p.obs_cam = oc.data(); p.obs_point = ox.data(); p.obs_xy = xy.data();
    p.pose_const = pose_const.data(); p.pose_fixed_t = fixed_t.data(); p.cam_const = cam_const.data();
    p.point_const = point_const.data();
    p.num_sensors = (int)sensor_const.size();
    p.sensors = rigs ? sensors.data() : nullptr;
    p.obs_sensor = rigs ? os.data() : nullptr;
    p.sensor_const = rigs ? sensor_const.data() : nullptr;
    p.num_priors = (int)prior_pose.size();
    p.prior_pose = prior_pose.data(); p.prior_sensor = prior_sensor.data();
    p.prior_position = prior_pos.data(); p.prior_sqrt_info = prior_A.data();
    p.prior_loss_type = BA_LOSS_TRIVIAL; p.prior_loss_scale = 1.0;
    return p;
  }
  // brute force
  int nvar(int k) const {
    int n = 0;
    for (int j = 0; j < npar(model[k]); ++j) n += !cam_const[(size_t)k * BA_CAM_STRIDE + j];
    return n;
  }
  bool sens_var(int64_t o) const { return rigs && os[o] >= 0 && !sensor_const[os[o]]; }
  bool active(int64_t o) const { return !pose_const[op[o]] || nvar(oc[o]) > 0 || !point_const[ox[o]] || sens_var(o); }
};

LayoutParams params(int rank = 0, int world = 1, bool by_point = false) {
  LayoutParams P;
  P.rank = rank; P.world = world; P.by_point = by_point;
  P.chunk = 512; P.heavy_chunks = 64; P.tile_pts = 256; P.tile_obs = 512; P.inc_chunk = 128; P.pair_chunk = 32;
  P.pair_incidences = true;
  return P;
}

// caller observation of c-order position c
int64_t obs_of_c(const Layout& L, int c) { return L.obs_of_a[L.c2a[c]]; }

// the two orders and both topology copies against the problem
void check_orders(const Prob& q, const Layout& L, int rank, int world, bool by_point) {
  std::vector<int64_t> want;
  int64_t n_global = 0;
  for (int j = 0; j < q.p.num_points; ++j)
    for (int64_t o = 0; o < q.p.num_obs; ++o)
      if (q.ox[o] == j && q.active(o) && (by_point ? q.ox[o] : q.op[o]) % world == rank) want.push_back(o);
  for (int64_t o = 0; o < q.p.num_obs; ++o) n_global += q.active(o);
  CHECK(L.n_active_global == n_global);
  CHECK(L.obs_of_a == want);
  const int n = (int)want.size();
  CHECK(L.n == n);
  std::vector<int> order(n);
  for (int a = 0; a < n; ++a) order[a] = a;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return std::make_pair(q.oc[want[a]], q.op[want[a]]) < std::make_pair(q.oc[want[b]], q.op[want[b]]);
  });
  CHECK(L.c2a == order);
  CHECK((int)L.a2c.size() == n);
  for (int c = 0; c < n; ++c) CHECK(L.a2c[L.c2a[c]] == c);
  CHECK((int)L.pt_ptr.size() == q.p.num_points + 1 && L.pt_ptr[0] == 0 && L.pt_ptr.back() == n);
  for (int j = 0; j < q.p.num_points; ++j)
    for (int a = L.pt_ptr[j]; a < L.pt_ptr[j + 1]; ++a) CHECK(q.ox[want[a]] == j);
  for (int a = 0; a < n; ++a) {
    const int64_t o = want[a];
    const int c = L.a2c[a];
    CHECK(L.a_pose[a] == q.op[o] && L.a_cam[a] == q.oc[o] && L.a_pt[a] == q.ox[o]);
    CHECK(L.a_xy[2 * a] == q.xy[2 * o] && L.a_xy[2 * a + 1] == q.xy[2 * o + 1]);
    CHECK(L.o_pose[c] == q.op[o] && L.o_cam[c] == q.oc[o] && L.o_pt[c] == q.ox[o]);
    CHECK(L.o_xy[2 * c] == q.xy[2 * o] && L.o_xy[2 * c + 1] == q.xy[2 * o + 1]);
    if (q.rigs) CHECK(L.a_sensor[a] == q.os[o] && L.o_sensor[c] == q.os[o]);
  }
}

// 6 poses (one constant, one unobserved), 3 cameras (one constant), n_pts points with tracks of 2 - 5, the first five
// constant; observations interleaved over the points
void mixed_problem(Prob& q, int n_pts) {
  for (int i = 0; i < 6; ++i) q.pose(i == 0);
  q.cam(BA_PINHOLE, {});
  q.cam(BA_SIMPLE_RADIAL, {0, 3});
  q.cam(BA_OPENCV, {0, 1, 2, 3});
  for (int j = 0; j < n_pts; ++j) q.point(j < 5);
  for (int r = 0; r < 5; ++r)
    for (int j = 0; j < n_pts; ++j)
      if (r < 2 + j % 4) q.obs((j + r) % 5, ((j + r) % 5 / 2 + j) % 3, j);
  q.get();
}

void test_orders() {
  Prob q;
  mixed_problem(q, 40);
  int inactive = 0;
  for (int64_t o = 0; o < q.p.num_obs; ++o) inactive += !q.active(o);
  CHECK(inactive >= 1);  // an observation whose blocks are all constant
  const Layout L = make_layout(q.p, params());
  check_orders(q, L, 0, 1, false);
  CHECK(L.pose_off[5] == -1 && L.blk_of_pose[5] == -1);  // nobody observes it
}

void test_tangent_layout() {
  Prob q;
  const int dim_of_fixed[9] = {6, 5, 5, 5, 6, 2, 2, 2, 3};  // pose_fixed_t = -1 .. 7
  for (int f = -1; f <= 7; ++f) q.pose(false, f);
  const int p_const = q.pose(true), p_unseen = q.pose(false);
  const int c_two = q.cam(BA_PINHOLE, {0, 3}), c_const = q.cam(BA_PINHOLE, {}), c_unseen = q.cam(BA_SIMPLE_RADIAL, {0, 1, 2, 3});
  const int c_opencv = q.cam(BA_OPENCV, {1, 2, 4, 6, 7});
  const int s_const = q.sensor(true), s_var = q.sensor(false), s_unseen = q.sensor(false);
  for (int j = 0; j < 12; ++j) q.point(j % 4 == 3);
  const int x_unseen = q.point(false);
  for (int j = 0; j < 12; ++j) {
    q.obs(j % 9, j % 2 ? c_two : c_opencv, j, j % 3 == 0 ? s_var : (j % 3 == 1 ? s_const : -1));
    q.obs((j + 4) % 9, c_const, j);
    q.obs(p_const, c_const, j);
  }
  const Layout L = make_layout(q.get(), params());
  int off = 0, moff = 0, b = 0;
  auto expect_block = [&](int kind, int dim, int got_off, int got_blk) {
    CHECK(got_off == off && got_blk == b);
    CHECK(L.blk_off[b] == off && L.blk_dim[b] == dim && L.blk_kind[b] == kind && L.blk_moff[b] == moff);
    off += dim; moff += dim * dim; ++b;
  };
  for (int i = 0; i < 9; ++i) {
    expect_block(0, dim_of_fixed[i], L.pose_off[i], L.blk_of_pose[i]);
    CHECK(L.pose_dim[i] == dim_of_fixed[i] && L.pose_fix[i] == i - 1);
  }
  for (int i : {p_const, p_unseen}) CHECK(L.pose_off[i] == -1 && L.blk_of_pose[i] == -1 && L.pose_dim[i] == 0 && L.pose_fix[i] == -1);
  expect_block(1, 2, L.cam_off[c_two], L.blk_of_cam[c_two]);
  expect_block(1, 5, L.cam_off[c_opencv], L.blk_of_cam[c_opencv]);
  for (int k : {c_const, c_unseen}) CHECK(L.cam_off[k] == -1 && L.blk_of_cam[k] == -1 && L.cam_dim[k] == 0);
  CHECK(L.cam_dim[c_two] == 2 && L.cam_dim[c_opencv] == 5);
  CHECK(L.cam_nvar[c_two] == 2 && L.cam_nvar[c_const] == 0 && L.cam_nvar[c_unseen] == 4 && L.cam_nvar[c_opencv] == 5);
  const int want_var[5] = {1, 2, 4, 6, 7};
  for (int d = 0; d < 5; ++d) CHECK(L.cam_var[(size_t)c_opencv * BA_CAM_STRIDE + d] == want_var[d]);
  CHECK(L.cam_var[(size_t)c_two * BA_CAM_STRIDE] == 0 && L.cam_var[(size_t)c_two * BA_CAM_STRIDE + 1] == 3);
  expect_block(2, 6, L.sens_off[s_var], L.blk_of_sens[s_var]);
  for (int k : {s_const, s_unseen}) CHECK(L.sens_off[k] == -1 && L.blk_of_sens[k] == -1);
  CHECK(L.n_blk() == b && L.n_c == off && L.moff_total == moff && L.n_var_sensors == 1);
  int poff = 0;
  for (int j = 0; j < 12; ++j) {
    CHECK(L.pt_off[j] == (j % 4 == 3 ? -1 : poff));
    if (j % 4 != 3) poff += 3;
  }
  CHECK(L.pt_off[x_unseen] == -1 && L.n_p == poff);
  CHECK(L.max_nvar == 5 && L.max_npar == 8 && ba_layout::pick_tier(L) == ba_layout::TIER_MAX);
  // tiers
  auto tier_of = [](int model, int nvar) {
    Prob t;
    std::vector<int> var(nvar);
    for (int d = 0; d < nvar; ++d) var[d] = d;
    t.pose(); t.cam(model, var); t.point();
    t.obs(0, 0, 0);
    const Layout Lt = make_layout(t.get(), params());
    CHECK(Lt.max_nvar == nvar && Lt.max_npar == npar(model));
    return ba_layout::pick_tier(Lt);
  };
  CHECK(tier_of(BA_OPENCV, 4) == ba_layout::TIER_NARROW);
  CHECK(tier_of(BA_OPENCV, 5) == ba_layout::TIER_MAX);
  CHECK(tier_of(BA_OPENCV, 8) == ba_layout::TIER_MAX);
  CHECK(tier_of(BA_FULL_OPENCV, 9) == ba_layout::TIER_WIDE);
  CHECK(tier_of(BA_FULL_OPENCV, 2) == ba_layout::TIER_WIDE);  // a 12-parameter model, whatever is variable
  Layout counts;
  counts.max_nvar = 9; counts.max_npar = 8;
  CHECK(ba_layout::pick_tier(counts) == ba_layout::TIER_WIDE);
}

// the c-order positions that touch block b, from the problem
std::set<int> positions_of_block(const Prob& q, const Layout& L, int b) {
  std::set<int> s;
  for (int c = 0; c < L.n; ++c) {
    const int64_t o = obs_of_c(L, c);
    if (L.blk_of_pose[q.op[o]] == b || L.blk_of_cam[q.oc[o]] == b || (q.rigs && q.os[o] >= 0 && L.blk_of_sens[q.os[o]] == b))
      s.insert(c);
  }
  return s;
}

void test_chunks() {
  Prob q;
  for (int i = 0; i < 8; ++i) q.pose();
  q.cam(BA_PINHOLE, {0, 1}); q.cam(BA_PINHOLE, {0}); q.cam(BA_PINHOLE, {2, 3});
  for (int j = 0; j < 60; ++j) q.point();
  for (int j = 0; j < 60; ++j)
    for (int r = 0; r < 4; ++r) {
      const int pi = (j + 2 * r) % 8;
      // camera 0 is shared by all images; pose 0 is also seen through cameras 1 and 2, pose 1 through camera 1
      const int ci = pi == 0 ? j % 3 : (pi == 1 && j % 2 ? 1 : 0);
      q.obs(pi, ci, j);
    }
  LayoutParams P = params();
  P.chunk = 64; P.heavy_chunks = 2;
  const Layout L = make_layout(q.get(), P);
  check_orders(q, L, 0, 1, false);
  const int nb = L.n_blk(), nch = (int)L.chunk_blk.size();
  CHECK(nb == 11 && (int)L.blk_chunk_ptr.size() == nb + 1 && L.blk_chunk_ptr[0] == 0 && L.blk_chunk_ptr[nb] == nch);
  CHECK((int)L.chunk_beg.size() == nch && (int)L.chunk_end.size() == nch);
  std::vector<int> want_heavy;
  bool some_block_has_two_runs = false;
  for (int b = 0; b < nb; ++b) {
    const std::set<int> want = positions_of_block(q, L, b);
    std::set<int> got;
    for (int ch = L.blk_chunk_ptr[b]; ch < L.blk_chunk_ptr[b + 1]; ++ch) {
      CHECK(L.chunk_blk[ch] == b);
      CHECK(L.chunk_beg[ch] < L.chunk_end[ch] && L.chunk_end[ch] - L.chunk_beg[ch] <= 64);
      for (int c = L.chunk_beg[ch]; c < L.chunk_end[ch]; ++c) {
        CHECK(want.count(c) == 1);        // a contiguous run of the block
        CHECK(got.insert(c).second);      // no position twice
      }
      if (ch > L.blk_chunk_ptr[b] && L.chunk_beg[ch] != L.chunk_end[ch - 1]) some_block_has_two_runs = true;
    }
    CHECK(got == want);
    const int count = L.blk_chunk_ptr[b + 1] - L.blk_chunk_ptr[b];
    if (count > 2) want_heavy.push_back(b);
    CHECK(L.blk_fin_end[b] == (count > 2 ? L.blk_chunk_ptr[b] + 1 : L.blk_chunk_ptr[b + 1]));
  }
  for (int ch = 0; ch < nch; ++ch) CHECK(ch >= L.blk_chunk_ptr[L.chunk_blk[ch]] && ch < L.blk_chunk_ptr[L.chunk_blk[ch] + 1]);
  CHECK(some_block_has_two_runs);
  CHECK(positions_of_block(q, L, L.blk_of_cam[0]).size() > 128);
  CHECK(L.heavy == want_heavy);
  CHECK(std::count(want_heavy.begin(), want_heavy.end(), L.blk_of_cam[0]) == 1);   // > 128 observations
  CHECK(std::count(want_heavy.begin(), want_heavy.end(), L.blk_of_pose[0]) == 1);  // three short runs
  CHECK((int)want_heavy.size() < nb);
}

void test_tiles() {
  Prob q;
  for (int i = 0; i < 200; ++i) q.pose();
  q.cam(BA_PINHOLE, {0});
  for (int j = 0; j < 700; ++j) {
    q.point();
    const int len = j % 50 == 7 ? 200 : 2 + j % 2;
    for (int r = 0; r < len; ++r) q.obs((j + r) % 200, 0, j);
  }
  const Layout L = make_layout(q.get(), params());
  CHECK(L.tile_pt.size() >= 3 && L.tile_pt.front() == 0 && L.tile_pt.back() == 700);
  bool hit_obs = false;
  for (size_t t = 0; t + 1 < L.tile_pt.size(); ++t) {
    const int q0 = L.tile_pt[t], q1 = L.tile_pt[t + 1];
    CHECK(q0 < q1 && q1 - q0 <= 256 && L.pt_ptr[q1] - L.pt_ptr[q0] <= 512);
    hit_obs |= q1 - q0 < 256 && q1 < 700;
  }
  CHECK(hit_obs);
  Prob z;
  for (int i = 0; i < 513; ++i) z.pose();
  z.cam(BA_PINHOLE, {0});
  z.point(); z.point();
  z.obs(0, 0, 0); z.obs(1, 0, 0);
  for (int i = 0; i < 513; ++i) z.obs(i, 0, 1);
  const Layout Lz = make_layout(z.get(), params());
  CHECK(Lz.tile_pt == std::vector<int>(1, 0));  // zero tiles
}

// sorted by block, chunks of <= max_len incidences of one block, per-block CSR, the list of blocks with incidences
void check_incidence_chunks(const Incidences& I, int n_blk, int max_len) {
  const int ni = I.n(), nch = (int)I.chunk_blk.size();
  CHECK((int)I.blk.size() == ni && (int)I.ptr.size() == ni + 1 && I.ptr[0] == 0);
  for (int i = 0; i + 1 < ni; ++i) CHECK(I.blk[i] <= I.blk[i + 1]);
  CHECK((int)I.chunk_beg.size() == nch + 1 && I.chunk_beg[0] == 0 && I.chunk_beg[nch] == ni);
  CHECK((int)I.blk_chunk.size() == n_blk + 1 && I.blk_chunk[0] == 0 && I.blk_chunk[n_blk] == nch);
  std::vector<int> blocks;
  for (int ch = 0; ch < nch; ++ch) {
    CHECK(I.chunk_beg[ch] < I.chunk_beg[ch + 1] && I.chunk_beg[ch + 1] - I.chunk_beg[ch] <= max_len);
    for (int i = I.chunk_beg[ch]; i < I.chunk_beg[ch + 1]; ++i) CHECK(I.blk[i] == I.chunk_blk[ch]);
    CHECK(ch >= I.blk_chunk[I.chunk_blk[ch]] && ch < I.blk_chunk[I.chunk_blk[ch] + 1]);
    if (blocks.empty() || blocks.back() != I.chunk_blk[ch]) blocks.push_back(I.chunk_blk[ch]);
  }
  for (int b = 0; b < n_blk; ++b) CHECK(I.blk_chunk[b] <= I.blk_chunk[b + 1]);
  CHECK(I.blocks == blocks);
  for (size_t k = 0; k + 1 < blocks.size(); ++k) CHECK(blocks[k] < blocks[k + 1]);
}

void test_solo_and_pairs() {
  // shared intrinsics and a two-sensor rig (sensor 1 variable): a frame's pose block sees a point through both sensors
  Prob q;
  for (int i = 0; i < 5; ++i) q.pose(i == 4);
  q.cam(BA_SIMPLE_RADIAL, {0, 3}); q.cam(BA_PINHOLE, {});
  q.sensor(true); q.sensor(false);
  for (int j = 0; j < 100; ++j) q.point(j % 10 == 9);
  for (int r = 0; r < 4; ++r)
    for (int j = 0; j < 100; ++j) {
      const int frame = (j + r / 2) % 5;
      if (r < 2 || j % 3 == 0) q.obs(frame, (r % 2 && j % 7 == 0) ? 1 : 0, j, j % 11 == 0 ? -1 : r % 2);
    }
  const Layout L = make_layout(q.get(), params());
  check_orders(q, L, 0, 1, false);
  // quadratic count over the observations of a point
  long long paired = 0, paired_kind[3] = {0, 0, 0};
  for (int a = 0; a < L.n; ++a) {
    const int64_t o = L.obs_of_a[a];
    int same[3] = {0, 0, 0};
    for (int a2 = 0; a2 < L.n; ++a2) {
      const int64_t o2 = L.obs_of_a[a2];
      if (q.ox[o2] != q.ox[o]) continue;
      same[0] += q.op[o2] == q.op[o];
      same[1] += q.oc[o2] == q.oc[o];
      same[2] += q.os[o] >= 0 && q.os[o2] == q.os[o];
    }
    const int want = (same[0] == 1 ? 1 : 0) | (same[1] == 1 ? 2 : 0) | (same[2] <= 1 ? 4 : 0);
    CHECK(L.solo[L.a2c[a]] == want);
    const bool variable[3] = {!q.pose_const[q.op[o]], q.nvar(q.oc[o]) > 0, q.os[o] >= 0 && !q.sensor_const[q.os[o]]};
    for (int k = 0; k < 3; ++k)
      if (same[k] > 1 && variable[k]) { ++paired; ++paired_kind[k]; }
  }
  CHECK(L.n_paired == paired && paired > 0);
  for (int k = 0; k < 3; ++k) CHECK(L.n_paired_kind[k] == paired_kind[k] && paired_kind[k] > 0);
  // a_boff of each kind
  for (int a = 0; a < L.n; ++a) {
    const int64_t o = L.obs_of_a[a];
    CHECK(L.a_boff[0][a] == L.pose_off[q.op[o]] && L.a_boff[1][a] == L.cam_off[q.oc[o]]);
    CHECK(L.a_boff[2][a] == (q.os[o] >= 0 ? L.sens_off[q.os[o]] : -1));
  }
  // the pair incidences as a set of (block, point, members)
  typedef std::tuple<int, int, std::vector<int>> Key;
  std::set<Key> want, got;
  for (int j = 0; j < q.p.num_points; ++j) {
    if (q.point_const[j]) continue;
    std::map<int, std::vector<int>> of_block;
    for (int a = 0; a < L.n; ++a) {
      const int64_t o = L.obs_of_a[a];
      if (q.ox[o] != j) continue;
      for (int b : {L.blk_of_pose[q.op[o]], L.blk_of_cam[q.oc[o]], q.os[o] >= 0 ? L.blk_of_sens[q.os[o]] : -1})
        if (b >= 0) of_block[b].push_back(a);
    }
    for (const auto& kv : of_block)
      if (kv.second.size() >= 2) want.insert(Key(kv.first, j, kv.second));
  }
  const Incidences& I = L.pairs;
  for (int i = 0; i < I.n(); ++i) {
    std::vector<int> mem(I.obs.begin() + I.ptr[i], I.obs.begin() + I.ptr[i + 1]);
    std::sort(mem.begin(), mem.end());
    CHECK(got.insert(Key(I.blk[i], I.pt[i], mem)).second);
  }
  CHECK(got == want && !want.empty());
  CHECK(I.ptr.back() == (int)I.obs.size());
  check_incidence_chunks(I, L.n_blk(), 32);
  CHECK(I.chunk_blk.size() > I.blocks.size());  // some block has more than one chunk
  LayoutParams off = params();
  off.pair_incidences = false;
  const Layout Loff = make_layout(q.p, off);
  CHECK(Loff.pairs.n() == 0 && Loff.pairs.obs.empty() && Loff.n_paired == paired && Loff.a_boff[1] == L.a_boff[1]);
}

void test_image_sharding(int world, int inc_chunk) {
  Prob q;
  mixed_problem(q, 50);
  // keys (point, variable-intrinsics camera) of the active observations of variable points, and the ranks they sit on
  std::map<std::pair<int, int>, std::set<int>> ranks;
  for (int64_t o = 0; o < q.p.num_obs; ++o)
    if (q.active(o) && q.nvar(q.oc[o]) > 0 && !q.point_const[q.ox[o]]) ranks[{q.ox[o], q.oc[o]}].insert(q.op[o] % world);
  std::vector<Layout> Ls;
  for (int r = 0; r < world; ++r) {
    LayoutParams P = params(r, world, false);
    P.inc_chunk = inc_chunk;
    Ls.push_back(make_layout(q.p, P));
    check_orders(q, Ls[r], r, world, false);
    CHECK(Ls[r].pairs.n() == 0);
  }
  std::vector<std::tuple<int, int, int>> want;  // (block, point, camera): the device order
  for (const auto& kv : ranks)
    if (kv.second.size() > 1) want.emplace_back(Ls[0].blk_of_cam[kv.first.second], kv.first.first, kv.first.second);
  std::sort(want.begin(), want.end());
  CHECK(!want.empty());
  std::vector<std::set<int64_t>> seen(want.size());
  for (int r = 0; r < world; ++r) {
    const Layout& L = Ls[r];
    const Incidences& I = L.inc;
    CHECK(I.n() == (int)want.size());
    CHECK(I.pt == Ls[0].inc.pt && I.blk == Ls[0].inc.blk && L.blk_of_cam == Ls[0].blk_of_cam);
    for (int i = 0; i < I.n(); ++i) {
      CHECK(I.blk[i] == std::get<0>(want[i]) && I.pt[i] == std::get<1>(want[i]));
      for (int k = I.ptr[i]; k < I.ptr[i + 1]; ++k) {
        const int64_t o = obs_of_c(L, I.obs[k]);
        CHECK(q.ox[o] == std::get<1>(want[i]) && q.oc[o] == std::get<2>(want[i]) && q.op[o] % world == r);
        CHECK(seen[i].insert(o).second);  // the ranks' lists are disjoint
      }
    }
    check_incidence_chunks(I, L.n_blk(), inc_chunk);
  }
  for (size_t i = 0; i < want.size(); ++i) {
    std::set<int64_t> all;
    for (int64_t o = 0; o < q.p.num_obs; ++o)
      if (q.active(o) && q.ox[o] == std::get<1>(want[i]) && q.oc[o] == std::get<2>(want[i])) all.insert(o);
    CHECK(seen[i] == all);
  }
  // point sharding: a point's observations sit on one rank, nothing spans
  for (int r = 0; r < world; ++r) {
    const Layout L = make_layout(q.p, params(r, world, true));
    check_orders(q, L, r, world, true);
    for (int64_t o : L.obs_of_a) CHECK(q.ox[o] % world == r);
    CHECK(L.inc.n() == 0 && L.inc.obs.empty());
  }
}

void test_priors() {
  Prob q;
  const int p_var = q.pose(), p_const = q.pose(true), p_const2 = q.pose(true), p_var2 = q.pose();
  q.cam(BA_PINHOLE, {});
  const int s_var = q.sensor(false), s_const = q.sensor(true);
  for (int j = 0; j < 4; ++j) q.point(true);
  q.obs(p_var, 0, 0); q.obs(p_const, 0, 1, s_var); q.obs(p_const2, 0, 2, s_const); q.obs(p_var2, 0, 3, s_var);
  q.prior(p_var2, s_var);      // both blocks variable
  q.prior(p_const2, s_const);  // nothing variable: dropped
  q.prior(p_const, s_var);     // constant pose, variable sensor
  q.prior(p_var, -1);
  q.prior(p_const2, -1);       // dropped
  const Layout L = make_layout(q.get(), params());
  const int kept[3] = {0, 2, 3};
  CHECK(L.n_priors() == 3);
  for (int k = 0; k < 3; ++k) {
    const int src = kept[k], pi = q.prior_pose[src], si = q.prior_sensor[src];
    CHECK(L.pr_pose[k] == pi && L.pr_sens[k] == si);
    CHECK(L.pr_po[k] == L.pose_off[pi] && L.pr_so[k] == (si >= 0 ? L.sens_off[si] : -1));
    CHECK(L.pr_pdim[k] == (L.pose_off[pi] >= 0 ? 6 : 0));
    for (int c = 0; c < 3; ++c) CHECK(L.pr_pos[3 * k + c] == q.prior_pos[3 * src + c]);
    for (int c = 0; c < 9; ++c) CHECK(L.pr_A[9 * k + c] == q.prior_A[9 * src + c]);
  }
  CHECK(L.pr_po[1] == -1 && L.pr_so[1] >= 0 && L.pr_so[3 - 1] == -1);
  // targets (block, prior, first column), grouped by block in prior order
  std::vector<std::array<int, 3>> want;
  for (int b = 0; b < L.n_blk(); ++b)
    for (int k = 0; k < 3; ++k) {
      if (L.blk_of_pose[L.pr_pose[k]] == b) want.push_back({b, k, 0});
      if (L.pr_sens[k] >= 0 && L.blk_of_sens[L.pr_sens[k]] == b) want.push_back({b, k, L.pr_pdim[k]});
    }
  CHECK(want.size() == 4 && L.tg_prior.size() == 4 && L.tg_base.size() == 4);
  CHECK(L.tb_blk.size() == 3 && L.tb_ptr.size() == 4 && L.tb_ptr[0] == 0 && L.tb_ptr[3] == 4);
  for (size_t t = 0; t < L.tb_blk.size(); ++t) {
    CHECK(L.tb_ptr[t] < L.tb_ptr[t + 1]);
    if (t > 0) CHECK(L.tb_blk[t - 1] < L.tb_blk[t]);
    for (int e = L.tb_ptr[t]; e < L.tb_ptr[t + 1]; ++e)
      CHECK(L.tb_blk[t] == want[e][0] && L.tg_prior[e] == want[e][1] && L.tg_base[e] == want[e][2]);
  }
  CHECK(L.tg_base[L.tb_ptr[2]] == 6 && L.tg_base[L.tb_ptr[2] + 1] == 0);  // the sensor block: after a 6-wide / a constant pose
}

template <typename F>
void expect_throw(const char* message, F&& make) {
  Prob q;
  q.pose(); q.pose(); q.cam(BA_PINHOLE, {0}); q.point(); q.sensor(false);
  q.obs(0, 0, 0, 0); q.obs(1, 0, 0, -1);
  q.prior(0, -1);
  q.get();
  make(q);
  try {
    make_layout(q.p, params());
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).rfind(message, 0) == 0) return;
    std::fprintf(stderr, "wrong message: %s (wanted: %s)\n", e.what(), message);
    std::exit(1);
  }
  std::fprintf(stderr, "no exception: %s\n", message);
  std::exit(1);
}

void test_errors() {
  expect_throw("observation index out of range", [](Prob& q) { q.ox[1] = 1; });
  expect_throw("observation index out of range", [](Prob& q) { q.op[0] = -1; });
  expect_throw("observation sensor index out of range", [](Prob& q) { q.os[1] = 1; });
  expect_throw("prior index out of range", [](Prob& q) { q.prior_pose[0] = 2; });
  expect_throw("prior index out of range", [](Prob& q) { q.prior_sensor[0] = 1; });
  expect_throw("pose_fixed_t out of range", [](Prob& q) { q.fixed_t[1] = 8; });
  expect_throw("pose_fixed_t out of range", [](Prob& q) { q.fixed_t[0] = -2; });
  expect_throw("unsupported camera model id 99 (supported: SIMPLE_PINHOLE,", [](Prob& q) { q.model[0] = 99; });
  expect_throw("num_priors < 0", [](Prob& q) { q.p.num_priors = -1; });
}

}  // namespace

int main() {
  test_orders();
  test_tangent_layout();
  test_chunks();
  test_tiles();
  test_solo_and_pairs();
  for (int world : {2, 3})
    for (int inc_chunk : {128, 8}) test_image_sharding(world, inc_chunk);
  test_priors();
  test_errors();
  std::printf("layout checks OK\n");
  return 0;
}
