// ba_layout.h -- the index layout of a bundle-adjustment solve, built on the host: which observations are active, the
// two observation orders, point tiles, the tangent space, chunks of the camera-side blocks, prior targets and the
// (point, block) incidences. Plain C++17: no HIP runtime, no switches, no device calls -- Solver::build
// (ba_kernels.hip) calls make_layout(), uploads what it returns and keeps the small maps; tests/cpp/test_ba_layout.cc
// checks it without a GPU.
#ifndef COLMAP_AMD_BA_LAYOUT_H_
#define COLMAP_AMD_BA_LAYOUT_H_

#include "../../include/colmap_amd/camera_models.hpp"
#include "../../include/colmap_amd_ba.h"

#include <algorithm>
#include <array>
#include <cstdint>
#include <functional>
#include <numeric>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

namespace ba_layout {

namespace models = colmap_amd::camera_models;

// The BA_* ids are ABI (colmap_amd_ba.h); the table is where everything else about a model is read.
#define BA_SAME_ID(name) static_assert(int(BA_##name) == int(models::name), "colmap_amd_ba.h and camera_models.hpp disagree on " #name)
BA_SAME_ID(SIMPLE_PINHOLE); BA_SAME_ID(PINHOLE); BA_SAME_ID(SIMPLE_RADIAL); BA_SAME_ID(RADIAL); BA_SAME_ID(OPENCV);
BA_SAME_ID(OPENCV_FISHEYE); BA_SAME_ID(FULL_OPENCV); BA_SAME_ID(FOV); BA_SAME_ID(SIMPLE_RADIAL_FISHEYE);
BA_SAME_ID(RADIAL_FISHEYE); BA_SAME_ID(THIN_PRISM_FISHEYE); BA_SAME_ID(RAD_TAN_THIN_PRISM_FISHEYE);
BA_SAME_ID(SIMPLE_DIVISION); BA_SAME_ID(DIVISION); BA_SAME_ID(SIMPLE_FISHEYE); BA_SAME_ID(FISHEYE); BA_SAME_ID(EUCM);
BA_SAME_ID(EQUIRECTANGULAR);
#undef BA_SAME_ID
static_assert(models::kNumModels == 18, "a model without a BA_* id");
static_assert(BA_CAM_STRIDE == models::kMaxParams, "BA_CAM_STRIDE holds the largest model");

// Host-side set-up loops over the observations (gathers into the device orders: random reads that one core serves at
// a cache miss a time): contiguous index ranges on up to 16 threads. fn(begin, end, thread).
template <typename F>
inline void host_parallel_for(int64_t n, F&& fn) {
  const int64_t grain = 1 << 16;
  int T = (int)std::min<int64_t>(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u), (n + grain - 1) / grain);
  if (T <= 1) {
    fn((int64_t)0, n, 0);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(T);
  for (int t = 0; t < T; ++t) th.emplace_back([&, t] { fn(n * t / T, n * (t + 1) / T, t); });
  for (auto& x : th) x.join();
}

// What the layout depends on besides the problem. The solver fills every field (its constants and switches).
struct LayoutParams {
  int rank = 0, world = 1;
  bool by_point = false;        // observations sharded by 3-D point instead of by image
  int chunk = 0;                // c-order observations per camera-side reduction chunk (used rounded down to even)
  int heavy_chunks = 0;         // a block with more chunks than this is heavy
  int tile_pts = 0, tile_obs = 0;  // a point tile holds at most this many points / observations
  int inc_chunk = 0, pair_chunk = 0;  // incidences of one block per chunk: spanning / pair incidences
  bool pair_incidences = true;  // build the pair incidences (single rank only)
  std::function<void(const char*)> stage;  // optional: called with a stage's name when the stage is done
};

// (point, block) incidences sorted by block, each with a CSR list of observations; a block's run is cut into chunks
struct Incidences {
  std::vector<int> pt, blk;   // [n]
  std::vector<int> ptr, obs;  // [n + 1], the observations of incidence i: obs[ptr[i] .. ptr[i + 1])
  std::vector<int> chunk_blk, chunk_beg;  // [n_chunks], [n_chunks + 1]: chunk c = incidences [chunk_beg[c], chunk_beg[c + 1])
  std::vector<int> blk_chunk;             // [n_blk + 1] chunks of every block
  std::vector<int> blocks;                // the blocks that have incidences, ascending
  int n() const { return (int)pt.size(); }
};

// Width tiers of a problem: at most 4 variable intrinsics per camera; at most KD_MAX; more, or a model with more than
// NPAR parameters
enum TierId { TIER_NARROW, TIER_MAX, TIER_WIDE };
constexpr int KD_MAX = 8;
constexpr int NPAR = 8;  // max number of parameters of a camera model of the two narrower tiers (J_params is 2 x NPAR)

struct Layout {
  // tier inputs
  std::vector<int> cam_nvar;  // [num_cams] variable intrinsics
  std::vector<int> cam_var;   // [num_cams][BA_CAM_STRIDE] their parameter indices
  int max_nvar = 0, max_npar = 0;
  // blocks some active observation (of any rank) uses
  std::vector<char> pose_used, cam_used, pt_used, sens_used;
  // orders. p-order: this rank's active observations, stable by point; c-order: stable by (camera, pose)
  int n = 0;                      // this rank's active observations
  int64_t n_active_global = 0;    // all ranks'
  bool has_sensors = false;
  std::vector<int64_t> obs_of_a;  // [n] p-order slot -> caller observation
  std::vector<int> pt_ptr;        // [num_points + 1] p-order range of a point
  std::vector<int> c2a, a2c;      // [n] c-order position <-> p-order position
  std::vector<int> a_pose, a_cam, a_pt, a_sensor, o_pose, o_cam, o_pt, o_sensor;  // topology in p-order / c-order
  std::vector<double> a_xy, o_xy;
  std::vector<unsigned char> solo;  // c-order: bit k set = no other observation of this point shares block kind k
  long long n_paired = 0;  // (observation, block kind) slots that have a partner of the same point in the block
  long long n_paired_kind[3] = {0, 0, 0};
  std::vector<int> tile_pt;  // points [tile_pt[t], tile_pt[t + 1]) form tile t; {0}: some track is longer than a tile
  // tangent space: pose blocks, then intrinsics blocks, then variable sensor_from_rig blocks; points apart
  std::vector<int> pose_off, pose_dim, pose_fix, cam_off, cam_dim, sens_off, pt_off;  // offsets: -1 = no block
  std::vector<int> blk_off, blk_dim, blk_kind, blk_moff;
  std::vector<int> blk_of_pose, blk_of_cam, blk_of_sens;
  int n_c = 0, n_p = 0, moff_total = 0, n_var_sensors = 0;
  // chunks: c-order ranges of one block each
  std::vector<int> chunk_blk, chunk_beg, chunk_end, blk_chunk_ptr, blk_fin_end, heavy;
  // position priors with a variable block, and their targets (block, prior, first column) grouped by block
  std::vector<int> pr_pose, pr_sens, pr_po, pr_so, pr_pdim;
  std::vector<double> pr_pos, pr_A;
  std::vector<int> tb_blk, tb_ptr, tg_prior, tg_base;
  // image sharding: (point, intrinsics block) incidences whose observations sit on more than one rank; obs = this
  // rank's observations (c-order)
  Incidences inc;
  // single rank: a_boff[k][a] = tangent offset of p-order observation a's block of kind k (-1: none), for the kinds
  // with pairs; pairs = the incidences with >= 2 observations in the block, obs = their members (p-order)
  std::vector<int> a_boff[3];
  Incidences pairs;

  int n_blk() const { return (int)blk_off.size(); }
  int n_priors() const { return (int)pr_pose.size(); }

  // Frees everything sized by the observations, chunks or incidences; the per-block and per-point maps stay.
  // keep_obs_maps: obs_of_a and a2c stay too.
  void release_observation_arrays(bool keep_obs_maps) {
    auto drop = [](auto&... v) { (std::decay_t<decltype(v)>().swap(v), ...); };
    drop(pt_ptr, c2a, a_pose, a_cam, a_pt, a_sensor, o_pose, o_cam, o_pt, o_sensor, a_xy, o_xy, solo, tile_pt);
    drop(chunk_blk, chunk_beg, chunk_end, blk_chunk_ptr, blk_fin_end, heavy, a_boff[0], a_boff[1], a_boff[2]);
    inc = Incidences{};
    pairs = Incidences{};
    if (!keep_obs_maps) drop(obs_of_a, a2c);
  }
};

inline int pick_tier(const Layout& L) {
  // a 12-parameter model takes the wide tier whatever its number of variable intrinsics (only that tier evaluates
  // 12 J_params columns)
  return L.max_npar > NPAR || L.max_nvar > KD_MAX ? TIER_WIDE : (L.max_nvar <= 4 ? TIER_NARROW : TIER_MAX);
}

inline bool sensor_variable(const ba_problem& p, int64_t o) {
  const int sv = p.obs_sensor ? p.obs_sensor[o] : -1;
  return sv >= 0 && p.sensor_const != nullptr && !p.sensor_const[sv];
}
// An observation is active when at least one of its blocks is variable. cam_nvar: [num_cams] variable intrinsics.
inline bool is_active(const ba_problem& p, const int* cam_nvar, int64_t o) {
  return !(p.pose_const[p.obs_pose[o]] && cam_nvar[p.obs_cam[o]] == 0 && p.point_const[p.obs_point[o]] &&
           !sensor_variable(p, o));
}

// 1. camera models and their variable intrinsics
inline void count_variable_intrinsics(const ba_problem& p, Layout& L) {
  L.cam_nvar.assign(p.num_cams, 0);
  L.cam_var.assign((size_t)p.num_cams * BA_CAM_STRIDE, 0);
  for (int k = 0; k < p.num_cams; ++k) {
    const int model = p.cam_model[k];
    const int P = models::num_params(model);
    if (P < 0)
      throw std::runtime_error("unsupported camera model id " + std::to_string(model) +
                               " (supported: SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, "
                               "OPENCV_FISHEYE, FOV, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE, SIMPLE_DIVISION, "
                               "DIVISION, SIMPLE_FISHEYE, FISHEYE, EUCM, FULL_OPENCV, THIN_PRISM_FISHEYE, "
                               "RAD_TAN_THIN_PRISM_FISHEYE, EQUIRECTANGULAR)");
    for (int j = 0; j < P; ++j)
      if (!p.cam_const[(size_t)k * BA_CAM_STRIDE + j]) L.cam_var[(size_t)k * BA_CAM_STRIDE + L.cam_nvar[k]++] = j;
    L.max_nvar = std::max(L.max_nvar, L.cam_nvar[k]);
    L.max_npar = std::max(L.max_npar, P);
  }
}

// 2. the active observations: all ranks' mark their blocks as used (the layout is the same on every rank), this
// rank's go into obs_of_a in the caller's order
inline void scan_active(const ba_problem& p, const LayoutParams& P, Layout& L) {
  L.obs_of_a.reserve(p.num_obs / P.world + 1);
  L.pose_used.assign(p.num_poses, 0); L.cam_used.assign(p.num_cams, 0); L.pt_used.assign(p.num_points, 0);
  L.sens_used.assign(std::max(p.num_sensors, 0) + 1, 0);
  for (int64_t o = 0; o < p.num_obs; ++o) {
    const int pi = p.obs_pose[o], ci = p.obs_cam[o], xi = p.obs_point[o];
    if (pi < 0 || pi >= p.num_poses || ci < 0 || ci >= p.num_cams || xi < 0 || xi >= p.num_points)
      throw std::runtime_error("observation index out of range");
    if (p.obs_sensor && (p.obs_sensor[o] < -1 || p.obs_sensor[o] >= p.num_sensors))
      throw std::runtime_error("observation sensor index out of range");
    if (!is_active(p, L.cam_nvar.data(), o)) continue;
    ++L.n_active_global;
    L.pose_used[pi] = L.cam_used[ci] = L.pt_used[xi] = 1;
    if (sensor_variable(p, o)) L.sens_used[p.obs_sensor[o]] = 1;
    // image sharding (BASELINE.json: "images shard across the GPUs") or point sharding (every
    // observation of a point on one rank: the point-side quantities stay local)
    if ((P.by_point ? xi : pi) % P.world == P.rank) L.obs_of_a.push_back(o);
  }
  L.n = (int)L.obs_of_a.size();
}

// 3. The two orders of the observations, by stable COUNTING sorts (the keys are block indices; comparison sorts of
// 2 M ... 20 M observations were most of the 0.3 s ... 5.5 s a solve spent before its first kernel)
inline void sort_orders(const ba_problem& p, Layout& L) {
  const int n = L.n;
  std::vector<int64_t>& active = L.obs_of_a;
  // p-order: sorted by point (stable: keeps the caller's order inside a track)
  L.pt_ptr.assign(p.num_points + 1, 0);
  for (int a = 0; a < n; ++a) L.pt_ptr[p.obs_point[active[a]] + 1]++;
  for (int j = 0; j < p.num_points; ++j) L.pt_ptr[j + 1] += L.pt_ptr[j];
  {
    std::vector<int> cursor(L.pt_ptr.begin(), L.pt_ptr.end() - 1);
    std::vector<int64_t> sorted((size_t)n);
    for (int a = 0; a < n; ++a) sorted[(size_t)cursor[p.obs_point[active[a]]]++] = active[a];
    active.swap(sorted);
  }
  // c-order: p-order positions sorted by (camera, pose) -> every camera-side block is a range. Least significant
  // key first: stable by pose, then stable by camera; ties keep the p-order (what std::stable_sort on the pair gave).
  L.c2a.resize(n); L.a2c.resize(n);
  std::vector<int> by_pose((size_t)n), cnt((size_t)std::max(p.num_poses, p.num_cams) + 1, 0);
  for (int a = 0; a < n; ++a) cnt[(size_t)p.obs_pose[active[a]] + 1]++;
  for (int i = 0; i < p.num_poses; ++i) cnt[(size_t)i + 1] += cnt[i];
  for (int a = 0; a < n; ++a) by_pose[(size_t)cnt[p.obs_pose[active[a]]]++] = a;
  std::fill(cnt.begin(), cnt.end(), 0);
  for (int a = 0; a < n; ++a) cnt[(size_t)p.obs_cam[active[a]] + 1]++;
  for (int k = 0; k < p.num_cams; ++k) cnt[(size_t)k + 1] += cnt[k];
  for (int i = 0; i < n; ++i) {
    const int a = by_pose[i];
    L.c2a[(size_t)cnt[p.obs_cam[active[a]]]++] = a;
  }
  for (int c = 0; c < n; ++c) L.a2c[L.c2a[c]] = c;
}

// 4. point tiles for the LDS-staged point passes
inline void cut_point_tiles(const ba_problem& p, const LayoutParams& P, Layout& L) {
  bool ok = true;
  int j = 0;
  L.tile_pt.assign(1, 0);
  while (j < p.num_points) {
    int j1 = j, obs = 0;
    while (j1 < p.num_points && j1 - j < P.tile_pts && obs + (L.pt_ptr[j1 + 1] - L.pt_ptr[j1]) <= P.tile_obs) {
      obs += L.pt_ptr[j1 + 1] - L.pt_ptr[j1];
      ++j1;
    }
    if (j1 == j) { ok = false; break; }  // a single track longer than a tile
    L.tile_pt.push_back(j1);
    j = j1;
  }
  if (!ok) L.tile_pt.assign(1, 0);
}

// 5. the topology in p-order (position a <-> c-order position a2c[a]) and in c-order, and the solo flags
inline void copy_topology(const ba_problem& p, Layout& L) {
  const int n = L.n;
  const bool has_sensors = L.has_sensors = p.obs_sensor != nullptr && p.num_sensors > 0 && p.sensors != nullptr;
  const std::vector<int64_t>& active = L.obs_of_a;
  L.a_pose.resize(n); L.a_cam.resize(n); L.a_pt.resize(n); L.a_xy.resize((size_t)2 * n);
  if (has_sensors) L.a_sensor.resize(n);
  host_parallel_for(n, [&](int64_t a0, int64_t a1, int) {
    for (int64_t a = a0; a < a1; ++a) {
      const int64_t o = active[a];
      L.a_pose[a] = p.obs_pose[o];
      L.a_cam[a] = p.obs_cam[o];
      L.a_pt[a] = p.obs_point[o];
      L.a_xy[2 * (size_t)a] = p.obs_xy[2 * o];
      L.a_xy[2 * (size_t)a + 1] = p.obs_xy[2 * o + 1];
      if (has_sensors) L.a_sensor[a] = p.obs_sensor[o];
    }
  });
  // solo flags: does another observation of the same point use the same pose / camera? (a track's entries of the
  // p-order arrays are neighbours in memory: the quadratic loop over a track stays in cache)
  L.solo.assign(n, 0);
  long long paired_t[16][4] = {};  // per thread: n_paired, n_paired_kind[0..2]
  host_parallel_for(p.num_points, [&](int64_t j0, int64_t j1, int t) {
    long long* acc = paired_t[t];
    for (int64_t j = j0; j < j1; ++j)
      for (int a = L.pt_ptr[j]; a < L.pt_ptr[j + 1]; ++a) {
        int same_pose = 0, same_cam = 0, same_sens = 0;
        const int sa = has_sensors ? L.a_sensor[a] : (p.obs_sensor ? p.obs_sensor[active[a]] : -1);
        const int pose_a = L.a_pose[a], cam_a = L.a_cam[a];
        for (int a2 = L.pt_ptr[j]; a2 < L.pt_ptr[j + 1]; ++a2) {
          same_pose += L.a_pose[a2] == pose_a;
          same_cam += L.a_cam[a2] == cam_a;
          same_sens += sa >= 0 && (has_sensors ? L.a_sensor[a2] : p.obs_sensor[active[a2]]) == sa;
        }
        L.solo[L.a2c[a]] = (unsigned char)((same_pose == 1 ? 1 : 0) | (same_cam == 1 ? 2 : 0) | (same_sens <= 1 ? 4 : 0));
        const int k0 = same_pose != 1 && !p.pose_const[pose_a];
        const int k1 = same_cam != 1 && L.cam_nvar[cam_a] > 0;
        const int k2 = same_sens > 1 && L.sens_used[sa];
        acc[0] += k0 + k1 + k2;
        acc[1] += k0;
        acc[2] += k1;
        acc[3] += k2;
      }
  });
  for (int t = 0; t < 16; ++t) {
    L.n_paired += paired_t[t][0];
    for (int k = 0; k < 3; ++k) L.n_paired_kind[k] += paired_t[t][1 + k];
  }
  L.o_pose.resize(n); L.o_cam.resize(n); L.o_pt.resize(n); L.o_xy.resize((size_t)2 * n);
  if (has_sensors) L.o_sensor.resize(n);
  host_parallel_for(n, [&](int64_t c0, int64_t c1, int) {
    for (int64_t c = c0; c < c1; ++c) {
      const int a = L.c2a[c];   // c-order from the p-order copies: one indirection, 4-byte indices
      if (has_sensors) L.o_sensor[c] = L.a_sensor[a];
      L.o_pose[c] = L.a_pose[a];
      L.o_cam[c] = L.a_cam[a];
      L.o_pt[c] = L.a_pt[a];
      L.o_xy[2 * (size_t)c] = L.a_xy[2 * (size_t)a];
      L.o_xy[2 * (size_t)c + 1] = L.a_xy[2 * (size_t)a + 1];
    }
  });
}

// 6. tangent layout: pose blocks, then intrinsics blocks, then variable sensor_from_rig blocks (camera side); points
inline void lay_out_tangent_space(const ba_problem& p, Layout& L) {
  L.pose_off.assign(p.num_poses, -1); L.pose_dim.assign(p.num_poses, 0); L.pose_fix.assign(p.num_poses, -1);
  L.cam_off.assign(p.num_cams, -1); L.cam_dim.assign(p.num_cams, 0);
  L.pt_off.assign(p.num_points, -1);
  L.blk_of_pose.assign(p.num_poses, -1); L.blk_of_cam.assign(p.num_cams, -1);
  int off = 0, moff = 0;
  auto add_block = [&](int kind, int dim) {
    L.blk_off.push_back(off); L.blk_dim.push_back(dim); L.blk_kind.push_back(kind); L.blk_moff.push_back(moff);
    off += dim;
    moff += dim * dim;
    return L.n_blk() - 1;
  };
  for (int i = 0; i < p.num_poses; ++i) {
    if (p.pose_const[i] || !L.pose_used[i]) continue;
    const int pf = p.pose_fixed_t[i];
    if (pf < -1 || pf > 7) throw std::runtime_error("pose_fixed_t out of range");
    L.pose_fix[i] = pf;
    L.pose_dim[i] = (pf >= 4 ? 0 : 3) + ((pf >= 0 && (pf & 3) != 3) ? 2 : 3);
    L.pose_off[i] = off;
    L.blk_of_pose[i] = add_block(0, L.pose_dim[i]);
  }
  for (int k = 0; k < p.num_cams; ++k) {
    if (L.cam_nvar[k] == 0 || !L.cam_used[k]) continue;
    L.cam_dim[k] = L.cam_nvar[k];
    L.cam_off[k] = off;
    L.blk_of_cam[k] = add_block(1, L.cam_nvar[k]);
  }
  // variable sensor_from_rig blocks (RigReprojErrorCostFunctor's cam_from_rig parameter block,
  // bundle_adjustment_ceres.cc:804-812): full 6-dimensional pose tangent, block kind 2
  L.sens_off.assign(std::max(p.num_sensors, 0), -1);
  L.blk_of_sens.assign(std::max(p.num_sensors, 0), -1);
  for (int sidx = 0; sidx < p.num_sensors; ++sidx) {
    if (!L.sens_used[sidx]) continue;
    L.sens_off[sidx] = off;
    L.blk_of_sens[sidx] = add_block(2, 6);
    ++L.n_var_sensors;
  }
  L.n_c = off;
  L.moff_total = moff;
  for (int j = 0; j < p.num_points; ++j) {
    if (p.point_const[j] || !L.pt_used[j]) continue;
    L.pt_off[j] = L.n_p;
    L.n_p += 3;
  }
}

// 7. per-block c-order runs, split into chunks. A camera's observations are one run (c-order is sorted by camera
// first); a pose seen through several cameras (a rig frame) owns one run per camera. Every chunk is a contiguous
// range of one block. A block with more than heavy_chunks chunks is heavy.
inline void cut_chunks(const LayoutParams& P, Layout& L) {
  const int n_blk = L.n_blk();
  std::vector<std::vector<std::pair<int, int>>> runs(n_blk);
  auto add_run = [&](int b, int c) {
    if (b < 0) return;
    auto& r = runs[b];
    if (!r.empty() && r.back().second == c) r.back().second = c + 1;
    else r.emplace_back(c, c + 1);
  };
  for (int c = 0; c < L.n; ++c) {
    add_run(L.blk_of_pose[L.o_pose[c]], c);
    add_run(L.blk_of_cam[L.o_cam[c]], c);
    if (L.has_sensors && L.o_sensor[c] >= 0) add_run(L.blk_of_sens[L.o_sensor[c]], c);
  }
  const int CHUNK = P.chunk & ~1;  // even: the MFMA Gram kernel consumes observation pairs
  L.blk_chunk_ptr.assign(n_blk + 1, 0);
  for (int b = 0; b < n_blk; ++b) {
    L.blk_chunk_ptr[b] = (int)L.chunk_blk.size();
    for (const auto& run : runs[b])
      for (int s = run.first; s < run.second; s += CHUNK) {
        L.chunk_blk.push_back(b);
        L.chunk_beg.push_back(s);
        L.chunk_end.push_back(std::min(s + CHUNK, run.second));
      }
  }
  L.blk_chunk_ptr[n_blk] = (int)L.chunk_blk.size();
  L.blk_fin_end.assign(std::max(n_blk, 1), 0);
  for (int b = 0; b < n_blk; ++b) {
    const bool heavy = L.blk_chunk_ptr[b + 1] - L.blk_chunk_ptr[b] > P.heavy_chunks;
    L.blk_fin_end[b] = heavy ? L.blk_chunk_ptr[b] + 1 : L.blk_chunk_ptr[b + 1];
    if (heavy) L.heavy.push_back(b);
  }
}

// 8. position priors whose pose or sensor_from_rig block is variable
inline void collect_priors(const ba_problem& p, Layout& L) {
  std::vector<std::array<int, 3>> targets;  // block, prior, first column
  if (p.num_priors < 0) throw std::runtime_error("num_priors < 0");
  for (int k = 0; k < p.num_priors; ++k) {
    const int pi = p.prior_pose[k];
    const int si = p.prior_sensor ? p.prior_sensor[k] : -1;
    if (pi < 0 || pi >= p.num_poses || si < -1 || si >= p.num_sensors) throw std::runtime_error("prior index out of range");
    const int po = L.pose_off[pi], so = si >= 0 ? L.sens_off[si] : -1;
    if (po < 0 && so < 0) continue;
    const int kk = L.n_priors();
    const int pdim = po >= 0 ? L.pose_dim[pi] : 0;
    L.pr_pose.push_back(pi); L.pr_sens.push_back(si); L.pr_po.push_back(po); L.pr_so.push_back(so); L.pr_pdim.push_back(pdim);
    L.pr_pos.insert(L.pr_pos.end(), p.prior_position + 3 * (size_t)k, p.prior_position + 3 * (size_t)k + 3);
    L.pr_A.insert(L.pr_A.end(), p.prior_sqrt_info + 9 * (size_t)k, p.prior_sqrt_info + 9 * (size_t)k + 9);
    if (po >= 0) targets.push_back({L.blk_of_pose[pi], kk, 0});
    if (so >= 0) targets.push_back({L.blk_of_sens[si], kk, pdim});
  }
  if (L.n_priors() == 0) return;
  if (p.prior_loss_type < BA_LOSS_TRIVIAL || p.prior_loss_type > BA_LOSS_HUBER || !(p.prior_loss_scale > 0.0))
    throw std::runtime_error("prior loss type / scale");
  std::stable_sort(targets.begin(), targets.end(), [](const std::array<int, 3>& a, const std::array<int, 3>& b) { return a[0] < b[0]; });
  for (size_t e = 0; e < targets.size(); ++e) {
    if (e == 0 || targets[e][0] != targets[e - 1][0]) { L.tb_blk.push_back(targets[e][0]); L.tb_ptr.push_back((int)e); }
    L.tg_prior.push_back(targets[e][1]);
    L.tg_base.push_back(targets[e][2]);
  }
  L.tb_ptr.push_back((int)targets.size());
}

// Chunks of at most max_len incidences of one block (I.blk is sorted), every block's range of chunks, and the blocks
// that have any
inline void chunk_incidences(Incidences& I, int n_blk, int max_len) {
  const int ni = I.n();
  I.blk_chunk.assign(n_blk + 1, 0);
  for (int i = 0; i < ni;) {
    int e = i;
    while (e < ni && I.blk[e] == I.blk[i] && e - i < max_len) ++e;
    if (I.blocks.empty() || I.blocks.back() != I.blk[i]) I.blocks.push_back(I.blk[i]);
    I.chunk_blk.push_back(I.blk[i]);
    I.chunk_beg.push_back(i);
    I.blk_chunk[I.blk[i] + 1]++;
    i = e;
  }
  I.chunk_beg.push_back(ni);
  for (int b = 0; b < n_blk; ++b) I.blk_chunk[b + 1] += I.blk_chunk[b];
}

// 9. Image sharding: (point, intrinsics block) incidences whose observations sit on more than one rank -- the
// pairs the local Schur-Jacobi terms cannot see (ba_inc_* kernels). Every rank walks the whole problem, so all
// ranks build the same list in the same order; a rank's own observations of an incidence go into a CSR list.
inline void build_spanning_incidences(const ba_problem& p, const LayoutParams& P, Layout& L) {
  if (P.world <= 1 || P.by_point) return;
  // global pass: per (point, camera) the set of ranks that hold an observation of it
  std::vector<std::pair<long long, int>> keys;  // (point * num_cams + cam, rank)
  for (int64_t o = 0; o < p.num_obs; ++o) {
    const int pi = p.obs_pose[o], ci = p.obs_cam[o], xi = p.obs_point[o];
    if (!is_active(p, L.cam_nvar.data(), o)) continue;
    if (L.cam_nvar[ci] == 0 || p.point_const[xi]) continue;  // no coupling through this block
    keys.emplace_back((long long)xi * p.num_cams + ci, pi % P.world);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  std::vector<long long> spanning;
  for (size_t k = 0; k + 1 < keys.size(); ++k)
    if (keys[k].first == keys[k + 1].first && (spanning.empty() || spanning.back() != keys[k].first))
      spanning.push_back(keys[k].first);
  if (spanning.empty()) return;
  const int ni = (int)spanning.size();
  Incidences& I = L.inc;
  I.pt.resize(ni); I.blk.resize(ni); I.ptr.assign(ni + 1, 0);
  // device order of the incidences: by block, then by (point, camera) key -- a block's run is contiguous, so
  // its terms are summed in one fixed order (ba_inc_correct_kernel); `pos` = key-order index -> device index
  std::vector<int> by_blk(ni), pos(ni);
  std::iota(by_blk.begin(), by_blk.end(), 0);
  std::stable_sort(by_blk.begin(), by_blk.end(), [&](int a, int b) {
    return L.blk_of_cam[(int)(spanning[a] % p.num_cams)] < L.blk_of_cam[(int)(spanning[b] % p.num_cams)];
  });
  for (int i = 0; i < ni; ++i) {
    pos[by_blk[i]] = i;
    I.pt[i] = (int)(spanning[by_blk[i]] / p.num_cams);
    I.blk[i] = L.blk_of_cam[(int)(spanning[by_blk[i]] % p.num_cams)];
  }
  // this rank's observations, c-order index c, by incidence
  std::vector<std::pair<int, int>> mine;  // (incidence, c)
  for (int c = 0; c < L.n; ++c) {
    const long long key = (long long)L.o_pt[c] * p.num_cams + L.o_cam[c];
    const auto it = std::lower_bound(spanning.begin(), spanning.end(), key);
    if (it != spanning.end() && *it == key) mine.emplace_back(pos[(int)(it - spanning.begin())], c);
  }
  std::sort(mine.begin(), mine.end());
  for (const auto& m : mine) I.ptr[m.first + 1]++;
  for (int i = 0; i < ni; ++i) I.ptr[i + 1] += I.ptr[i];
  I.obs.reserve(mine.size());
  for (const auto& m : mine) I.obs.push_back(m.second);
  if (I.obs.empty()) I.obs.push_back(0);
  chunk_incidences(I, L.n_blk(), P.inc_chunk);
}

// The p-order block offsets of a kind (0 pose, 1 intrinsics, 2 sensor_from_rig)
inline std::vector<int> block_offsets_of_kind(const Layout& L, int kind) {
  std::vector<int> ab(L.n, -1);
  for (int a = 0; a < L.n; ++a) {
    if (kind == 0) ab[a] = L.pose_off[L.a_pose[a]];
    else if (kind == 1) ab[a] = L.cam_off[L.a_cam[a]];
    else ab[a] = (L.has_sensors && L.a_sensor[a] >= 0) ? L.sens_off[L.a_sensor[a]] : -1;
  }
  return ab;
}

// 10. pairs of observations of one point inside one block: the p-order block offsets of the kinds that have such
// pairs and, on a single rank, the pair incidences themselves, sorted by block (ba_pair_cross_kernel); a sharded
// solve keeps the per-observation kernel for its local pairs (the cross-rank ones are the spanning incidences)
inline void build_pair_incidences(const ba_problem& p, const LayoutParams& P, Layout& L) {
  for (int kind = 0; kind < 3; ++kind)
    if (L.n_paired_kind[kind] > 0) L.a_boff[kind] = block_offsets_of_kind(L, kind);
  if (L.n_paired <= 0 || P.world != 1 || !P.pair_incidences) return;
  const int n_blk = L.n_blk();
  std::vector<int> blk_of_off(std::max(L.n_c, 0) + 1, -1);  // tangent offset -> block
  for (int b = 0; b < n_blk; ++b) blk_of_off[L.blk_off[b]] = b;
  struct Inc { int blk, pt, first, count; };
  std::vector<Inc> incs;
  std::vector<int> members;  // p-order observation indices, grouped per incidence
  std::vector<std::pair<int, int>> grp;  // (block offset, a) of one point and kind
  for (int kind = 0; kind < 3; ++kind) {
    if (L.n_paired_kind[kind] <= 0) continue;
    const std::vector<int>& ab = L.a_boff[kind];
    for (int j = 0; j < p.num_points; ++j) {
      if (L.pt_off[j] < 0) continue;  // a constant point has no C^-1: its observations do not couple
      grp.clear();
      for (int a = L.pt_ptr[j]; a < L.pt_ptr[j + 1]; ++a)
        if (ab[a] >= 0) grp.emplace_back(ab[a], a);
      std::sort(grp.begin(), grp.end());
      for (size_t i = 0; i < grp.size();) {
        size_t e = i;
        while (e < grp.size() && grp[e].first == grp[i].first) ++e;
        if (e - i >= 2) {
          incs.push_back({blk_of_off[grp[i].first], j, (int)members.size(), (int)(e - i)});
          for (size_t k = i; k < e; ++k) members.push_back(grp[k].second);
        }
        i = e;
      }
    }
  }
  if (incs.empty()) return;
  std::stable_sort(incs.begin(), incs.end(), [](const Inc& a, const Inc& b) { return a.blk < b.blk; });
  const int ni = (int)incs.size();
  Incidences& I = L.pairs;
  I.pt.resize(ni); I.blk.resize(ni); I.ptr.assign(ni + 1, 0);
  I.obs.reserve(members.size());
  for (int i = 0; i < ni; ++i) {
    I.pt[i] = incs[i].pt; I.blk[i] = incs[i].blk;
    I.obs.insert(I.obs.end(), members.begin() + incs[i].first, members.begin() + incs[i].first + incs[i].count);
    I.ptr[i + 1] = (int)I.obs.size();
  }
  chunk_incidences(I, n_blk, P.pair_chunk);
}

// The whole layout, in the steps above. The incidences are left out where the solve cannot start (no active
// observation anywhere, or none on this rank).
inline Layout make_layout(const ba_problem& p, const LayoutParams& P) {
  Layout L;
  auto stage = [&](const char* name) { if (P.stage) P.stage(name); };
  count_variable_intrinsics(p, L);
  scan_active(p, P, L);
  stage("scan");
  sort_orders(p, L);
  stage("orders");
  cut_point_tiles(p, P, L);
  copy_topology(p, L);
  stage("topology");
  lay_out_tangent_space(p, L);
  cut_chunks(P, L);
  collect_priors(p, L);
  stage("blocks+chunks");
  if (L.n == 0) return L;
  build_spanning_incidences(p, P, L);
  build_pair_incidences(p, P, L);
  return L;
}

}  // namespace ba_layout

#endif  // COLMAP_AMD_BA_LAYOUT_H_
