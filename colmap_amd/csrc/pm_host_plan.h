// pm_host_plan.h -- everything PatchMatch decides on the host before its device calls: the checks on the caller's
// options and problem, the pose tables of the four sweep directions, the scalar half of a parameter block, the span of
// a problem's packed source images, the order in which slabs are tried when those are re-homed, which problems may
// share a run's launches, the shape of a run (columns per wave, helper wave), the sweep schedule with the parameter
// blocks of a run, and the sizes of its sub-batches. Plain C++17: no HIP runtime, no stream, no switches (their values
// come in as ints) -- pm_api.cpp builds a plan, then does the device work the plan states;
// tests/cpp/test_pm_host_plan.cc checks it without a GPU. This is the first of two layers: WHICH kernels serve a run
// is decided after it by pm_plan_run (PmRunPlan, pm_kernels.hip), which needs the LDS layouts there.
#ifndef COLMAP_AMD_PM_HOST_PLAN_H_
#define COLMAP_AMD_PM_HOST_PLAN_H_

#include "../../include/colmap_amd_pm.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace colmap_amd {

constexpr int kPoseStride = 43;  // K4 R9 T3 C3 P12 invP12 (reference patch_match_cuda.cu:1762)
constexpr int kRngWords = 6;     // XORWOW: x[5] + d

// Packed source images ("footprints": one dword per texel position = its 2 x 2 bilinear neighbourhood) are
// stored as vertical strips of kFpStrip = 16 entries: inside a strip the rows follow each other, 64 bytes each, so
// a 128-byte cache line is a 16 x 2 block of entries and the entry index is
//   (ex / 16) * 16 * rows + 16 * ey + (ex % 16).
// Why strips: (a) the 11 x 11 sweep kernels leave that index to the address unit (swizzled buffer resource,
// pm_kernels.hip: fp_resource), which is what makes 2-D blocking free; (b) the texture-address unit serves a quad
// of lanes in one cycle only when its four addresses lie within 16 bytes (scripts/ubench/gather_rates.hip,
// profiles/r04_ubench_gather_rates.log) -- the taps of a quad are neighbours along x, so wide strip rows keep
// the quads of a warped 11 x 11 window fast (16 x 2: 17-19 cycles per gather instruction in the microbenchmark,
// 8 x 4: 24, lane-per-line: 64) while two rows per line still halve the lines a window touches against a
// row-major image. Entry (ex, ey) holds texel position (ex - kFpRingX, ey - kFpRingY); positions -2 and w (h) are
// the all-zero border ring a clamped tap reads; the ring offsets are one strip / whole lines so that texel (0, 0)
// starts a cache line.
#ifndef PM_FP_STRIP
#define PM_FP_STRIP 16  // entries per strip row: 16 (x 2 rows per 128-byte cache line); measured 8 (x 4): +4.4 %, 32 (x 1): +1.2 % launch time
#endif
constexpr int kFpStrip = PM_FP_STRIP;
constexpr int kFpRingX = kFpStrip, kFpRingY = 4;
inline int pm_fp_width(int w) { return (w + kFpRingX + 1 + kFpStrip - 1) & ~(kFpStrip - 1); }    // entries per row (whole strips)
inline int pm_fp_height(int h) { return (h + kFpRingY + 1 + 3) & ~3; }   // rows (multiple of 4)
inline size_t pm_fp_entries(int w, int h) { return (size_t)pm_fp_width(w) * pm_fp_height(h); }

// Per-sweep kernel parameters (reference SweepOptions, patch_match_cuda.cu:914-931,
// plus the geometry of the virtual rotation).
struct PmParams {
  // geometry
  int W, H;         // un-rotated reference image size
  int rot;          // number of 90-degree CCW rotations of the sweep frame (0..3)
  int S;            // number of source images
  int src_w, src_h; // source slot size (max over sources)
  float fp_xmax, fp_ymax;  // src_w + kFpRingX, src_h + kFpRingY: last used column / row of the packed image
  int fp_rows1;            // rows of the packed image (pm_fp_height), minus one (fp_index)
  int radius, step, ntap1d, ntaps;
  int num_samples;
  int rec_stride;   // floats per pixel record: 4 + 3*S
  int sel_in_off;   // record offset of prev_sel_prob (read)
  int sel_out_off;  // record offset of sel_prob (backward msgs, then written)
  int C;            // image columns per workgroup
  int help;         // waves per column group of the 11 x 11 sweep kernel: 2 = a helper wave shares pass B (pm_sweep_pair_kernel, C = 1)
  int ablate;       // profiling only (COLMAP_AMD_PM_ABLATE): bit 0 skip the NCC task passes, bit 1 skip the
                    // hypothesis generation, bit 2 skip the backward-message pre-pass; results are garbage
  int prune;        // 11 x 11 sweep kernels: 1 = P4 runs in two stages and skips the second-stage evaluations of hypotheses
                    // that can no longer win (sweep_wave_body); 0 = single stage (COLMAP_AMD_PM_PRUNE=0). Same results
  int xcd_map;      // batched launch of the generic kernel: 0 problem = id % batch, 1 neighbouring problems per XCD
  float refK[4];    // rotated {fx, cx, fy, cy}
  float refInvK[4]; // rotated {1/fx, -cx/fx, 1/fy, -cy/fy}
  float perturbation;
  float perturbation_pi;
  float prev_sel_prob_weight;
  float spatial_norm, color_norm;
  float cos_min_tri, inv_inc_sigma_sq, inv_ncc_sigma_sq, ncc_norm;
  float geom_reg, geom_max_cost;
  float filter_min_ncc;
  float filter_cos_min_tri;
  float filter_geom_max_cost;
  int filter_min_num_consistent;
  // device pointers
  float* rec;               // [H*W][rec_stride]
  const uint32_t* const* src_fp_tab;  // [S] pointers to packed 2x2 footprints, pm_fp_entries(src_w, src_h) each
                                      // (separate allocations: shareable between problems)
  const uint32_t* fp_base;            // lowest address among them: base of the problem's buffer resource, or null
  const uint32_t* src_fp_off;         // [S] (address - fp_base) / kFpStrip: the images as slots of that resource
  const float* src_depth;   // [S][src_h][src_w] or null
  const uint8_t* ref_img;   // [H][W]
  const float* ref_sum;     // [H][W]
  const float* ref_sqsum;   // [H][W]
  uint32_t* rng;            // [H*W][6]
  float* draws;             // [rot H][rot W][pm_draw_stride]: the sweep's random numbers per pixel of the sweep frame
                            // (pm_draw_kernel -> 11 x 11 sweep kernel), or null: the generic kernel draws in place
  uint8_t* mask;            // [S][H][W] or null
  const float* poses;       // [S][43] for this rotation
  unsigned long long* prof; // optional phase-cycle counters [kPmProfSlots] (debug), else null
  unsigned long long* evals; // NCC evaluations executed by the sweep kernels of this run (one atomic
                             // add per workgroup at its end), always allocated
  unsigned long long* answered; // [3] of them the 11 x 11 wave kernels answered without taps (pm_patch_class.h): by the
                                // sweep kernels, by the initial cost; [2]: pruned by the sweep kernels (never listed for
                                // stage 2 of P4); one atomic add per wave at its end
  unsigned long long* trace; // optional progress trace (debug, pm_enable_progress_trace): [column group][row / 128]
                             // device-wide clock when the group's wave reached that row, last sweep launch; else null
  int trace_stride;          // samples per column group
};

}  // namespace colmap_amd

namespace pm_host {

using colmap_amd::PmParams;
using colmap_amd::kPoseStride;

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define PM_CHECK(cond, msg)                                                                      \
  do {                                                                                           \
    if (!(cond)) throw ::pm_host::Fail(std::string("Check failed: ") + #cond + " " + (msg));     \
  } while (0)

// ---- validation ----

inline void CheckOptions(const pm_options& o) {
  // PatchMatchOptions::Check, reference mvs/patch_match_options.cc:73-100
  if (o.depth_min != -1.0f || o.depth_max != -1.0f) {
    PM_CHECK(o.depth_min <= o.depth_max, "depth_min <= depth_max");
    PM_CHECK(o.depth_min >= 0.0, "depth_min >= 0");
  }
  PM_CHECK(o.window_radius <= 32, "window_radius <= kMaxPatchMatchWindowRadius");
  PM_CHECK(o.sigma_color > 0.0, "");
  PM_CHECK(o.window_radius > 0, "");
  PM_CHECK(o.window_step > 0, "");
  PM_CHECK(o.window_step <= 2, "");
  PM_CHECK(o.num_samples > 0, "");
  PM_CHECK(o.ncc_sigma > 0.0, "");
  PM_CHECK(o.min_triangulation_angle >= 0.0, "");
  PM_CHECK(o.min_triangulation_angle < 180.0, "");
  PM_CHECK(o.incident_angle_sigma > 0.0, "");
  PM_CHECK(o.num_iterations > 0, "");
  PM_CHECK(o.geom_consistency_regularizer >= 0.0, "");
  PM_CHECK(o.geom_consistency_max_cost >= 0.0, "");
  PM_CHECK(o.filter_min_ncc >= -1.0, "");
  PM_CHECK(o.filter_min_ncc <= 1.0, "");
  PM_CHECK(o.filter_min_triangulation_angle >= 0.0, "");
  PM_CHECK(o.filter_min_triangulation_angle <= 180.0, "");
  PM_CHECK(o.filter_min_num_consistent >= 0, "");
  PM_CHECK(o.filter_geom_consistency_max_cost >= 0.0, "");
  // the reference's kernel dispatch only instantiates radius 1..20 (patch_match_cuda.cu:1313-1337)
  PM_CHECK(o.window_radius <= 20, "window size not supported (reference instantiates radius 1..20)");
  PM_CHECK(o.sigma_spatial > 0.0,
           "sigma_spatial must be resolved by the caller (PatchMatchController sets it to "
           "window_radius, patch_match.cc:436-438)");
  PM_CHECK(o.depth_min > 0.0 && o.depth_max > 0.0,
           "depth range must be set (PatchMatchController::ProcessProblem, patch_match.cc:425-434)");
}

inline void CheckProblem(const pm_options& o, const pm_problem& p) {
  // PatchMatch::Check, reference mvs/patch_match.cc:67-126
  PM_CHECK(o.gpu_index >= -1, "gpu_index >= -1");
  PM_CHECK(p.images != nullptr, "problem.images");
  PM_CHECK(p.num_src_images > 0, "src_image_idxs.size() > 0");
  PM_CHECK(p.src_image_idxs != nullptr, "src_image_idxs");
  std::set<int> unique(p.src_image_idxs, p.src_image_idxs + p.num_src_images);
  unique.insert(p.ref_image_idx);
  PM_CHECK((int)unique.size() == p.num_src_images + 1,
           "duplicate source images or reference image used as source");
  for (int idx : unique) {
    PM_CHECK(idx >= 0, "image_idx >= 0");
    PM_CHECK(idx < p.num_images, "image_idx < images.size()");
    const pm_image& im = p.images[idx];
    PM_CHECK(im.width > 0 && im.height > 0, "bitmap size");
    PM_CHECK(im.gray != nullptr, "grey bitmap");
    PM_CHECK(std::abs(im.K[1] - 0.0f) < 1e-6f, "K[1]");
    PM_CHECK(std::abs(im.K[3] - 0.0f) < 1e-6f, "K[3]");
    PM_CHECK(std::abs(im.K[6] - 0.0f) < 1e-6f, "K[6]");
    PM_CHECK(std::abs(im.K[7] - 0.0f) < 1e-6f, "K[7]");
    PM_CHECK(std::abs(im.K[8] - 1.0f) < 1e-6f, "K[8]");
    if (o.geom_consistency) PM_CHECK(im.depth_map != nullptr, "depth map for geom_consistency");
  }
  if (o.geom_consistency) {
    PM_CHECK(p.images[p.ref_image_idx].normal_map != nullptr, "reference normal map");
    PM_CHECK(p.images[p.ref_image_idx].depth_map != nullptr, "reference depth map");
  }
}

// ---- pose tables (reference mvs/image.cc:97-150), float like the reference ----

inline void Mat33Mul(const float A[9], const float B[9], float C[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

inline void ComputeRelativePose(const float R1[9], const float T1[3], const float R2[9], const float T2[3],
                                float R[9], float T[3]) {
  float R1t[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R1t[3 * i + j] = R1[3 * j + i];
  Mat33Mul(R2, R1t, R);
  for (int i = 0; i < 3; ++i)
    T[i] = T2[i] - (R[3 * i] * T1[0] + R[3 * i + 1] * T1[1] + R[3 * i + 2] * T1[2]);
}

inline void ComposeProjectionMatrix(const float K[9], const float R[9], const float T[3], float P[12]) {
  float RT[12];
  for (int i = 0; i < 3; ++i) {
    RT[4 * i] = R[3 * i];
    RT[4 * i + 1] = R[3 * i + 1];
    RT[4 * i + 2] = R[3 * i + 2];
    RT[4 * i + 3] = T[i];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j)
      P[4 * i + j] = K[3 * i] * RT[j] + K[3 * i + 1] * RT[4 + j] + K[3 * i + 2] * RT[8 + j];
}

inline void ComposeInverseProjectionMatrix(const float K[9], const float R[9], const float T[3],
                                           float inv_P[12]) {
  float m[16];
  ComposeProjectionMatrix(K, R, T, m);
  m[12] = m[13] = m[14] = 0.0f;
  m[15] = 1.0f;
  // explicit cofactor table (general 4x4 inverse), term order fixed so that the
  // result is a deterministic function of m
  float inv[16];
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  const float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
  const float inv_det = 1.0f / det;
  for (int i = 0; i < 12; ++i) inv_P[i] = inv[i] * inv_det;
}

inline void ComputeProjectionCenter(const float R[9], const float T[3], float C[3]) {
  for (int i = 0; i < 3; ++i) C[i] = -(R[i] * T[0] + R[3 + i] * T[1] + R[6 + i] * T[2]);
}

inline void RotatePose(const float RR[9], float R[9], float T[3]) {
  float Rn[9], Tn[3];
  Mat33Mul(RR, R, Rn);
  for (int i = 0; i < 3; ++i) Tn[i] = RR[3 * i] * T[0] + RR[3 * i + 1] * T[1] + RR[3 * i + 2] * T[2];
  std::memcpy(R, Rn, sizeof(Rn));
  std::memcpy(T, Tn, sizeof(Tn));
}

// The tables of the four sweep directions: direction i sees the reference image rotated i times by 90 degrees.
struct PoseTables {
  std::vector<float> poses;  // [4][S][43]
  float ref_K[4][4], ref_inv_K[4][4];
};

// W, H: size of the reference image; src_idxs: the S source images, in the order of the problem.
inline PoseTables BuildPoseTables(const pm_problem& prob, int W, int H, const std::vector<int>& src_idxs) {
  // InitTransforms, reference patch_match_cuda.cu:1694-1808
  PoseTables t;
  const int S = (int)src_idxs.size();
  const pm_image& ref = prob.images[prob.ref_image_idx];
  for (int i = 0; i < 4; ++i) {
    t.ref_K[i][0] = ref.K[0];
    t.ref_K[i][1] = ref.K[2];
    t.ref_K[i][2] = ref.K[4];
    t.ref_K[i][3] = ref.K[5];
  }
  std::swap(t.ref_K[1][0], t.ref_K[1][2]);
  std::swap(t.ref_K[1][1], t.ref_K[1][3]);
  t.ref_K[1][3] = W - 1 - t.ref_K[1][3];
  t.ref_K[2][1] = W - 1 - t.ref_K[2][1];
  t.ref_K[2][3] = H - 1 - t.ref_K[2][3];
  std::swap(t.ref_K[3][0], t.ref_K[3][2]);
  std::swap(t.ref_K[3][1], t.ref_K[3][3]);
  t.ref_K[3][1] = H - 1 - t.ref_K[3][1];
  for (int i = 0; i < 4; ++i) {
    t.ref_inv_K[i][0] = 1.0f / t.ref_K[i][0];
    t.ref_inv_K[i][1] = -t.ref_K[i][1] / t.ref_K[i][0];
    t.ref_inv_K[i][2] = 1.0f / t.ref_K[i][2];
    t.ref_inv_K[i][3] = -t.ref_K[i][3] / t.ref_K[i][2];
  }
  float rotated_R[9], rotated_T[3];
  std::memcpy(rotated_R, ref.R, sizeof(rotated_R));
  std::memcpy(rotated_T, ref.T, sizeof(rotated_T));
  const float R_z90[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
  t.poses.assign((size_t)4 * S * kPoseStride, 0.0f);
  for (int i = 0; i < 4; ++i) {
    for (int s = 0; s < S; ++s) {
      const pm_image& im = prob.images[src_idxs[s]];
      float* p = t.poses.data() + ((size_t)i * S + s) * kPoseStride;
      p[0] = im.K[0]; p[1] = im.K[2]; p[2] = im.K[4]; p[3] = im.K[5];
      float rel_R[9], rel_T[3];
      ComputeRelativePose(rotated_R, rotated_T, im.R, im.T, rel_R, rel_T);
      std::memcpy(p + 4, rel_R, sizeof(rel_R));
      std::memcpy(p + 13, rel_T, sizeof(rel_T));
      ComputeProjectionCenter(rel_R, rel_T, p + 16);
      ComposeProjectionMatrix(im.K, rel_R, rel_T, p + 19);
      ComposeInverseProjectionMatrix(im.K, rel_R, rel_T, p + 31);
    }
    RotatePose(R_z90, rotated_R, rotated_T);
  }
  return t;
}

// The parameter block of a problem for sweep direction `rot`: its base with that direction's intrinsics and pose
// records (`dev_poses`: the device copy of PoseTables::poses).
inline PmParams ParamsForSweep(const PmParams& base, const PoseTables& t, const float* dev_poses, int rot) {
  PmParams p = base;
  p.rot = rot;
  for (int k = 0; k < 4; ++k) {
    p.refK[k] = t.ref_K[rot][k];
    p.refInvK[k] = t.ref_inv_K[rot][k];
  }
  p.poses = dev_poses + (size_t)rot * base.S * kPoseStride;
  return p;
}

// ---- shape scalars ----

// Workgroup size of the generic sweep kernel: whole waves, 128 unless requested.
inline int SweepThreads(int threads_per_group) {
  const int threads = threads_per_group > 0 ? ((threads_per_group + 63) / 64) * 64 : 128;
  return std::min(threads, 256);  // pm_sweep_kernel __launch_bounds__
}

// The scalar half of a problem's parameter block (InitWorkspaceMemory, reference :1810-1857); every pointer is null
// and C is 0: pm_pick_columns (pm_kernels.hip) chooses it from these scalars.
inline PmParams ShapeParams(const pm_options& opt, int W, int H, int S, int src_w, int src_h) {
  PmParams b;
  std::memset(&b, 0, sizeof(b));
  b.W = W; b.H = H; b.S = S; b.src_w = src_w; b.src_h = src_h;
  b.fp_xmax = (float)(src_w + colmap_amd::kFpRingX); b.fp_ymax = (float)(src_h + colmap_amd::kFpRingY);
  b.fp_rows1 = colmap_amd::pm_fp_height(src_h) - 1;
  b.radius = opt.window_radius;
  b.step = opt.window_step;
  b.ntap1d = (2 * b.radius) / b.step + 1;
  b.ntaps = b.ntap1d * b.ntap1d;
  b.num_samples = opt.num_samples;
  b.rec_stride = 4 + 3 * S;
  b.sel_out_off = 4 + S;       // sweep 0 writes half A ...
  b.sel_in_off = 4 + 2 * S;    // ... and reads half B (= 0.5)
  // SweepOptions (reference :1420-1438); doubles narrowed to float where the reference does
  const float sigma_spatial = (float)opt.sigma_spatial;
  const float sigma_color = (float)opt.sigma_color;
  b.spatial_norm = 1.0f / (2.0f * sigma_spatial * sigma_spatial);
  b.color_norm = 1.0f / (2.0f * sigma_color * sigma_color);
  const float ncc_sigma = (float)opt.ncc_sigma;
  const float min_tri = (float)(opt.min_triangulation_angle * 0.0174532925199432);
  const float inc_sigma = (float)opt.incident_angle_sigma;
  // LikelihoodComputer ctor (reference :700-707, 796-802)
  b.cos_min_tri = std::cos(min_tri);
  b.inv_inc_sigma_sq = -0.5f / (inc_sigma * inc_sigma);
  b.inv_ncc_sigma_sq = -0.5f / (ncc_sigma * ncc_sigma);
  b.ncc_norm = (float)(2.0f / (std::sqrt(2.0f * M_PI) * ncc_sigma *
                               erff(2.0f / (ncc_sigma * 1.414213562f))));
  b.geom_reg = (float)opt.geom_consistency_regularizer;
  b.geom_max_cost = (float)opt.geom_consistency_max_cost;
  b.filter_min_ncc = (float)opt.filter_min_ncc;
  b.filter_cos_min_tri =
      std::cos((float)(opt.filter_min_triangulation_angle * 0.0174532925199432));
  b.filter_geom_max_cost = (float)opt.filter_geom_consistency_max_cost;
  b.filter_min_num_consistent = opt.filter_min_num_consistent;
  return b;
}

// ---- source-image span ----

// The 11 x 11 sweep kernels read all S packed images of a problem through ONE buffer resource when they can
// (pm_kernels.hip: fp_resource): base = the lowest image address, an image = the slot (address - base) / kFpStrip in
// the offset register. The address unit forms the buffer offset in 32 bits, so every image must END within 4 GB of the
// base; problems whose images lie further apart take the explicit-index build of the same kernels (fp_base = null).

// Bytes one buffer resource may cover. slab_slots: pm_debug_set_image_slab_slots (0: the hardware's 32-bit offsets;
// tests: one slab of that many images).
inline uint64_t FpSpanLimit(size_t slab_slots, size_t image_bytes) {
  return slab_slots ? (uint64_t)slab_slots * image_bytes + 4097 : (1ull << 32);
}

struct FpSpan {
  uint64_t base;               // lowest address
  std::vector<uint32_t> offs;  // [S] (address - base) / kFpStrip
  bool fits;                   // one buffer resource reaches every image
};

// addrs: the S images' addresses; fp_count: entries (dwords) of one image; limit: FpSpanLimit.
inline FpSpan PlanFpSpan(const uint64_t* addrs, int S, size_t fp_count, uint64_t limit) {
  FpSpan span;
  span.base = *std::min_element(addrs, addrs + S);
  span.offs.resize(S);
  span.fits = span.base % 256 == 0;
  for (int s = 0; s < S; ++s) {
    const uint64_t d = addrs[s] - span.base;
    span.fits = span.fits && d % 256 == 0 && d + fp_count * sizeof(uint32_t) + 4096 < limit;
    span.offs[s] = (uint32_t)((d / colmap_amd::kFpStrip) & 0xffffffffull);
  }
  return span;
}

// ---- re-homing order ----

// The slabs to try, best first, when a problem's images must move into one slab: the slab with most of the problem's
// images, then the newest slab if it is not among them. slab[s]: the slab (its base address) that holds image s, null
// for an image outside the pool; newest_free: the newest slab of this slot size, if it has a free slot, else null.
inline std::vector<const char*> RehomeCandidates(const std::vector<const char*>& slab, const char* newest_free) {
  std::map<const char*, int> votes;
  for (const char* s : slab)
    if (s) ++votes[s];
  std::vector<std::pair<int, const char*>> cand;
  for (auto& v : votes) cand.push_back({v.second, v.first});
  std::sort(cand.begin(), cand.end(), [](auto& a, auto& b) { return a.first > b.first; });
  if (newest_free && !votes.count(newest_free)) cand.push_back({0, newest_free});
  std::vector<const char*> order;
  for (auto& c : cand) order.push_back(c.second);
  return order;
}

// ---- run compatibility ----

// What two problems must agree on to share a run's launches (every launch covers all problems of a run).
struct RunKey {
  int device, W, H, S, src_w, src_h;
  int window_radius, window_step, num_samples, num_iterations, geom_consistency, filter, max_sweeps;
  bool prof, trace;  // phase profile / progress trace enabled
};

inline RunKey MakeRunKey(int device, const PmParams& base, const pm_options& o) {
  return {device, base.W, base.H, base.S, base.src_w, base.src_h,
          o.window_radius, o.window_step, o.num_samples, o.num_iterations, o.geom_consistency, o.filter, o.max_sweeps,
          base.prof != nullptr, base.trace != nullptr};
}

// kRunDebug: a problem with its profile or trace enabled runs alone unless the caller batches it explicitly.
enum RunMismatch { kRunMatch = 0, kRunDevice, kRunSizes, kRunOptions, kRunDebug };

// The first way in which two problems differ, in the order of the enumerators; kRunMatch: they can run together.
inline RunMismatch CompareRunKeys(const RunKey& a, const RunKey& b) {
  if (a.device != b.device) return kRunDevice;
  if (!(a.W == b.W && a.H == b.H && a.S == b.S && a.src_w == b.src_w && a.src_h == b.src_h)) return kRunSizes;
  if (!(a.window_radius == b.window_radius && a.window_step == b.window_step && a.num_samples == b.num_samples &&
        a.num_iterations == b.num_iterations && a.geom_consistency == b.geom_consistency && a.filter == b.filter &&
        a.max_sweeps == b.max_sweeps))
    return kRunOptions;
  if (a.prof || b.prof || a.trace || b.trace) return kRunDebug;
  return kRunMatch;
}

// ---- run shape ----

struct HandleColumns {
  int C;           // the problem's columns per group: pm_pick_columns at create time, or again under COLMAP_AMD_PM_COLS
                   // for a problem that requested none
  bool requested;  // the caller set columns_per_group
};

struct RunShape {
  int C, help;  // columns per wave, waves per column group: what every parameter block of the run carries
};

// Columns per wave by occupancy. A wave sweeps C columns top to bottom, so a launch has (problems x columns / C)
// waves for 16 wave slots per CU. C = 2 is the shape a handle is created for (pm_pick_columns; a full GPU takes three,
// PlanWideColumns below), but ONE
// 2560 x 1920 problem -- how the reference's controller drives the seam, one problem per GPU thread
// (mvs/patch_match.cc:190-204) -- then has 960 .. 1 280 waves for 4 096 slots: with fewer than ~3/4 of the slots
// covered by everything alive on the device, one column per wave doubles the waves. The results do not depend
// on C (tests: group shapes); an explicit columns_per_group is respected.
// One launch geometry for the batch: the columns per wave of THIS run are a property of the run (every parameter
// block of the run carries it), never written back to a handle -- a handle re-run in another batch, or traced, sees
// its own shape again.
// cols[n]: the problems of the run; ntaps, W, H: their common window and image size; live_handles: problems alive on
// the device; ncu: its compute units; cols_switch, help_switch: COLMAP_AMD_PM_COLS (experiments: columns per group for
// the handles that requested none) and COLMAP_AMD_PM_HELP.
inline RunShape PlanRunShape(const HandleColumns* cols, int n, int ntaps, int W, int H, int live_handles, int ncu,
                             int cols_switch, int help_switch) {
  int run_C = 64, run_help = 1;  // (64: pm_pick_columns never gives more)
  bool automatic = ntaps == 121;
  for (int b = 0; b < n; ++b) {
    run_C = std::min(run_C, cols[b].C);
    automatic = automatic && !cols[b].requested;
  }
  if (automatic && cols_switch <= 0) {
    const long long slots = 16ll * ncu;
    const int alive = std::max(n, live_handles);
    const long long waves2 = (long long)alive * ((std::min(W, H) + 1) / 2);
    // (images too small to fill the GPU either way keep the common shape: their time is launch latency)
    const int C = (std::min(W, H) >= 512 && waves2 * 4 < slots * 3) ? 1 : 2;
    run_C = std::min(run_C, C);
    // ... and when even one wave per column leaves the GPU half empty (20 wave slots per CU for the photometric
    // kernel; ONE 2560 x 1920 problem = 1 920 .. 2 560 waves for 5 120), a second wave per column shares the NCC
    // rounds (pm_sweep_pair_kernel): bit-identical, test_group_shapes_do_not_change_results.
    if (C == 1 && run_C == 1 && 2 * waves2 * 10 <= 20ll * ncu * 6) run_help = 2;
  }
  // COLMAP_AMD_PM_HELP (tests, A/B runs): 1 = never, 2 = always (one column per wave, any image size)
  if (help_switch == 1) run_help = 1;
  if (help_switch == 2 && ntaps == 121) {
    run_C = 1;
    run_help = 2;
  }
  return {run_C, run_help};
}

// ---- three columns per wave ----

// The second step of the run shape, behind PlanRunShape: an AUTOMATIC two-column shape becomes three columns per wave
// where the launch is issue-bound. A row step's phases outside the tap rounds cost the same instructions for two
// columns as for three (at S = 20: 60 of 64 lanes in the lane-per-(column, view) phases, 24 stage-1 tasks = six whole
// rounds, 15 cost sums), so a full GPU spends fewer instructions per column (measured in
// DESIGN.md 1.5). Raised exactly when
//   * the shape is PlanRunShape's own two columns: 11 x 11 window, no handle requested its columns, neither
//     COLMAP_AMD_PM_COLS nor COLMAP_AMD_PM_HELP set, no helper wave;
//   * the pass is photometric (the geometric block of three columns exceeds the workgroup's LDS budget) and the
//     lane-per-(column, view) phases are still one pass: 3 S <= 64;
//   * fits3: PmRunPlan::wave_kernels_fit at three columns -- a shape the wave kernels do not hold keeps two columns, it
//     never reaches the generic family through this rule;
//   * everything alive on the device, at three columns per wave, is at least kWideOversubscription times the 16 wave
//     slots per CU the three-column kernel has: below that a launch is a few long waves per slot and its time is the
//     longest wave's, which three columns lengthen. (2: measured at 2560 x 1920, S = 20 -- 8 images alive, 1.25 x the
//     slots: three columns lose 1.4 %; 13 images, 2.03 x: they gain 2.2 %; the benchmark's 16, 2.5 x: 3.4 %.)
// wide_switch: COLMAP_AMD_PM_WIDE -- 0 = never (the shape of PlanRunShape), 1 = the rule above, 2 = the rule without
// its last clause (tests: images too small to fill a GPU).
constexpr int kWideColumns = 3;
constexpr int kWideOversubscription = 2;
inline RunShape PlanWideColumns(RunShape shape, const HandleColumns* cols, int n, int ntaps, int S, bool geom, int W,
                                int H, int live_handles, int ncu, int cols_switch, int help_switch, int wide_switch,
                                bool fits3) {
  bool automatic = ntaps == 121 && cols_switch <= 0 && help_switch <= 0 && wide_switch != 0;
  for (int b = 0; b < n; ++b) automatic = automatic && !cols[b].requested;
  if (!automatic || shape.C != 2 || shape.help != 1) return shape;
  if (geom || kWideColumns * S > 64 || !fits3) return shape;
  const long long slots = 16ll * ncu;
  const int alive = std::max(n, live_handles);
  const long long waves3 = (long long)alive * ((std::min(W, H) + kWideColumns - 1) / kWideColumns);
  if (wide_switch != 2 && waves3 < kWideOversubscription * slots) return shape;
  return {kWideColumns, 1};
}

// ---- sweep schedule ----

// RunWithWindowSizeAndStep, reference patch_match_cuda.cu:1393-1546: num_iterations x 4 sweeps, one per direction.
struct Sweep {
  int rot;
  float perturbation, perturbation_pi, prev_sel_prob_weight;
  int sel_out_off, sel_in_off;     // record halves the sweep writes / reads
  bool filter_photo, filter_geom;  // the last sweep of the full schedule filters
};

struct SweepSchedule {
  int total;                  // sweeps of the full schedule
  std::vector<Sweep> sweeps;  // those the run launches: [limit]
  int final_sel_off;          // the half written by the last of them: what pm_launch_extract reads
};

// max_sweeps (debug): > 0 stop after this many sweeps; 0: all; < 0: initial cost only. sel_out_off, sel_in_off: the
// halves of sweep 0 (ShapeParams).
inline SweepSchedule PlanSweeps(int num_iterations, int max_sweeps, bool filter, bool geom, int sel_out_off,
                                int sel_in_off) {
  SweepSchedule sch;
  sch.total = num_iterations * 4;
  const int limit = max_sweeps > 0 ? std::min(max_sweeps, sch.total) : (max_sweeps < 0 ? 0 : sch.total);
  const float total_num_steps = (float)sch.total;
  int sel_out = sel_out_off, sel_in = sel_in_off;
  for (int k = 0; k < limit; ++k) {
    const int iter = k / 4, sweep = k % 4;
    Sweep s;
    s.rot = k % 4;
    // exponentially reduce the perturbation, linearly increase the influence of the
    // previous selection probabilities (reference :1446-1451)
    s.perturbation = 1.0f / std::pow(2.0f, iter + sweep / 4.0f);
    s.perturbation_pi = (float)(s.perturbation * M_PI);
    s.prev_sel_prob_weight = (float)(iter * 4 + sweep) / total_num_steps;
    s.sel_out_off = sel_out;
    s.sel_in_off = sel_in;
    const bool last_sweep = k == sch.total - 1;
    s.filter_photo = last_sweep && filter;
    s.filter_geom = last_sweep && filter && geom;
    sch.sweeps.push_back(s);
    std::swap(sel_out, sel_in);  // Rotate(): prev_sel_prob <- sel_prob (reference :1911-1915)
  }
  sch.final_sel_off = sel_in;
  return sch;
}

// One problem of a run: its base block, its tables and the device copy of their pose records.
struct RunProblem {
  const PmParams* base;
  const PoseTables* tables;
  const float* dev_poses;
};

// The parameter blocks of a run, [initial cost | sweep 0 | ... | sweep limit-1] x n problems: block [k + 1][b] is
// problem b's block for sweep k. xcd_switch: COLMAP_AMD_PM_XCD_MAP, the workgroup -> (problem, column group) mapping of
// a batched sweep launch (pm_sweep_kernel). fp_resource: PmRunPlan::fp_resource -- one kernel serves the whole batch,
// so unless every problem's images allow buffer-resource addressing NO block of the run carries a base.
inline std::vector<PmParams> FillParamBlocks(const SweepSchedule& sch, const RunProblem* probs, int n,
                                             const RunShape& shape, int xcd_switch, bool fp_resource) {
  const int xcd_map = (xcd_switch == 1 && n % 8 == 0) ? 1 : (xcd_switch == 2 ? 2 : 0);
  std::vector<PmParams> blocks((sch.sweeps.size() + 1) * n);
  for (size_t k = 0; k <= sch.sweeps.size(); ++k) {
    for (int b = 0; b < n; ++b) {
      const int rot = k == 0 ? 0 : sch.sweeps[k - 1].rot;
      PmParams p = ParamsForSweep(*probs[b].base, *probs[b].tables, probs[b].dev_poses, rot);
      p.C = shape.C;
      p.help = shape.help;
      if (!fp_resource) p.fp_base = nullptr;
      if (k > 0) {
        const Sweep& s = sch.sweeps[k - 1];
        p.perturbation = s.perturbation;
        p.perturbation_pi = s.perturbation_pi;
        p.prev_sel_prob_weight = s.prev_sel_prob_weight;
        p.sel_out_off = s.sel_out_off;
        p.sel_in_off = s.sel_in_off;
        p.xcd_map = xcd_map;
        p.ablate = 0;  // (profiling builds: pm_api.cpp overrides the finished array)
      }
      blocks[k * n + b] = p;
    }
  }
  return blocks;
}

// ---- sub-batches ----

// pm_run_batch: a batch of 16 or more problems runs as TWO sub-batches of at least eight images, the first a whole
// multiple of eight (a launch maps problem = workgroup id % batch, so eight problems sit on one XCD's L2 each): half
// the batch rounded up to eights, less where that would leave the second fewer than eight. Returns the size of the
// first; n: the batch runs as one. split_switch: COLMAP_AMD_PM_BATCH_SPLIT (0 = never).
inline int FirstSubBatch(int n, int split_switch) {
  const bool split = n >= 16 && split_switch != 0;
  return split ? std::min(((n - 8) / 8) * 8, ((n / 2 + 7) / 8) * 8) : n;
}

}  // namespace pm_host

#endif  // COLMAP_AMD_PM_HOST_PLAN_H_
