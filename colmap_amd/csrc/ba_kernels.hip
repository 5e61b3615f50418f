// ba_kernels.hip -- gfx950 bundle-adjustment solve: Jacobian builder (one reprojection
// residual per lane) + Levenberg-Marquardt with an implicit-Schur preconditioned CG.
//
// What it replaces: ceres::Solve as COLMAP configures it for large problems
// (ITERATIVE_SCHUR + SCHUR_JACOBI, reference estimators/bundle_adjustment_ceres.cc:203-213)
// together with the in-tree cost functions it evaluates
// (cost_functions/reprojection_error.h:61-212, quaternion_utils.h:105-153,
// sensor/models_jacobian.h:139-321). Semantics of the trust-region loop follow Ceres
// (restated in oracle/ba_oracle.c, which this file is tested against); the layout is new:
//
//  * SoA Jacobian in HBM, fp64: per observation 2x6 pose-tangent, 2x4 intrinsics-tangent,
//    2x3 point columns and the residual, each column contiguous over observations so that
//    the observation-parallel kernels (one lane per residual) read/write coalesced.
//  * Two observation orders, fixed once on the host: "c-order" (sorted by camera, then pose)
//    holds the camera-side Jacobian columns, so every pose / intrinsics block is a contiguous
//    range that the camera-side reductions stream; "p-order" (sorted by 3-D point) holds the
//    point columns, so the point-side passes (C_j = E_j^T E_j + D, C^-1 E^T x,
//    back-substitution) are a lane per point walking a contiguous segment. Only the 16-byte
//    per-observation vectors (J_c x, v) cross between the orders through the permutation.
//  * Camera-side reductions (gradient, J^T v, block-Jacobi Gram blocks) run a wave per chunk
//    of a parameter block's observation list with a wave-level tree reduction into a
//    per-chunk partial; a second tiny kernel adds a block's chunks in order. No atomics
//    anywhere: results are bit-reproducible run to run.
//  * The Schur-Jacobi blocks B_ii = sum J_i^T J_i (pose 6x6 / intrinsics up to 4x4 per
//    block, K = 2 x #observations) are dense Gram contractions and run on the f64 matrix
//    cores (v_mfma_f64_16x16x4_f64: A = B = a 4-row slab of J, D accumulates the 16x16
//    Gram tile).
//  * S x = (B + D^2) x - E C^-1 E^T x is never formed: three kernels per product.
#include "../../include/colmap_amd_ba.h"
#include "../../include/colmap_amd_ba_covariance.h"
#include "ba_probe.h"
#include "ba_schur_explicit.h"
#include "switches.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include "ba_layout.h"  // after the HIP header: the camera-model table gets its host/device qualifiers

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <thread>
#include <type_traits>
#include <string>
#include <vector>

using colmap_amd::dev_switch_int;
using ba_layout::KD_MAX;
using ba_layout::NPAR;
using ba_layout::TIER_MAX;
using ba_layout::TIER_NARROW;
using ba_layout::TIER_WIDE;

extern "C" void pm_release_cached_memory(void);  // pm_api.cpp (same library)

namespace {

thread_local std::string g_ba_error;
thread_local double g_spmv_ms = 0.0;
thread_local long long g_spmv_launches = 0;
thread_local long long g_spmv_bytes = 0;
thread_local double g_mfma_ms = 0.0;       // time inside the f64 MFMA Gram kernel (Schur-Jacobi blocks)
thread_local long long g_mfma_launches = 0;
thread_local long long g_pcg_pipelined_solves = 0, g_pcg_stepwise_solves = 0;  // linear solves per PCG loop, last ba_solve

#define BA_HIP(expr)                                                                           \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); \
  } while (0)

constexpr int PD = 6;        // pose tangent width (5 when the gauge holds a translation coordinate)
// The intrinsics tangent width KD (row stride of Jcam / cam_var) and the widest camera-side block BD
// (stride of the per-chunk partials) are chosen per problem: <KD, BD> = <4, 6> when no camera has
// more than 4 variable intrinsics (every model with the principal point fixed except OPENCV), else
// <8, 8>, or <16, 16> (below). The kernels whose register footprint depends on them are templates
// (instantiated through Solver::with_tier); the others read V.kd / V.bd.
constexpr int KD_WIDE = 16;  // FULL_OPENCV / THIN_PRISM_FISHEYE (12), RAD_TAN_THIN_PRISM_FISHEYE (16): third <KD, BD> tier
constexpr int NPAR_WIDE = 16;
static int chunk_size() {     // observations per camera-side reduction chunk (one wave each)
  const int v = dev_switch_int("COLMAP_AMD_BA_CHUNK", 512);
  return v >= 64 ? v : 512;
}
constexpr int NSCALAR = 16;
constexpr int TILE_OBS = 512;  // observations staged in LDS per point-pass workgroup
constexpr int TILE_PTS = 256;

// Sum over ranks of a device vector (in place). world == 1: nothing. Two transports: a caller
// supplied host callback (any communicator: gloo, MPI, ...) or RCCL on the solver's stream.
struct Comm {
  int rank = 0, world = 1;
  bool by_point = false;  // observations sharded by 3-D point instead of by image (ba_comm::sharding)
  ba_allreduce_fn fn = nullptr;
  void* user = nullptr;
  ncclComm_t nccl = nullptr;
  std::vector<double> host;
  long long calls = 0, doubles = 0;

  void allreduce(double* dev, size_t n, hipStream_t st) {
    if (world <= 1 || n == 0) return;
    ++calls;
    doubles += (long long)n;
    if (nccl) {
      const ncclResult_t r = ncclAllReduce(dev, dev, n, ncclDouble, ncclSum, nccl, st);
      if (r != ncclSuccess) throw std::runtime_error(std::string("RCCL all-reduce failed: ") + ncclGetErrorString(r));
      return;
    }
    host.resize(n);
    BA_HIP(hipMemcpyAsync(host.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP(hipStreamSynchronize(st));
    if (fn(user, host.data(), (int64_t)n) != 0) throw std::runtime_error("all-reduce callback failed");
    BA_HIP(hipMemcpyAsync(dev, host.data(), n * sizeof(double), hipMemcpyHostToDevice, st));
    BA_HIP(hipStreamSynchronize(st));
  }
};

enum Scalar { S_COST = 0, S_GMAX, S_RHO, S_RHO_LAST, S_PQ, S_Q, S_MODEL, S_NEWCOST, S_ITER };

// ------------------------------------------------------------------------------------------
// Device-side view of the problem
// ------------------------------------------------------------------------------------------
struct View {
  int n_obs, n_poses, n_cams, n_points, n_c, n_p, n_blk, n_chunks;
  // parameters (current / candidate)
  double *poses, *cams, *points;
  // topology
  const int *o_pose, *o_cam, *o_pt;  // per observation, c-order (sorted by camera, then pose)
  const double* o_xy;                // c-order
  const int* o_sensor;               // c-order: sensor_from_rig of the observation, -1 none; or NULL
  double* sensors;                   // [n][7] (current / candidate)
  const int* sens_off;               // [n] tangent offset of a variable sensor_from_rig (6-wide), -1 constant; or NULL
  double* Jsens;                     // c-order [2 x 6][n_obs] sensor-tangent columns (only with variable sensors)
  int n_sensors;
  int loss_type;                     // BA_LOSS_*
  const int* stop;                   // pipelined PCG: kernels of an iteration enqueued past convergence return at once; else NULL
  double loss_scale;
  const int *c2a, *a2c;              // c-order position <-> p-order position (sorted by point)
  // p-order copies of the per-observation topology (the point-side linearisation pass reads them
  // coalesced); NULL: the c-order pass scatters the point columns through c2a instead
  const int *a_pose, *a_cam, *a_pt, *a_sensor;
  const double* a_xy;
  const unsigned char* solo;         // c-order: bit k set = no other observation of this point shares block kind k
  const int *pose_off, *pose_dim, *pose_fix;  // pose_fix: held translation coordinate or -1, + 4 when
                                              // the rotation is held (ba_problem::pose_fixed_t)
  const int *cam_off, *cam_dim, *cam_var, *cam_model;
  const int *pt_off, *pt_ptr;
  const int* tile_pt;  // point tiles: points [tile_pt[t], tile_pt[t+1]) have <= TILE_OBS observations
  const int4* tile_info;  // {first point, end point, first p-order observation, observations} of tile t: one load
  int n_tiles;         // 0: some track is longer than a tile, use the untiled kernel
  const int *blk_off, *blk_dim, *blk_kind, *blk_moff;
  const int *chunk_blk, *chunk_beg, *chunk_end;  // chunks are c-order ranges
  const int* blk_chunk_ptr;  // chunks of block b: [blk_chunk_ptr[b], blk_chunk_ptr[b+1])
  const int* blk_fin_end;    // the finalize kernels add the rows [blk_chunk_ptr[b], blk_fin_end[b]): all of the block's
                             // chunks, or only the first one for a HEAVY block (more than kHeavyChunks chunks: a camera
                             // shared by many images), whose rows ba_cpart_heavy_reduce_kernel has summed into it
  const int* heavy_blk;      // [n_heavy] the heavy blocks
  int n_heavy;
  // Observation pairs of one point inside one block (shared intrinsics, rig frames), per block kind k with such pairs:
  // a_boff[k][a] = tangent offset of p-order observation a's block of kind k (-1: none / constant), Wp[k][a] =
  // J_k,a^T E_a (wdim[k] x 3), rebuilt with every linearisation by ba_obs_w_kernel. Null for a kind without pairs.
  const int* a_boff[3];
  double* Wp[3];
  int wdim[3];
  double* cpart;             // [n_chunks][bd*bd] per-chunk partial results (no atomics)
  int kd, bd;                // intrinsics tangent width (Jcam / cam_var row stride), widest block
  // linearisation
  double *Jpose, *Jcam, *res;  // c-order
  double *Jpt, *res_p;         // p-order
  // fp32 copies of the same (scaled) columns for the PCG operator only (ba_options / COLMAP_AMD_BA_OPERATOR_F32):
  // the inexact inner solve streams half the bytes, accumulation stays fp64; cost, gradient, Schur-Jacobi
  // blocks, reduced right-hand side, back-substitution and step evaluation read the fp64 columns. NULL: off.
  float *Jpose32, *Jcam32, *Jpt32;
  double *scale_c, *scale_p;
  double* scalars;
};

// The two 16-byte-per-observation vectors that cross between the observation orders inside an implicit
// product, jx = J_c x and v = J_c x - E u, are both stored in C-ORDER as interleaved (row 0, row 1) pairs:
// the camera-side kernels (ba_obs_jx, ba_block_jtv) access them coalesced, and the point pass -- the one
// kernel that works in p-order -- GATHERS jx (one 16-byte load per observation through a2c) and SCATTERS v
// (one 16-byte store). Measured at BA-1 per product: two planes with 8-byte scattered stores on both
// crossings 106 + 81 + 56 us (obs_jx, point pass, jtv); gathers on both crossings 54 + 59 + 107 us (the
// gather inside the wave-per-chunk reduction of jtv is the expensive one); this layout: see DESIGN.md 2.4.
__device__ __forceinline__ double2 pair_load(const double* __restrict__ p, int i) {
  return reinterpret_cast<const double2*>(p)[i];
}
__device__ __forceinline__ void pair_store(double* __restrict__ p, int i, double a, double b) {
  reinterpret_cast<double2*>(p)[i] = make_double2(a, b);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Deterministic workgroup sum (fixed tree: lanes by xor-shuffle, then waves in index order).
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double wave_part[16];
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wave_part[wave] = v;
  __syncthreads();
  double total = 0.0;
  for (int w = 0; w < nwaves; ++w) total += wave_part[w];
  return total;
}

// out[0] = sum(partials[0..n)) in a fixed order (single workgroup)
__global__ void __launch_bounds__(1024) ba_final_sum_kernel(const double* __restrict__ partials, int n,
                                                            double* __restrict__ out) {
  double acc = 0.0;
  int i = threadIdx.x;
  for (; i + 7 * 1024 < n; i += 8 * 1024) {  // eight loads in flight, added in the rolled loop's order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partials[i + u * 1024];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; i < n; i += 1024) acc += partials[i];
  const double total = block_sum(acc);
  if (threadIdx.x == 0) *out = total;
}

__device__ __forceinline__ void atomic_max_pos(double* addr, double v) {
  // non-negative doubles order like their bit patterns
  atomicMax(reinterpret_cast<unsigned long long*>(addr), (unsigned long long)__double_as_longlong(v));
}

// ------------------------------------------------------------------------------------------
// Per-residual math (reference reprojection_error.h:68-134)
// ------------------------------------------------------------------------------------------
// QuaternionRotatePointWithJac, quaternion_utils.h:105-153
__device__ __forceinline__ void quat_rotate(const double* q, const double* p, double out[3], double* J) {
  const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
  const double px = p[0], py = p[1], pz = p[2];
  const double qx_py = qx * py, qx_pz = qx * pz, qy_px = qy * px, qy_pz = qy * pz, qz_px = qz * px,
               qz_py = qz * py;
  const double c0 = qy_pz - qz_py, c1 = qz_px - qx_pz, c2 = qx_py - qy_px;
  const double d0 = qy * c2 - qz * c1, d1 = qz * c0 - qx * c2, d2 = qx * c1 - qy * c0;
  out[0] = px + 2.0 * (qw * c0 + d0);
  out[1] = py + 2.0 * (qw * c1 + d1);
  out[2] = pz + 2.0 * (qw * c2 + d2);
  if (J) {
    const double qx_px = qx * px, qy_py = qy * py, qz_pz = qz * pz, qw_px = qw * px, qw_py = qw * py,
                 qw_pz = qw * pz;
    J[0] = 2.0 * (qy_py + qz_pz);
    J[1] = 2.0 * (-2.0 * qy_px + qx_py + qw_pz);
    J[2] = 2.0 * (-2.0 * qz_px - qw_py + qx_pz);
    J[3] = 2.0 * (-qz_py + qy_pz);
    J[4] = 2.0 * (qy_px - 2.0 * qx_py - qw_pz);
    J[5] = 2.0 * (qx_px + qz_pz);
    J[6] = 2.0 * (qw_px - 2.0 * qz_py + qy_pz);
    J[7] = 2.0 * (qz_px - qx_pz);
    J[8] = 2.0 * (qz_px + qw_py - 2.0 * qx_pz);
    J[9] = 2.0 * (-qw_px + qz_py - 2.0 * qy_pz);
    J[10] = 2.0 * (qx_px + qy_py);
    J[11] = 2.0 * (-qy_px + qx_py);
  }
}

// ImgFromCamWithJac, sensor/models_jacobian.h:139-321 (+ HasProjectableDepth, models.h:281-285)
template <bool JAC, int NP>
__device__ __forceinline__ bool img_from_cam(int model, const double* prm, double u, double v, double w,
                                             double& x, double& y, double* Jpar, double* Juvw) {
  if (model == BA_SIMPLE_DIVISION || model == BA_DIVISION) {
    // Fitzgibbon's one-parameter division model, closed form (internal::DivisionScaleWithJac,
    // models_jacobian.h:88-113; :1291-1411): no cheirality test, the discriminant decides
    const bool two_f = model == BA_DIVISION;
    const double f1 = prm[0], f2 = two_f ? prm[1] : prm[0];
    const int ic = two_f ? 2 : 1;
    const double k = prm[ic + 2];
    const double rho2 = u * u + v * v;
    const double disc_sq = w * w - 4.0 * rho2 * k;
    if (disc_sq < 0.0) return false;
    const double disc = sqrt(disc_sq);
    const double r = 2.0 / (w + disc);
    x = f1 * r * u + prm[ic];
    y = f2 * r * v + prm[ic + 1];
    if (JAC) {
      const double inv_disc = 1.0 / disc, r_sq = r * r;
      const double dr_du = 2.0 * r_sq * k * u * inv_disc, dr_dv = 2.0 * r_sq * k * v * inv_disc;
      const double dr_dw = -0.5 * r_sq * (1.0 + w * inv_disc), dr_dk = r_sq * rho2 * inv_disc;
      Juvw[0] = f1 * (r + u * dr_du); Juvw[1] = f1 * u * dr_dv; Juvw[2] = f1 * u * dr_dw;
      Juvw[3] = f2 * v * dr_du; Juvw[4] = f2 * (r + v * dr_dv); Juvw[5] = f2 * v * dr_dw;
#pragma unroll
      for (int c = 0; c < NP; ++c) Jpar[c] = Jpar[NP + c] = 0.0;
      Jpar[0] = r * u;
      Jpar[NP + (two_f ? 1 : 0)] = r * v;
      Jpar[ic] = 1.0;
      Jpar[NP + ic + 1] = 1.0;
      Jpar[ic + 2] = f1 * u * dr_dk;
      Jpar[NP + ic + 2] = f2 * v * dr_dk;
    }
    return true;
  }
  if (model == BA_EQUIRECTANGULAR) {
    // spherical panorama (models_jacobian.h:1502-1565): every non-zero direction projects, no cheirality
    // test; the two parameters (width, height) are metadata and always constant
    const double width = prm[0], height = prm[1];
    const double horizontal = sqrt(u * u + w * w);
    if (horizontal + fabs(v) < 2.220446049250313e-16) return false;
    const double theta = atan2(u, w), phi = atan2(-v, horizontal);
    const double kInv2Pi = 1.0 / (2.0 * 3.14159265358979323846), kInvPi = 1.0 / 3.14159265358979323846;
    x = (theta * kInv2Pi + 0.5) * width;
    y = (0.5 - phi * kInvPi) * height;
    if (JAC) {
      const double R2 = horizontal * horizontal, N2 = R2 + v * v;
      const double inv_R2 = 1.0 / R2, inv_N2 = 1.0 / N2, inv_N2_h = inv_N2 / horizontal;
      Juvw[0] = width * kInv2Pi * (w * inv_R2); Juvw[1] = 0.0; Juvw[2] = width * kInv2Pi * (-u * inv_R2);
      Juvw[3] = -height * kInvPi * (u * v * inv_N2_h); Juvw[4] = -height * kInvPi * (-horizontal * inv_N2);
      Juvw[5] = -height * kInvPi * (v * w * inv_N2_h);
#pragma unroll
      for (int c = 0; c < NP; ++c) Jpar[c] = Jpar[NP + c] = 0.0;
      Jpar[0] = theta * kInv2Pi + 0.5;
      Jpar[NP + 1] = 0.5 - phi * kInvPi;
    }
    return true;
  }
  if (!(w >= 2.220446049250313e-16)) return false;
  if (model == BA_EUCM) {  // models_jacobian.h:1413-1500
    const double f1 = prm[0], f2 = prm[1], alpha = prm[4], beta = prm[5];
    const double q = u * u + v * v;
    const double rho2 = beta * q + w * w;
    if (rho2 < 0.0) return false;
    const double rho = sqrt(rho2);
    const double den = alpha * rho + (1.0 - alpha) * w;
    if (!(den >= 2.220446049250313e-16)) return false;
    const double xn = u / den, yn = v / den;
    x = f1 * xn + prm[2];
    y = f2 * yn + prm[3];
    if (JAC) {
      const double inv_rho = 1.0 / rho, inv_den = 1.0 / den, inv_den2 = inv_den * inv_den;
      const double dden_du = alpha * beta * u * inv_rho, dden_dv = alpha * beta * v * inv_rho;
      const double dden_dw = alpha * w * inv_rho + (1.0 - alpha);
      const double dden_dalpha = rho - w, dden_dbeta = alpha * q * 0.5 * inv_rho;
      Juvw[0] = f1 * (inv_den - u * dden_du * inv_den2); Juvw[1] = f1 * (-u * dden_dv * inv_den2);
      Juvw[2] = f1 * (-u * dden_dw * inv_den2);
      Juvw[3] = f2 * (-v * dden_du * inv_den2); Juvw[4] = f2 * (inv_den - v * dden_dv * inv_den2);
      Juvw[5] = f2 * (-v * dden_dw * inv_den2);
      Jpar[0] = xn; Jpar[1] = 0.0; Jpar[2] = 1.0; Jpar[3] = 0.0;
      Jpar[4] = f1 * (-u * dden_dalpha * inv_den2); Jpar[5] = f1 * (-u * dden_dbeta * inv_den2);
      Jpar[NP + 0] = 0.0; Jpar[NP + 1] = yn; Jpar[NP + 2] = 0.0; Jpar[NP + 3] = 1.0;
      Jpar[NP + 4] = f2 * (-v * dden_dalpha * inv_den2); Jpar[NP + 5] = f2 * (-v * dden_dbeta * inv_den2);
    }
    return true;
  }
  const double inv_w = 1.0 / w;
  const double uu = u * inv_w, vv = v * inv_w;
  if (model == BA_FOV) {  // models_jacobian.h:627-724 (the three branches of FOVCameraModel::Distortion)
    const double f1 = prm[0], f2 = prm[1], omega = prm[4];
    const double a = uu, b = vv;
    const double radius2 = a * a + b * b, omega2 = omega * omega;
    const double kEpsilon = 1e-4;
    double factor, factor_r, factor_omega;
    if (omega2 < kEpsilon) {
      factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
      factor_r = omega2 / 3.0;
      factor_omega = 2.0 * omega * radius2 / 3.0 - omega / 6.0;
    } else if (radius2 < kEpsilon) {
      const double t = tan(omega / 2.0), t2 = t * t;
      const double Q = t * (4.0 * t2 * radius2 - 3.0);
      factor = -2.0 * Q / (3.0 * omega);
      factor_r = -8.0 * t * t2 / (3.0 * omega);
      const double dt_domega = 0.5 * (1.0 + t2);
      const double Q_omega = dt_domega * (12.0 * t2 * radius2 - 3.0);
      factor_omega = -2.0 / (3.0 * omega2) * (Q_omega * omega - Q);
    } else {
      const double radius = sqrt(radius2), t = tan(omega / 2.0);
      const double arg = 2.0 * radius * t, atan_arg = atan(arg);
      const double inv_denom_arg = 1.0 / (1.0 + arg * arg);
      factor = atan_arg / (radius * omega);
      factor_r = (2.0 * t * radius * inv_denom_arg - atan_arg) / (2.0 * radius2 * radius * omega);
      factor_omega = (radius * omega * (1.0 + t * t) * inv_denom_arg - atan_arg) / (radius * omega2);
    }
    const double du = a * factor, dv = b * factor;
    x = f1 * du + prm[2];
    y = f2 * dv + prm[3];
    if (JAC) {
      const double cross = 2.0 * a * b * factor_r;
      const double A0 = f1 * (factor + 2.0 * a * a * factor_r), A1 = f1 * cross, A2 = f2 * cross,
                   A3 = f2 * (factor + 2.0 * b * b * factor_r);
      Juvw[0] = A0 * inv_w; Juvw[1] = A1 * inv_w; Juvw[2] = -(A0 * a + A1 * b) * inv_w;
      Juvw[3] = A2 * inv_w; Juvw[4] = A3 * inv_w; Juvw[5] = -(A2 * a + A3 * b) * inv_w;
      Jpar[0] = du; Jpar[1] = 0.0; Jpar[2] = 1.0; Jpar[3] = 0.0; Jpar[4] = f1 * a * factor_omega;
      Jpar[NP + 0] = 0.0; Jpar[NP + 1] = dv; Jpar[NP + 2] = 0.0; Jpar[NP + 3] = 1.0;
      Jpar[NP + 4] = f2 * b * factor_omega;
    }
    return true;
  }
  if (model == BA_SIMPLE_PINHOLE) {
    const double f = prm[0];
    x = f * uu + prm[1];
    y = f * vv + prm[2];
    if (JAC) {
      const double fw = f * inv_w;
      Juvw[0] = fw; Juvw[1] = 0.0; Juvw[2] = -fw * uu; Juvw[3] = 0.0; Juvw[4] = fw; Juvw[5] = -fw * vv;
      Jpar[0] = uu; Jpar[1] = 1.0; Jpar[2] = 0.0;
      Jpar[NP + 0] = vv; Jpar[NP + 1] = 0.0; Jpar[NP + 2] = 1.0;
    }
    return true;
  }
  if (model == BA_PINHOLE) {
    const double f1 = prm[0], f2 = prm[1];
    x = f1 * uu + prm[2];
    y = f2 * vv + prm[3];
    if (JAC) {
      Juvw[0] = f1 * inv_w; Juvw[1] = 0.0; Juvw[2] = -f1 * inv_w * uu;
      Juvw[3] = 0.0; Juvw[4] = f2 * inv_w; Juvw[5] = -f2 * inv_w * vv;
      Jpar[0] = uu; Jpar[1] = 0.0; Jpar[2] = 1.0; Jpar[3] = 0.0;
      Jpar[NP + 0] = 0.0; Jpar[NP + 1] = vv; Jpar[NP + 2] = 0.0; Jpar[NP + 3] = 1.0;
    }
    return true;
  }
  if (model == BA_OPENCV_FISHEYE || model == BA_SIMPLE_RADIAL_FISHEYE || model == BA_RADIAL_FISHEYE ||
      model == BA_SIMPLE_FISHEYE || model == BA_FISHEYE) {
    // equidistant projection (internal::FisheyeProjectionWithJac, models_jacobian.h:51-80) followed by a
    // radial polynomial in the squared fisheye radius (:726-942); SIMPLE_FISHEYE / FISHEYE (:1190-1288)
    // are the same projection without distortion coefficients (nk = 0: identical values, the
    // polynomial terms vanish exactly)
    const bool two_f = model == BA_OPENCV_FISHEYE || model == BA_FISHEYE;
    const double f1 = prm[0], f2 = two_f ? prm[1] : prm[0];
    const int ic = two_f ? 2 : 1;                                  // index of cx
    const int nk = model == BA_OPENCV_FISHEYE ? 4 : (model == BA_RADIAL_FISHEYE ? 2 : (model == BA_SIMPLE_RADIAL_FISHEYE ? 1 : 0));
    const double* k = prm + ic + 2;
    const double a = uu, b = vv;                                   // normalised coordinates
    const double r2 = a * a + b * b;
    const double r = sqrt(r2);
    double fu, fv, Jf0 = 1.0, Jf1 = 0.0, Jf2 = 0.0, Jf3 = 1.0;
    if (r < 2.220446049250313e-16) {
      fu = a;
      fv = b;
    } else {
      const double theta = atan(r);
      const double sc = theta / r;
      fu = sc * a;
      fv = sc * b;
      if (JAC) {
        const double g = (r / (1.0 + r2) - theta) / (r2 * r);
        Jf0 = sc + a * a * g; Jf1 = a * b * g; Jf2 = a * b * g; Jf3 = sc + b * b * g;
      }
    }
    const double fu2 = fu * fu, fv2 = fv * fv, t2 = fu2 + fv2;
    double tp[4];
    tp[0] = t2; tp[1] = t2 * t2; tp[2] = tp[1] * t2; tp[3] = tp[1] * tp[1];
    double radial = 0.0;
    for (int i = 0; i < nk; ++i) radial += k[i] * tp[i];
    const double fu_d = fu + fu * radial, fv_d = fv + fv * radial;
    x = f1 * fu_d + prm[ic];
    y = f2 * fv_d + prm[ic + 1];
    if (JAC) {
      double d_radial = 0.0;
      for (int i = 0; i < nk; ++i) d_radial += (double)(i + 1) * k[i] * (i == 0 ? 1.0 : tp[i - 1]);
      const double cross = 2.0 * fu * fv * d_radial;
      const double i0 = 1.0 + radial + 2.0 * fu2 * d_radial, i3 = 1.0 + radial + 2.0 * fv2 * d_radial;
      const double m0 = i0 * Jf0 + cross * Jf2, m1 = i0 * Jf1 + cross * Jf3;
      const double m2 = cross * Jf0 + i3 * Jf2, m3 = cross * Jf1 + i3 * Jf3;
      const double A0 = f1 * m0, A1 = f1 * m1, A2 = f2 * m2, A3 = f2 * m3;
      Juvw[0] = A0 * inv_w; Juvw[1] = A1 * inv_w; Juvw[2] = -(A0 * a + A1 * b) * inv_w;
      Juvw[3] = A2 * inv_w; Juvw[4] = A3 * inv_w; Juvw[5] = -(A2 * a + A3 * b) * inv_w;
#pragma unroll
      for (int c = 0; c < NP; ++c) Jpar[c] = Jpar[NP + c] = 0.0;
      Jpar[0] = fu_d;
      Jpar[NP + (two_f ? 1 : 0)] = fv_d;
      Jpar[ic] = 1.0;
      Jpar[NP + ic + 1] = 1.0;
      for (int i = 0; i < nk; ++i) {
        Jpar[ic + 2 + i] = f1 * fu * tp[i];
        Jpar[NP + ic + 2 + i] = f2 * fv * tp[i];
      }
    }
    return true;
  }
  if (NP >= 12 && model == BA_FULL_OPENCV) {  // models_jacobian.h:498-625: rational radial term num / den + tangential
    const double f1 = prm[0], f2 = prm[1], k1 = prm[4], k2 = prm[5], p1 = prm[6], p2 = prm[7];
    const double k3 = prm[8], k4 = prm[9], k5 = prm[10], k6 = prm[11];
    const double uu2 = uu * uu, vv2 = vv * vv, uv = uu * vv, r2 = uu2 + vv2, r4 = r2 * r2, r6 = r4 * r2;
    const double num = 1.0 + k1 * r2 + k2 * r4 + k3 * r6;
    const double den = 1.0 + k4 * r2 + k5 * r4 + k6 * r6;
    const double inv_den = 1.0 / den;
    const double radial = num * inv_den;
    const double xd = uu * radial + 2.0 * p1 * uv + p2 * (r2 + 2.0 * uu2);
    const double yd = vv * radial + 2.0 * p2 * uv + p1 * (r2 + 2.0 * vv2);
    x = f1 * xd + prm[2];
    y = f2 * yd + prm[3];
    if (JAC) {
      const double num_prime = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r4;
      const double den_prime = k4 + 2.0 * k5 * r2 + 3.0 * k6 * r4;
      const double d_radial = (num_prime * den - num * den_prime) * inv_den * inv_den;
      const double cross = 2.0 * uv * d_radial;
      const double a00 = f1 * (radial + 2.0 * uu2 * d_radial + 2.0 * p1 * vv + 6.0 * p2 * uu);
      const double a01 = f1 * (cross + 2.0 * p1 * uu + 2.0 * p2 * vv);
      const double a10 = f2 * (cross + 2.0 * p2 * vv + 2.0 * p1 * uu);
      const double a11 = f2 * (radial + 2.0 * vv2 * d_radial + 2.0 * p2 * uu + 6.0 * p1 * vv);
      Juvw[0] = a00 * inv_w; Juvw[1] = a01 * inv_w; Juvw[2] = -(a00 * uu + a01 * vv) * inv_w;
      Juvw[3] = a10 * inv_w; Juvw[4] = a11 * inv_w; Juvw[5] = -(a10 * uu + a11 * vv) * inv_w;
      const double n1 = r2 * inv_den, n2 = r4 * inv_den, n3 = r6 * inv_den;
      const double nn = -num * inv_den * inv_den;
      const double d4 = nn * r2, d5 = nn * r4, d6 = nn * r6;
      Jpar[0] = xd; Jpar[1] = 0.0; Jpar[2] = 1.0; Jpar[3] = 0.0;
      Jpar[4] = f1 * uu * n1; Jpar[5] = f1 * uu * n2; Jpar[6] = f1 * 2.0 * uv; Jpar[7] = f1 * (r2 + 2.0 * uu2);
      Jpar[8] = f1 * uu * n3; Jpar[9] = f1 * uu * d4; Jpar[10] = f1 * uu * d5; Jpar[11] = f1 * uu * d6;
      Jpar[NP + 0] = 0.0; Jpar[NP + 1] = yd; Jpar[NP + 2] = 0.0; Jpar[NP + 3] = 1.0;
      Jpar[NP + 4] = f2 * vv * n1; Jpar[NP + 5] = f2 * vv * n2; Jpar[NP + 6] = f2 * (r2 + 2.0 * vv2);
      Jpar[NP + 7] = f2 * 2.0 * uv;
      Jpar[NP + 8] = f2 * vv * n3; Jpar[NP + 9] = f2 * vv * d4; Jpar[NP + 10] = f2 * vv * d5; Jpar[NP + 11] = f2 * vv * d6;
    }
    return true;
  }
  if (NP >= 16 && model == BA_RAD_TAN_THIN_PRISM_FISHEYE) {
    // models_jacobian.h:1049-1188: equidistant projection, radial polynomial th_radial(theta^2) with six
    // coefficients, then tangential (p0, p1) + thin-prism (s0..s3) distortion of the radially distorted point
    const double f1 = prm[0], f2 = prm[1];
    const double* k = prm + 4;
    const double p0 = prm[10], p1 = prm[11], s0 = prm[12], s1 = prm[13], s2 = prm[14], s3 = prm[15];
    const double a = uu, b = vv;
    const double rr2 = a * a + b * b;
    const double rr = sqrt(rr2);
    double fu, fv, Jf0 = 1.0, Jf1 = 0.0, Jf2 = 0.0, Jf3 = 1.0;
    if (rr < 2.220446049250313e-16) {
      fu = a;
      fv = b;
    } else {
      const double theta = atan(rr);
      const double sc = theta / rr;
      fu = sc * a;
      fv = sc * b;
      if (JAC) {
        const double g = (rr / (1.0 + rr2) - theta) / (rr2 * rr);
        Jf0 = sc + a * a * g; Jf1 = a * b * g; Jf2 = a * b * g; Jf3 = sc + b * b * g;
      }
    }
    const double theta2 = fu * fu + fv * fv;
    double th_radial = 1.0, d_th_radial = 0.0, theta_pow[6], power = 1.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double prev = power;
      power *= theta2;
      theta_pow[i] = power;
      th_radial += k[i] * power;
      d_th_radial += (double)(i + 1) * k[i] * prev;
    }
    const double xr = th_radial * fu, yr = th_radial * fv;
    const double xr2 = xr * xr, yr2 = yr * yr, xyr = xr * yr, r2 = xr2 + yr2, r4 = r2 * r2;
    const double X = xr + 2.0 * p1 * xyr + p0 * (r2 + 2.0 * xr2) + s0 * r2 + s1 * r4;
    const double Y = yr + 2.0 * p0 * xyr + p1 * (r2 + 2.0 * yr2) + s2 * r2 + s3 * r4;
    x = f1 * X + prm[2];
    y = f2 * Y + prm[3];
    if (JAC) {
      const double B00 = 1.0 + 2.0 * p1 * yr + 6.0 * p0 * xr + 2.0 * s0 * xr + 4.0 * s1 * xr * r2;
      const double B01 = 2.0 * p1 * xr + 2.0 * p0 * yr + 2.0 * s0 * yr + 4.0 * s1 * yr * r2;
      const double B10 = 2.0 * p0 * yr + 2.0 * p1 * xr + 2.0 * s2 * xr + 4.0 * s3 * xr * r2;
      const double B11 = 1.0 + 2.0 * p0 * xr + 6.0 * p1 * yr + 2.0 * s2 * yr + 4.0 * s3 * yr * r2;
      const double cross = 2.0 * fu * fv * d_th_radial;
      const double A0 = th_radial + 2.0 * fu * fu * d_th_radial, A3 = th_radial + 2.0 * fv * fv * d_th_radial;
      const double n0 = B00 * A0 + B01 * cross, n1 = B00 * cross + B01 * A3;
      const double n2 = B10 * A0 + B11 * cross, n3 = B10 * cross + B11 * A3;
      const double m0 = n0 * Jf0 + n1 * Jf2, m1 = n0 * Jf1 + n1 * Jf3;
      const double m2 = n2 * Jf0 + n3 * Jf2, m3 = n2 * Jf1 + n3 * Jf3;
      const double J0 = f1 * m0, J1 = f1 * m1, J2 = f2 * m2, J3 = f2 * m3;
      Juvw[0] = J0 * inv_w; Juvw[1] = J1 * inv_w; Juvw[2] = -(J0 * a + J1 * b) * inv_w;
      Juvw[3] = J2 * inv_w; Juvw[4] = J3 * inv_w; Juvw[5] = -(J2 * a + J3 * b) * inv_w;
#pragma unroll
      for (int c = 0; c < NP; ++c) Jpar[c] = Jpar[NP + c] = 0.0;
      Jpar[0] = X; Jpar[2] = 1.0;
      Jpar[NP + 1] = Y; Jpar[NP + 3] = 1.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double dxr = fu * theta_pow[i], dyr = fv * theta_pow[i];
        Jpar[4 + i] = f1 * (B00 * dxr + B01 * dyr);
        Jpar[NP + 4 + i] = f2 * (B10 * dxr + B11 * dyr);
      }
      Jpar[10] = f1 * (r2 + 2.0 * xr2); Jpar[11] = f1 * 2.0 * xyr;
      Jpar[NP + 10] = f2 * 2.0 * xyr; Jpar[NP + 11] = f2 * (r2 + 2.0 * yr2);
      Jpar[12] = f1 * r2; Jpar[13] = f1 * r4;
      Jpar[NP + 14] = f2 * r2; Jpar[NP + 15] = f2 * r4;
    }
    return true;
  }
  if (NP >= 12 && model == BA_THIN_PRISM_FISHEYE) {
    // models_jacobian.h:944-1047: equidistant projection, then radial (k1..k4) + tangential (p1, p2) +
    // thin-prism (sx1, sy1) distortion in fisheye coordinates
    const double f1 = prm[0], f2 = prm[1], k1 = prm[4], k2 = prm[5], p1 = prm[6], p2 = prm[7];
    const double k3 = prm[8], k4 = prm[9], sx1 = prm[10], sy1 = prm[11];
    const double a = uu, b = vv;
    const double rr2 = a * a + b * b;
    const double rr = sqrt(rr2);
    double fu, fv, Jf0 = 1.0, Jf1 = 0.0, Jf2 = 0.0, Jf3 = 1.0;
    if (rr < 2.220446049250313e-16) {
      fu = a;
      fv = b;
    } else {
      const double theta = atan(rr);
      const double sc = theta / rr;
      fu = sc * a;
      fv = sc * b;
      if (JAC) {
        const double g = (rr / (1.0 + rr2) - theta) / (rr2 * rr);
        Jf0 = sc + a * a * g; Jf1 = a * b * g; Jf2 = a * b * g; Jf3 = sc + b * b * g;
      }
    }
    const double fu2 = fu * fu, fv2 = fv * fv, fuv = fu * fv, r2 = fu2 + fv2, r4 = r2 * r2, r6 = r4 * r2, r8 = r4 * r4;
    const double radial = k1 * r2 + k2 * r4 + k3 * r6 + k4 * r8;
    const double du = fu * radial + 2.0 * p1 * fuv + p2 * (r2 + 2.0 * fu2) + sx1 * r2;
    const double dv = fv * radial + 2.0 * p2 * fuv + p1 * (r2 + 2.0 * fv2) + sy1 * r2;
    const double fu_d = fu + du, fv_d = fv + dv;
    x = f1 * fu_d + prm[2];
    y = f2 * fv_d + prm[3];
    if (JAC) {
      const double d_radial = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r4 + 4.0 * k4 * r6;
      const double cross = 2.0 * fuv * d_radial;
      const double i0 = 1.0 + radial + 2.0 * fu2 * d_radial + 2.0 * p1 * fv + 6.0 * p2 * fu + 2.0 * sx1 * fu;
      const double i1 = cross + 2.0 * p1 * fu + 2.0 * p2 * fv + 2.0 * sx1 * fv;
      const double i2 = cross + 2.0 * p2 * fv + 2.0 * p1 * fu + 2.0 * sy1 * fu;
      const double i3 = 1.0 + radial + 2.0 * fv2 * d_radial + 2.0 * p2 * fu + 6.0 * p1 * fv + 2.0 * sy1 * fv;
      const double m0 = i0 * Jf0 + i1 * Jf2, m1 = i0 * Jf1 + i1 * Jf3;
      const double m2 = i2 * Jf0 + i3 * Jf2, m3 = i2 * Jf1 + i3 * Jf3;
      const double A0 = f1 * m0, A1 = f1 * m1, A2 = f2 * m2, A3 = f2 * m3;
      Juvw[0] = A0 * inv_w; Juvw[1] = A1 * inv_w; Juvw[2] = -(A0 * a + A1 * b) * inv_w;
      Juvw[3] = A2 * inv_w; Juvw[4] = A3 * inv_w; Juvw[5] = -(A2 * a + A3 * b) * inv_w;
      Jpar[0] = fu_d; Jpar[1] = 0.0; Jpar[2] = 1.0; Jpar[3] = 0.0;
      Jpar[4] = f1 * fu * r2; Jpar[5] = f1 * fu * r4; Jpar[6] = f1 * 2.0 * fuv; Jpar[7] = f1 * (r2 + 2.0 * fu2);
      Jpar[8] = f1 * fu * r6; Jpar[9] = f1 * fu * r8; Jpar[10] = f1 * r2; Jpar[11] = 0.0;
      Jpar[NP + 0] = 0.0; Jpar[NP + 1] = fv_d; Jpar[NP + 2] = 0.0; Jpar[NP + 3] = 1.0;
      Jpar[NP + 4] = f2 * fv * r2; Jpar[NP + 5] = f2 * fv * r4; Jpar[NP + 6] = f2 * (r2 + 2.0 * fv2);
      Jpar[NP + 7] = f2 * 2.0 * fuv;
      Jpar[NP + 8] = f2 * fv * r6; Jpar[NP + 9] = f2 * fv * r8; Jpar[NP + 10] = 0.0; Jpar[NP + 11] = f2 * r2;
    }
    return true;
  }
  if (model == BA_OPENCV) {  // models_jacobian.h:401-496
    const double f1 = prm[0], f2 = prm[1], k1 = prm[4], k2 = prm[5], p1 = prm[6], p2 = prm[7];
    const double uu2 = uu * uu, vv2 = vv * vv, uv = uu * vv, r2 = uu2 + vv2, r4 = r2 * r2;
    const double radial = k1 * r2 + k2 * r4;
    const double du = uu * radial + 2.0 * p1 * uv + p2 * (r2 + 2.0 * uu2);
    const double dv = vv * radial + 2.0 * p2 * uv + p1 * (r2 + 2.0 * vv2);
    const double xd = uu + du, yd = vv + dv;
    x = f1 * xd + prm[2];
    y = f2 * yd + prm[3];
    if (JAC) {
      const double d_radial_d_r2 = k1 + 2.0 * k2 * r2;
      const double cross = 2.0 * uv * d_radial_d_r2;
      const double du_duu = radial + 2.0 * uu2 * d_radial_d_r2 + 2.0 * p1 * vv + 6.0 * p2 * uu;
      const double du_dvv = cross + 2.0 * p1 * uu + 2.0 * p2 * vv;
      const double dv_duu = cross + 2.0 * p2 * vv + 2.0 * p1 * uu;
      const double dv_dvv = radial + 2.0 * vv2 * d_radial_d_r2 + 2.0 * p2 * uu + 6.0 * p1 * vv;
      const double a00 = f1 * (1.0 + du_duu);
      const double a01 = f1 * du_dvv;
      const double a10 = f2 * dv_duu;
      const double a11 = f2 * (1.0 + dv_dvv);
      Juvw[0] = a00 * inv_w; Juvw[1] = a01 * inv_w; Juvw[2] = -(a00 * uu + a01 * vv) * inv_w;
      Juvw[3] = a10 * inv_w; Juvw[4] = a11 * inv_w; Juvw[5] = -(a10 * uu + a11 * vv) * inv_w;
      Jpar[0] = xd; Jpar[1] = 0.0; Jpar[2] = 1.0; Jpar[3] = 0.0;
      Jpar[4] = f1 * uu * r2; Jpar[5] = f1 * uu * r4; Jpar[6] = f1 * 2.0 * uv; Jpar[7] = f1 * (r2 + 2.0 * uu2);
      Jpar[NP + 0] = 0.0; Jpar[NP + 1] = yd; Jpar[NP + 2] = 0.0; Jpar[NP + 3] = 1.0;
      Jpar[NP + 4] = f2 * vv * r2; Jpar[NP + 5] = f2 * vv * r4; Jpar[NP + 6] = f2 * (r2 + 2.0 * vv2);
      Jpar[NP + 7] = f2 * 2.0 * uv;
    }
    return true;
  }
  if (model == BA_RADIAL) {  // models_jacobian.h:323-398
    const double f = prm[0], k1 = prm[3], k2 = prm[4];
    const double uu2 = uu * uu, vv2 = vv * vv, r2 = uu2 + vv2, r4 = r2 * r2;
    const double radial = k1 * r2 + k2 * r4;
    const double xd = uu * (1.0 + radial), yd = vv * (1.0 + radial);
    x = f * xd + prm[1];
    y = f * yd + prm[2];
    if (JAC) {
      const double d_radial_d_r2 = k1 + 2.0 * k2 * r2;
      const double cross = 2.0 * uu * vv * d_radial_d_r2;
      const double a00 = f * (1.0 + radial + 2.0 * uu2 * d_radial_d_r2);
      const double a01 = f * cross;
      const double a10 = f * cross;
      const double a11 = f * (1.0 + radial + 2.0 * vv2 * d_radial_d_r2);
      Juvw[0] = a00 * inv_w; Juvw[1] = a01 * inv_w; Juvw[2] = -(a00 * uu + a01 * vv) * inv_w;
      Juvw[3] = a10 * inv_w; Juvw[4] = a11 * inv_w; Juvw[5] = -(a10 * uu + a11 * vv) * inv_w;
      Jpar[0] = xd; Jpar[1] = 1.0; Jpar[2] = 0.0; Jpar[3] = f * uu * r2; Jpar[4] = f * uu * r4;
      Jpar[NP + 0] = yd; Jpar[NP + 1] = 0.0; Jpar[NP + 2] = 1.0; Jpar[NP + 3] = f * vv * r2;
      Jpar[NP + 4] = f * vv * r4;
    }
    return true;
  }
  const double f = prm[0], k = prm[3];
  const double uu2 = uu * uu, vv2 = vv * vv, r2 = uu2 + vv2, k_r2 = k * r2, alpha = 1.0 + k_r2;
  const double xd = alpha * uu, yd = alpha * vv;
  x = f * xd + prm[1];
  y = f * yd + prm[2];
  if (JAC) {
    const double two_k = 2.0 * k, fw = f * inv_w, beta = 1.0 + 3.0 * k_r2, tkuv = two_k * uu * vv;
    Juvw[0] = fw * (alpha + two_k * uu2); Juvw[1] = fw * tkuv; Juvw[2] = -fw * uu * beta;
    Juvw[3] = fw * tkuv; Juvw[4] = fw * (alpha + two_k * vv2); Juvw[5] = -fw * vv * beta;
    Jpar[0] = xd; Jpar[1] = 1.0; Jpar[2] = 0.0; Jpar[3] = f * uu * r2;
    Jpar[NP + 0] = yd; Jpar[NP + 1] = 0.0; Jpar[NP + 2] = 1.0; Jpar[NP + 3] = f * vv * r2;
  }
  return true;
}

// ceres::LossFunction::Evaluate for the losses COLMAP can select (CreateLossFunction,
// bundle_adjustment_ceres.cc:66-80; Ceres loss_function.cc restated, see oracle/ba_oracle.c:bao_loss):
// rho[0] = rho(s), rho[1] = rho'(s), rho[2] = rho''(s), s = |r|^2.
__device__ __forceinline__ void loss_eval(int type, double a, double s, double rho[3]) {
  const double kMin = 2.2250738585072014e-308;
  if (type == BA_LOSS_HUBER) {
    const double b = a * a;
    if (s > b) {
      const double r = sqrt(s);
      rho[0] = 2.0 * a * r - b;
      rho[1] = fmax(kMin, a / r);
      rho[2] = -rho[1] / (2.0 * s);
    } else {
      rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
    }
  } else if (type == BA_LOSS_SOFT_L1) {
    const double b = a * a, c = 1.0 / b;
    const double sum = 1.0 + s * c;
    const double tmp = sqrt(sum);
    rho[0] = 2.0 * b * (tmp - 1.0);
    rho[1] = fmax(kMin, 1.0 / tmp);
    rho[2] = -(c * rho[1]) / (2.0 * sum);
  } else if (type == BA_LOSS_CAUCHY) {
    const double b = a * a, c = 1.0 / b;
    const double sum = 1.0 + s * c;
    const double inv = 1.0 / sum;
    rho[0] = b * log(sum);
    rho[1] = fmax(kMin, inv);
    rho[2] = -c * (inv * inv);
  } else {
    rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
  }
}

__device__ __forceinline__ void quat_to_rot(const double* q, double R[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
               tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

template <typename JT> struct JSel;
template <> struct JSel<double> {
  static __device__ __forceinline__ const double* pose(const View& V) { return V.Jpose; }
  static __device__ __forceinline__ const double* cam(const View& V) { return V.Jcam; }
  static __device__ __forceinline__ const double* pt(const View& V) { return V.Jpt; }
};
template <> struct JSel<float> {
  static __device__ __forceinline__ const float* pose(const View& V) { return V.Jpose32; }
  static __device__ __forceinline__ const float* cam(const View& V) { return V.Jcam32; }
  static __device__ __forceinline__ const float* pt(const View& V) { return V.Jpt32; }
};

// Evaluate one observation; JAC: also the tangent-space, column-scaled Jacobian blocks.
// Jpar is laid out 2 x NPAR whatever the model (columns beyond the model's parameters are not read).
// PSIDE: also write the point-side columns and the p-order residual (scattered through c2a); false when
// ba_linearize_point_kernel produces them in its own p-order pass.
// ONLY >= 0: the PLAIN instantiation for the commonest problem shape -- every camera of model ONLY, no sensor_from_rig
// observations, trivial loss, no fp32 operator copies (the host checks; launch_linearize). The same expressions with the
// model switch, the rig branch and the corrector folded away at compile time: bit-identical columns, two thirds of the
// registers.
template <bool JAC, int KD, bool PSIDE = true, int ONLY = -1>
__global__ void __launch_bounds__(256) ba_linearize_kernel(View V, const double* __restrict__ poses,
                                                          const double* __restrict__ cams,
                                                          const double* __restrict__ points,
                                                          const double* __restrict__ sensors,
                                                          double* __restrict__ partials) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  double cost = 0.0;
  if (o < V.n_obs) {
    const int pi = V.o_pose[o], ci = V.o_cam[o], xi = V.o_pt[o];
    const double* q = poses + 7 * (size_t)pi;
    const double* prm = cams + BA_CAM_STRIDE * (size_t)ci;
    const double* X = points + 3 * (size_t)xi;
    constexpr bool PLAIN = ONLY >= 0;
    const int model = PLAIN ? ONLY : V.cam_model[ci];
    constexpr int NP = KD > KD_MAX ? NPAR_WIDE : NPAR;  // J_params columns (12-parameter models only in the wide tier)
    double JR[12], Juvw[6], Jpar[2 * NP], pc[3];
    quat_rotate(q, X, pc, JAC ? JR : nullptr);
    pc[0] += q[4]; pc[1] += q[5]; pc[2] += q[6];
    // sensor_from_rig (RigReprojErrorCostFunctor / ...ConstantRigCostFunctor, reprojection_error.h:
    // 344-417): p_cam = R_s p_rig + t_s
    const int si = (!PLAIN && V.o_sensor) ? V.o_sensor[o] : -1;
    const int soff = (si >= 0 && V.sens_off) ? V.sens_off[si] : -1;
    double Rs[9], JRs[12], prig[3] = {pc[0], pc[1], pc[2]};
    if (si >= 0) {
      const double* sfr = sensors + 7 * (size_t)si;
      quat_to_rot(sfr, Rs);
      if (JAC && soff >= 0) {
        double tmp[3];
        quat_rotate(sfr, prig, tmp, JRs);  // d(R_s p_rig)/dq_s
      }
      const double p0 = pc[0], p1 = pc[1], p2 = pc[2];
      pc[0] = Rs[0] * p0 + Rs[1] * p1 + Rs[2] * p2 + sfr[4];
      pc[1] = Rs[3] * p0 + Rs[4] * p1 + Rs[5] * p2 + sfr[5];
      pc[2] = Rs[6] * p0 + Rs[7] * p1 + Rs[8] * p2 + sfr[6];
    }
    double rx = 0.0, ry = 0.0;
    const bool ok = img_from_cam<JAC, NP>(model, prm, pc[0], pc[1], pc[2], rx, ry, Jpar, Juvw);
    if (ok) {
      rx -= V.o_xy[2 * (size_t)o];
      ry -= V.o_xy[2 * (size_t)o + 1];
    } else {
      rx = ry = 0.0;  // behind the camera: zero residual and Jacobian (:96-116)
    }
    // robust loss: cost = 1/2 rho(|r|^2)
    const double sq_norm = rx * rx + ry * ry;
    double rho[3];
    if (PLAIN) { rho[0] = sq_norm; rho[1] = 1.0; rho[2] = 0.0; }
    else loss_eval(V.loss_type, V.loss_scale, sq_norm, rho);
    cost = 0.5 * rho[0];
    if (JAC) {
      double Js[2][6];  // sensor_from_rig tangent columns: J_uvw [dR_s p/dq_s PlusJacobian | I]
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) Js[r][c] = 0.0;
      if (ok && soff >= 0) {
        const double* sfr = sensors + 7 * (size_t)si;
        const double x = sfr[0], y = sfr[1], z = sfr[2], w = sfr[3];
        const double PJs[12] = {w, z, -y, -z, w, x, y, -x, w, -x, -y, -z};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          double Jq[4];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            Jq[c] = Juvw[3 * r] * JRs[c] + Juvw[3 * r + 1] * JRs[4 + c] + Juvw[3 * r + 2] * JRs[8 + c];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            Js[r][c] = Jq[0] * PJs[c] + Jq[1] * PJs[3 + c] + Jq[2] * PJs[6 + c] + Jq[3] * PJs[9 + c];
            Js[r][3 + c] = Juvw[3 * r + c];
          }
        }
      }
      if (ok && si >= 0) {  // derivative w.r.t. the point in the rig frame: J_uvw R_s
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const double j0 = Juvw[3 * r], j1 = Juvw[3 * r + 1], j2 = Juvw[3 * r + 2];
          Juvw[3 * r] = j0 * Rs[0] + j1 * Rs[3] + j2 * Rs[6];
          Juvw[3 * r + 1] = j0 * Rs[1] + j1 * Rs[4] + j2 * Rs[7];
          Juvw[3 * r + 2] = j0 * Rs[2] + j1 * Rs[5] + j2 * Rs[8];
        }
      }
      const size_t N = (size_t)V.n_obs;
      const int a = V.c2a[o];  // p-order slot of this observation
      const int pdim = V.pose_dim[pi], poff = V.pose_off[pi];
      const int cdim = V.cam_dim[ci], coff = V.cam_off[ci];
      const int ptoff = V.pt_off[xi];
      // pose block: J_uvw * dRp/dq * PlusJacobian (EigenQuaternionManifold, xyzw) | J_uvw
      double Jp[2][PD], Jk[2][KD], Jx[2][3];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < PD; ++c) Jp[r][c] = 0.0;
#pragma unroll
        for (int c = 0; c < KD; ++c) Jk[r][c] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) Jx[r][c] = 0.0;
      }
      if (ok && pdim > 0) {
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        const double PJ[12] = {w, z, -y, -z, w, x, y, -x, w, -x, -y, -z};
        const int pf = V.pose_fix[pi];
        const bool rotc = pf >= 4;  // constant_rig_from_world_rotation: translation columns only
        const int fix = pf < 0 ? -1 : ((pf & 3) == 3 ? -1 : (pf & 3));
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          // translation columns with the held coordinate removed; selects, not Jp[r][d++] -- a dynamically
          // indexed local array lives in scratch
          const double t0 = fix == 0 ? Juvw[3 * r + 1] : Juvw[3 * r];
          const double t1 = (fix == 0 || fix == 1) ? Juvw[3 * r + 2] : Juvw[3 * r + 1];
          const double t2 = fix < 0 ? Juvw[3 * r + 2] : 0.0;
          if (!rotc) {
            double Jq[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
              Jq[c] = Juvw[3 * r] * JR[c] + Juvw[3 * r + 1] * JR[4 + c] + Juvw[3 * r + 2] * JR[8 + c];
#pragma unroll
            for (int c = 0; c < 3; ++c)
              Jp[r][c] = Jq[0] * PJ[c] + Jq[1] * PJ[3 + c] + Jq[2] * PJ[6 + c] + Jq[3] * PJ[9 + c];
            Jp[r][3] = t0; Jp[r][4] = t1; Jp[r][5] = t2;
          } else {
            Jp[r][0] = t0; Jp[r][1] = t1; Jp[r][2] = t2;
          }
        }
      }
      // intrinsics block: variable subset of the model's parameters
      if (ok) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int c = 0; c < KD; ++c)
            if (c < cdim) {
              // select chain instead of Jpar[dynamic index]: a dynamically indexed local array lives in scratch
              const int idx = V.cam_var[KD * ci + c];
              double sel = 0.0;
#pragma unroll
              for (int j = 0; j < NP; ++j) sel = (idx == j) ? Jpar[NP * r + j] : sel;
              Jk[r][c] = sel;
            }
      }
      // point block: J_uvw * R(q)
      if (PSIDE && ok && ptoff >= 0) {
        double R[9];
        quat_to_rot(q, R);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            Jx[r][c] = Juvw[3 * r] * R[c] + Juvw[3 * r + 1] * R[3 + c] + Juvw[3 * r + 2] * R[6 + c];
      }
      // ceres::internal::Corrector: r' = residual_scaling r, J' = sqrt(rho') (J - alpha/|r|^2 r r^T J)
      if (!PLAIN && V.loss_type != BA_LOSS_TRIVIAL) {
        const double sqrt_rho1 = sqrt(rho[1]);
        double residual_scaling = sqrt_rho1, alpha_sq_norm = 0.0;
        if (!(sq_norm == 0.0 || rho[2] <= 0.0)) {
          const double D = 1.0 + 2.0 * sq_norm * rho[2] / rho[1];
          const double alpha = 1.0 - sqrt(D);
          residual_scaling = sqrt_rho1 / (1.0 - alpha);
          alpha_sq_norm = alpha / sq_norm;
        }
        auto correct = [&](double& j0, double& j1) {
          const double rtj = rx * j0 + ry * j1;
          j0 = sqrt_rho1 * (j0 - alpha_sq_norm * rx * rtj);
          j1 = sqrt_rho1 * (j1 - alpha_sq_norm * ry * rtj);
        };
#pragma unroll
        for (int c = 0; c < PD; ++c) correct(Jp[0][c], Jp[1][c]);
#pragma unroll
        for (int c = 0; c < 6; ++c) correct(Js[0][c], Js[1][c]);
#pragma unroll
        for (int c = 0; c < KD; ++c) correct(Jk[0][c], Jk[1][c]);
        if (PSIDE) {
#pragma unroll
          for (int c = 0; c < 3; ++c) correct(Jx[0][c], Jx[1][c]);
        }
        rx *= residual_scaling;
        ry *= residual_scaling;
      }
      V.res[o] = rx;
      V.res[N + o] = ry;
      if (PSIDE) {
        V.res_p[a] = rx;
        V.res_p[N + a] = ry;
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < PD; ++c) {
          const double s = (c < pdim) ? V.scale_c[poff + c] : 0.0;
          V.Jpose[(size_t)(r * PD + c) * N + o] = Jp[r][c] * s;
          if (!PLAIN && V.Jpose32) V.Jpose32[(size_t)(r * PD + c) * N + o] = (float)(Jp[r][c] * s);
        }
#pragma unroll
        for (int c = 0; c < KD; ++c) {
          const double s = (c < cdim) ? V.scale_c[coff + c] : 0.0;
          V.Jcam[(size_t)(r * KD + c) * N + o] = Jk[r][c] * s;
          if (!PLAIN && V.Jcam32) V.Jcam32[(size_t)(r * KD + c) * N + o] = (float)(Jk[r][c] * s);
        }
        if (!PLAIN && V.sens_off) {
#pragma unroll
          for (int c = 0; c < 6; ++c)
            V.Jsens[(size_t)(r * 6 + c) * N + o] = soff >= 0 ? Js[r][c] * V.scale_c[soff + c] : 0.0;
        }
        if (PSIDE) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double s = (ptoff >= 0) ? V.scale_p[ptoff + c] : 0.0;
            V.Jpt[(size_t)(r * 3 + c) * N + a] = Jx[r][c] * s;
            if (!PLAIN && V.Jpt32) V.Jpt32[(size_t)(r * 3 + c) * N + a] = (float)(Jx[r][c] * s);
          }
        }
      }
    }
  }
  cost = block_sum(cost);
  if (threadIdx.x == 0) partials[blockIdx.x] = cost;
}

// Point side of the linearisation in its own p-order pass: one lane per p-order slot re-evaluates the
// observation (R X + t, the projection and J_uvw: ~200 fp64 flops, free next to the memory traffic) and
// writes the 2 x 3 point columns and the p-order residual COALESCED. The c-order pass used to scatter these
// eight doubles per lane through c2a: eight 64-byte write transactions for 64 bytes of payload
// (WRITE_SIZE 1.14 GB per launch at BA-1 for 0.45 GB of columns). Same expressions in the same order as
// ba_linearize_kernel, so the columns are bit-identical to the scattered ones.
template <int KD, int ONLY = -1>
__global__ void __launch_bounds__(256) ba_linearize_point_kernel(View V, const double* __restrict__ poses,
                                                                const double* __restrict__ cams,
                                                                const double* __restrict__ points,
                                                                const double* __restrict__ sensors) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= V.n_obs) return;
  const int pi = V.a_pose[a], ci = V.a_cam[a], xi = V.a_pt[a];
  const double* q = poses + 7 * (size_t)pi;
  const double* prm = cams + BA_CAM_STRIDE * (size_t)ci;
  const double* X = points + 3 * (size_t)xi;
  constexpr bool PLAIN = ONLY >= 0;
  const int model = PLAIN ? ONLY : V.cam_model[ci];
  constexpr int NP = KD > KD_MAX ? NPAR_WIDE : NPAR;
  double Juvw[6], Jpar[2 * NP], pc[3];
  quat_rotate(q, X, pc, nullptr);
  pc[0] += q[4]; pc[1] += q[5]; pc[2] += q[6];
  const int si = (!PLAIN && V.a_sensor) ? V.a_sensor[a] : -1;
  double Rs[9];
  if (si >= 0) {
    const double* sfr = sensors + 7 * (size_t)si;
    quat_to_rot(sfr, Rs);
    const double p0 = pc[0], p1 = pc[1], p2 = pc[2];
    pc[0] = Rs[0] * p0 + Rs[1] * p1 + Rs[2] * p2 + sfr[4];
    pc[1] = Rs[3] * p0 + Rs[4] * p1 + Rs[5] * p2 + sfr[5];
    pc[2] = Rs[6] * p0 + Rs[7] * p1 + Rs[8] * p2 + sfr[6];
  }
  double rx = 0.0, ry = 0.0;
  const bool ok = img_from_cam<true, NP>(model, prm, pc[0], pc[1], pc[2], rx, ry, Jpar, Juvw);
  if (ok) {
    rx -= V.a_xy[2 * (size_t)a];
    ry -= V.a_xy[2 * (size_t)a + 1];
  } else {
    rx = ry = 0.0;
  }
  const double sq_norm = rx * rx + ry * ry;
  if (ok && si >= 0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const double j0 = Juvw[3 * r], j1 = Juvw[3 * r + 1], j2 = Juvw[3 * r + 2];
      Juvw[3 * r] = j0 * Rs[0] + j1 * Rs[3] + j2 * Rs[6];
      Juvw[3 * r + 1] = j0 * Rs[1] + j1 * Rs[4] + j2 * Rs[7];
      Juvw[3 * r + 2] = j0 * Rs[2] + j1 * Rs[5] + j2 * Rs[8];
    }
  }
  const int ptoff = V.pt_off[xi];
  double Jx[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (ok && ptoff >= 0) {
    double R[9];
    quat_to_rot(q, R);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        Jx[r][c] = Juvw[3 * r] * R[c] + Juvw[3 * r + 1] * R[3 + c] + Juvw[3 * r + 2] * R[6 + c];
  }
  if (!PLAIN && V.loss_type != BA_LOSS_TRIVIAL) {
    double rho[3];
    loss_eval(V.loss_type, V.loss_scale, sq_norm, rho);
    const double sqrt_rho1 = sqrt(rho[1]);
    double residual_scaling = sqrt_rho1, alpha_sq_norm = 0.0;
    if (!(sq_norm == 0.0 || rho[2] <= 0.0)) {
      const double D = 1.0 + 2.0 * sq_norm * rho[2] / rho[1];
      const double alpha = 1.0 - sqrt(D);
      residual_scaling = sqrt_rho1 / (1.0 - alpha);
      alpha_sq_norm = alpha / sq_norm;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double rtj = rx * Jx[0][c] + ry * Jx[1][c];
      const double j0 = Jx[0][c], j1 = Jx[1][c];
      Jx[0][c] = sqrt_rho1 * (j0 - alpha_sq_norm * rx * rtj);
      Jx[1][c] = sqrt_rho1 * (j1 - alpha_sq_norm * ry * rtj);
    }
    rx *= residual_scaling;
    ry *= residual_scaling;
  }
  const size_t N = (size_t)V.n_obs;
  V.res_p[a] = rx;
  V.res_p[N + a] = ry;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double s = (ptoff >= 0) ? V.scale_p[ptoff + c] : 0.0;
      V.Jpt[(size_t)(r * 3 + c) * N + a] = Jx[r][c] * s;
      if (!PLAIN && V.Jpt32) V.Jpt32[(size_t)(r * 3 + c) * N + a] = (float)(Jx[r][c] * s);
    }
}

// ------------------------------------------------------------------------------------------
// Point-side passes: one lane per 3-D point, contiguous observation segment
// ------------------------------------------------------------------------------------------

// g_p = E^T r and diag(E^T E)
__global__ void ba_point_grad_kernel(View V, double* __restrict__ gp, double* __restrict__ diag_p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points) return;
  const int off = V.pt_off[j];
  if (off < 0) return;
  const size_t N = (size_t)V.n_obs;
  double g[3] = {0, 0, 0}, d[3] = {0, 0, 0};
  for (int o = V.pt_ptr[j]; o < V.pt_ptr[j + 1]; ++o)
    for (int r = 0; r < 2; ++r) {
      const double rr = V.res_p[r * N + o];
      for (int c = 0; c < 3; ++c) {
        const double J = V.Jpt[(size_t)(r * 3 + c) * N + o];
        g[c] += J * rr;
        d[c] += J * J;
      }
    }
  for (int c = 0; c < 3; ++c) {
    gp[off + c] = g[c];
    diag_p[off + c] = d[c];
  }
}

// E_j^T E_j of this rank's observations (upper triangle xx xy xz yy yz zz), [6][n_points]
__global__ void ba_point_gram_kernel(View V, double* __restrict__ Craw) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points) return;
  const size_t N = (size_t)V.n_obs;
  double C[6] = {0, 0, 0, 0, 0, 0};
  if (V.pt_off[j] >= 0)
    for (int o = V.pt_ptr[j]; o < V.pt_ptr[j + 1]; ++o)
      for (int r = 0; r < 2; ++r) {
        const double a = V.Jpt[(size_t)(r * 3 + 0) * N + o], b = V.Jpt[(size_t)(r * 3 + 1) * N + o],
                     c = V.Jpt[(size_t)(r * 3 + 2) * N + o];
        C[0] += a * a; C[1] += a * b; C[2] += a * c; C[3] += b * b; C[4] += b * c; C[5] += c * c;
      }
  for (int e = 0; e < 6; ++e) Craw[(size_t)e * V.n_points + j] = C[e];
}

// C_j = (sum over ranks of E_j^T E_j) + Dp^2, inverted (3x3 cofactor inverse)
__global__ void ba_point_blocks_kernel(View V, const double* __restrict__ Craw, const double* __restrict__ Dp,
                                       double* __restrict__ Cinv) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points) return;
  const int off = V.pt_off[j];
  if (off < 0) return;
  double C[6];
  for (int e = 0; e < 6; ++e) C[e] = Craw[(size_t)e * V.n_points + j];
  C[0] += Dp[off] * Dp[off];
  C[3] += Dp[off + 1] * Dp[off + 1];
  C[5] += Dp[off + 2] * Dp[off + 2];
  const double a = C[0], b = C[1], c = C[2], d = C[3], e = C[4], f = C[5];
  const double A = d * f - e * e, B = c * e - b * f, Cc = b * e - c * d;
  const double det = a * A + b * B + c * Cc;
  const double id = 1.0 / det;
  double* out = Cinv + 9 * (size_t)j;
  out[0] = A * id; out[1] = B * id; out[2] = Cc * id;
  out[3] = B * id; out[4] = (a * f - c * c) * id; out[5] = (b * c - a * e) * id;
  out[6] = Cc * id; out[7] = (b * c - a * e) * id; out[8] = (a * d - b * b) * id;
}

// MODE 0 (Schur product): u = C^-1 E^T jx ; v_o = jx_o - E_o u
// MODE 1 (reduced rhs):   u = C^-1 g_p     ; v_o = -E_o u
// MODE 2 (back-subst.):   dp = C^-1 (g_p - E^T jx)
// MODE 3 (tiled kernel only): MODE 2 + the model cost change of the step, one partial sum per tile
// MODE 4 (tiled kernel only): MODE 1 + G_o = E_o C^-1 E_o^T of every observation for the Schur-Jacobi blocks
template <int MODE>
__global__ void ba_point_pass_kernel(View V, const double* __restrict__ Cinv, const double* __restrict__ jx,
                                     const double* __restrict__ gp, double* __restrict__ v,
                                     double* __restrict__ dp) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points) return;
  const int off = V.pt_off[j];
  const size_t N = (size_t)V.n_obs;
  const int beg = V.pt_ptr[j], end = V.pt_ptr[j + 1];
  if (off < 0) {  // constant point: no point block
    if (MODE == 0) for (int o = beg; o < end; ++o) { const int c = V.a2c[o]; const double2 j2 = pair_load(jx, c); pair_store(v, c, j2.x, j2.y); }
    if (MODE == 1) for (int o = beg; o < end; ++o) pair_store(v, V.a2c[o], 0.0, 0.0);
    return;
  }
  double t[3] = {0, 0, 0};
  if (MODE != 1) {
    for (int o = beg; o < end; ++o) {
      const double2 j2 = pair_load(jx, V.a2c[o]);
      for (int r = 0; r < 2; ++r) {
        const double x = r ? j2.y : j2.x;
        for (int c = 0; c < 3; ++c) t[c] += V.Jpt[(size_t)(r * 3 + c) * N + o] * x;
      }
    }
  }
  if (MODE == 1) for (int c = 0; c < 3; ++c) t[c] = gp[off + c];
  if (MODE == 2) for (int c = 0; c < 3; ++c) t[c] = gp[off + c] - t[c];
  const double* Ci = Cinv + 9 * (size_t)j;
  double u[3];
  for (int r = 0; r < 3; ++r) u[r] = Ci[3 * r] * t[0] + Ci[3 * r + 1] * t[1] + Ci[3 * r + 2] * t[2];
  if (MODE == 2) {
    for (int c = 0; c < 3; ++c) dp[off + c] = u[c];
    return;
  }
  for (int o = beg; o < end; ++o) {
    const int c = V.a2c[o];
    double2 j2 = make_double2(0.0, 0.0);
    if (MODE == 0) j2 = pair_load(jx, c);
    double out[2];
    for (int r = 0; r < 2; ++r) {
      const double eu = V.Jpt[(size_t)(r * 3 + 0) * N + o] * u[0] + V.Jpt[(size_t)(r * 3 + 1) * N + o] * u[1] +
                        V.Jpt[(size_t)(r * 3 + 2) * N + o] * u[2];
      out[r] = (r ? j2.y : j2.x) - eu;
    }
    pair_store(v, c, out[0], out[1]);
  }
}

// Sharded variants (observations of a point live on several ranks): E^T jx partial -> all-reduce
// -> C^-1 and the per-observation update.
__global__ void ba_point_t_kernel(View V, const double* __restrict__ jx, double* __restrict__ t) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points) return;
  const int off = V.pt_off[j];
  if (off < 0) return;
  const size_t N = (size_t)V.n_obs;
  double acc[3] = {0, 0, 0};
  for (int o = V.pt_ptr[j]; o < V.pt_ptr[j + 1]; ++o) {
    const double2 j2 = pair_load(jx, V.a2c[o]);
    for (int r = 0; r < 2; ++r) {
      const double x = r ? j2.y : j2.x;
      for (int c = 0; c < 3; ++c) acc[c] += V.Jpt[(size_t)(r * 3 + c) * N + o] * x;
    }
  }
  for (int c = 0; c < 3; ++c) t[off + c] = acc[c];
}
// MODE 0: v_o = jx_o - E_o C^-1 t ; MODE 2: dp = C^-1 (g_p - t)
template <int MODE>
__global__ void ba_point_apply_kernel(View V, const double* __restrict__ Cinv, const double* __restrict__ jx,
                                      const double* __restrict__ gp, const double* __restrict__ t,
                                      double* __restrict__ v, double* __restrict__ dp) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points) return;
  const int off = V.pt_off[j];
  const size_t N = (size_t)V.n_obs;
  const int beg = V.pt_ptr[j], end = V.pt_ptr[j + 1];
  if (off < 0) {
    if (MODE == 0) for (int o = beg; o < end; ++o) { const int c = V.a2c[o]; const double2 j2 = pair_load(jx, c); pair_store(v, c, j2.x, j2.y); }
    return;
  }
  double tt[3];
  for (int c = 0; c < 3; ++c) tt[c] = MODE == 2 ? gp[off + c] - t[off + c] : t[off + c];
  const double* Ci = Cinv + 9 * (size_t)j;
  double u[3];
  for (int r = 0; r < 3; ++r) u[r] = Ci[3 * r] * tt[0] + Ci[3 * r + 1] * tt[1] + Ci[3 * r + 2] * tt[2];
  if (MODE == 2) {
    for (int c = 0; c < 3; ++c) dp[off + c] = u[c];
    return;
  }
  for (int o = beg; o < end; ++o) {
    const int c = V.a2c[o];
    const double2 j2 = pair_load(jx, c);
    double out[2];
    for (int r = 0; r < 2; ++r) {
      const double eu = V.Jpt[(size_t)(r * 3 + 0) * N + o] * u[0] + V.Jpt[(size_t)(r * 3 + 1) * N + o] * u[1] +
                        V.Jpt[(size_t)(r * 3 + 2) * N + o] * u[2];
      out[r] = (r ? j2.y : j2.x) - eu;
    }
    pair_store(v, c, out[0], out[1]);
  }
}

// Same passes over tiles of consecutive points (<= TILE_PTS points, <= TILE_OBS observations per workgroup), a LANE
// PER OBSERVATION: the lane keeps its observation's six point columns, its (gathered) jx pair and its c-order
// position in registers from the first load to the final store; only the six products E_o[r][c] jx_o[r] of every
// observation and the 3-vector u = C^-1 t of every point cross the lanes, through 30 KB of LDS. A point's lane adds
// its observations' products in the order of the untiled kernel (bit-identical sums) -- 60 LDS reads per point where
// the columns used to be walked twice (160 reads and two dependent passes per point on 51 of 256 lanes at track length 10). Everything
// a lane needs later (C^-1, g_p, the tangent offset, the observation range) is requested before the first barrier.
template <int MODE, typename JT = double>
__global__ void __launch_bounds__(TILE_PTS) ba_point_pass_tiled_kernel(View V, const double* __restrict__ Cinv,
                                                                       const double* __restrict__ jx,
                                                                       const double* __restrict__ gp,
                                                                       double* __restrict__ v,
                                                                       double* __restrict__ dp,
                                                                       double* __restrict__ model_part = nullptr,
                                                                       double* __restrict__ Gout = nullptr) {
  constexpr bool kRhs = MODE == 1 || MODE == 4, kG = MODE == 4;
  constexpr bool kDp = MODE == 2 || MODE == 3, kModel = MODE == 3, kStoreV = MODE <= 1 || MODE == 4;
  constexpr int KPT = TILE_OBS / TILE_PTS;  // observations per lane
  __shared__ double st[6][kRhs ? 1 : TILE_OBS];  // the six products E_o[r][c] * jx_o[r] of every observation
  __shared__ double su[3][MODE == 2 ? 1 : TILE_PTS];  // u of the tile's points (0 for a constant point; MODE 3: y_p)
  __shared__ unsigned char sfix[MODE == 2 ? 1 : TILE_PTS];
  __shared__ double sci[kG ? 9 : 1][kG ? TILE_PTS : 1];  // MODE 4: C^-1 of the tile's points for the observations' lanes
  [[maybe_unused]] double res2[KPT][2];
  const int t = blockIdx.x, tid = threadIdx.x;
  // (the stop flag of the pipelined PCG is looked at AFTER the loads below are on their way: a workgroup's life is a
  //  chain of dependent round trips -- flag, tile, positions, gather -- and this takes the first one off it; a
  //  stopped launch only writes scratch nobody reads)
  const int stop = V.stop ? *V.stop : 0;
  const int4 ti = V.tile_info[t];
  const int p0 = ti.x, p1 = ti.y, a0 = ti.z, na = ti.w;
  const size_t N = (size_t)V.n_obs;
  const JT* __restrict__ Jp = JSel<JT>::pt(V);
  double J[KPT][6];
  double2 x2[KPT];
  int cpos[KPT], lpt[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int i = tid + k * TILE_PTS;
    x2[k] = make_double2(0.0, 0.0);
    cpos[k] = 0; lpt[k] = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) J[k][c] = 0.0;
    if (i < na) {
      cpos[k] = V.a2c[a0 + i];
      if (MODE != 2) lpt[k] = V.a_pt[a0 + i] - p0;
#pragma unroll
      for (int c = 0; c < 6; ++c) J[k][c] = (double)Jp[(size_t)c * N + a0 + i];
      if (!kRhs) x2[k] = pair_load(jx, cpos[k]);  // gather: jx lives in c-order
      if (kModel) { res2[k][0] = V.res_p[a0 + i]; res2[k][1] = V.res_p[N + a0 + i]; }
    }
  }
  // the point's lane: what it needs after the barrier is on its way now
  const int j = p0 + tid;
  int off = -1, beg = 0, end = 0;
  double Ci[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  if (j < p1) {
    off = V.pt_off[j];
    beg = V.pt_ptr[j] - a0;
    end = V.pt_ptr[j + 1] - a0;
    if (off >= 0) {
#pragma unroll
      for (int e = 0; e < 9; ++e) Ci[e] = Cinv[9 * (size_t)j + e];
      if (MODE != 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = gp[off + c];
      }
    }
  }
  if (stop) return;
  if (!kRhs) {
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      const int i = tid + k * TILE_PTS;
      if (i < na) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          st[c][i] = J[k][c] * x2[k].x;
          st[3 + c][i] = J[k][3 + c] * x2[k].y;
        }
      }
    }
    __syncthreads();
  }
  if (j < p1) {
    double u[3] = {0.0, 0.0, 0.0};
    if (off >= 0) {
      double tt[3] = {0.0, 0.0, 0.0};
      if (!kRhs) {
        // (the order of the untiled kernel and of the oracle: observation, residual row, component -- an inner
        //  solve of fifty CG iterations on an ill-conditioned system amplifies any other association to 1e-6)
        for (int o = beg; o < end; ++o) {
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) tt[c] += st[r * 3 + c][o];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) tt[c] = kRhs ? g[c] : kDp ? g[c] - tt[c] : tt[c];
#pragma unroll
      for (int r = 0; r < 3; ++r) u[r] = Ci[3 * r] * tt[0] + Ci[3 * r + 1] * tt[1] + Ci[3 * r + 2] * tt[2];
      if (kDp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dp[off + c] = u[c];
      }
    }
    if (MODE != 2) {
#pragma unroll
      for (int c = 0; c < 3; ++c) su[c][tid] = u[c];
      sfix[tid] = off < 0 ? 1 : 0;
      if (kG) {
#pragma unroll
        for (int e = 0; e < 9; ++e) sci[e][tid] = Ci[e];
      }
    }
  }
  if (MODE == 2) return;
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int i = tid + k * TILE_PTS;
    if (i < na) {
      const int lp = lpt[k];
      const double u0 = su[0][lp], u1 = su[1][lp], u2 = su[2][lp];
      if (kModel) {  // model cost change -(J step).(r + J step / 2), J step = -(jx + E y_p) (ba_model_from_jx_kernel)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          double m = r ? x2[k].y : x2[k].x;
          if (!sfix[lp]) m += J[k][r * 3] * u0 + J[k][r * 3 + 1] * u1 + J[k][r * 3 + 2] * u2;
          m = -m;
          acc -= m * (res2[k][r] + 0.5 * m);
        }
        continue;
      }
      if (kG) {  // G_o = E_o C^-1 E_o^T (ba_obs_schur_g_kernel: the same expressions), one 32-byte record at the c-order position
        double g00 = 0.0, g01 = 0.0, g11 = 0.0;
        if (!sfix[lp]) {
          double ci[9];
#pragma unroll
          for (int e = 0; e < 9; ++e) ci[e] = sci[e][lp];
          const double e00 = J[k][0], e01 = J[k][1], e02 = J[k][2], e10 = J[k][3], e11 = J[k][4], e12 = J[k][5];
          const double t00 = e00 * ci[0] + e01 * ci[3] + e02 * ci[6], t01 = e00 * ci[1] + e01 * ci[4] + e02 * ci[7],
                       t02 = e00 * ci[2] + e01 * ci[5] + e02 * ci[8];
          const double t10 = e10 * ci[0] + e11 * ci[3] + e12 * ci[6], t11 = e10 * ci[1] + e11 * ci[4] + e12 * ci[7],
                       t12 = e10 * ci[2] + e11 * ci[5] + e12 * ci[8];
          g00 = t00 * e00 + t01 * e01 + t02 * e02;
          g01 = t00 * e10 + t01 * e11 + t02 * e12;
          g11 = t10 * e10 + t11 * e11 + t12 * e12;
        }
        double2* rec = reinterpret_cast<double2*>(Gout + 4 * (size_t)cpos[k]);
        rec[0] = make_double2(g00, g01);
        rec[1] = make_double2(g11, 0.0);
      }
      double out[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const double eu = J[k][r * 3 + 0] * u0 + J[k][r * 3 + 1] * u1 + J[k][r * 3 + 2] * u2;
        const double xr = MODE == 0 ? (r ? x2[k].y : x2[k].x) : 0.0;
        out[r] = sfix[lp] ? xr : xr - eu;  // constant point: no point block, v = jx (MODE 0) / 0 (MODE 1)
      }
      if (kStoreV) pair_store(v, cpos[k], out[0], out[1]);  // one 16-byte scattered store
    }
  }
  if (kModel) {
    acc = block_sum(acc);
    if (tid == 0) model_part[t] = acc;
  }
}

// Point-major reductions over the same tiles, columns staged through LDS (coalesced loads over the tile's
// observation range, the per-point segment walk reads LDS).
// MODE 0: g_p = E^T r, the column norms of E and E^T E (upper triangle, [6][n_points]) of the points
//         (replaces ba_point_grad_kernel + ba_point_gram_kernel when tiles exist)
// MODE 1: model cost change -(J step).(r + J step / 2) with J step = -(jx + E y_p), partial sum per tile
template <int MODE>
__global__ void __launch_bounds__(TILE_PTS) ba_point_reduce_tiled_kernel(View V, const double* __restrict__ jx,
                                                                         const double* __restrict__ dpv,
                                                                         double* __restrict__ out0,
                                                                         double* __restrict__ out1,
                                                                         double* __restrict__ Craw) {
  __shared__ double sJ[6][TILE_OBS];
  __shared__ double sr[2][TILE_OBS];
  __shared__ double sx[MODE == 1 ? 2 : 1][MODE == 1 ? TILE_OBS : 1];
  const int t = blockIdx.x;
  const int p0 = V.tile_pt[t], p1 = V.tile_pt[t + 1];
  const int a0 = V.pt_ptr[p0], na = V.pt_ptr[p1] - a0;
  const size_t N = (size_t)V.n_obs;
  for (int i = threadIdx.x; i < na; i += TILE_PTS) {
#pragma unroll
    for (int c = 0; c < 6; ++c) sJ[c][i] = V.Jpt[(size_t)c * N + a0 + i];
    sr[0][i] = V.res_p[a0 + i];
    sr[1][i] = V.res_p[N + a0 + i];
    if (MODE == 1) {
      const double2 j2 = pair_load(jx, V.a2c[a0 + i]);
      sx[0][i] = j2.x;
      sx[1][i] = j2.y;
    }
  }
  __syncthreads();
  const int j = p0 + threadIdx.x;
  double acc = 0.0;
  if (j < p1) {
    const int off = V.pt_off[j];
    const int beg = V.pt_ptr[j] - a0, end = V.pt_ptr[j + 1] - a0;
    if (MODE == 0) {
      double C[6] = {0, 0, 0, 0, 0, 0};
      if (off >= 0) {
        double g[3] = {0, 0, 0};
        for (int o = beg; o < end; ++o)
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const double rr = sr[r][o];
            const double a = sJ[r * 3][o], b = sJ[r * 3 + 1][o], c = sJ[r * 3 + 2][o];
            g[0] += a * rr; g[1] += b * rr; g[2] += c * rr;
            C[0] += a * a; C[1] += a * b; C[2] += a * c; C[3] += b * b; C[4] += b * c; C[5] += c * c;
          }
        for (int c = 0; c < 3; ++c) out0[off + c] = g[c];
        out1[off] = C[0]; out1[off + 1] = C[3]; out1[off + 2] = C[5];  // column norms = diagonal of E^T E
      }
      for (int e = 0; e < 6; ++e) Craw[(size_t)e * V.n_points + j] = C[e];
    } else {
      double y[3] = {0.0, 0.0, 0.0};
      if (off >= 0) { y[0] = dpv[off]; y[1] = dpv[off + 1]; y[2] = dpv[off + 2]; }
      for (int o = beg; o < end; ++o)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          double m = sx[r][o];
          if (off >= 0) m += sJ[r * 3][o] * y[0] + sJ[r * 3 + 1][o] * y[1] + sJ[r * 3 + 2][o] * y[2];
          m = -m;
          acc -= m * (sr[r][o] + 0.5 * m);
        }
    }
  }
  if (MODE == 1) {
    acc = block_sum(acc);
    if (threadIdx.x == 0) out0[blockIdx.x] = acc;
  }
}

// ------------------------------------------------------------------------------------------
// Observation-parallel passes
// ------------------------------------------------------------------------------------------

// jx_o = Jc_o x  (both residual rows), x a camera-side vector
template <int KD, typename JT = double>
__global__ void ba_obs_jx_kernel(View V, const double* __restrict__ x, double* __restrict__ jx) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_obs) return;
  if (V.stop && *V.stop) return;
  const size_t N = (size_t)V.n_obs;
  const JT* __restrict__ Jpo = JSel<JT>::pose(V);
  const JT* __restrict__ Jca = JSel<JT>::cam(V);
  const int pi = V.o_pose[o], ci = V.o_cam[o];
  const int pdim = V.pose_dim[pi], poff = V.pose_off[pi], cdim = V.cam_dim[ci], coff = V.cam_off[ci];
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int c = 0; c < PD; ++c)
    if (c < pdim) {
      const double xv = x[poff + c];
      a0 += (double)Jpo[(size_t)c * N + o] * xv;
      a1 += (double)Jpo[(size_t)(PD + c) * N + o] * xv;
    }
#pragma unroll
  for (int c = 0; c < KD; ++c)
    if (c < cdim) {
      const double xv = x[coff + c];
      a0 += (double)Jca[(size_t)c * N + o] * xv;
      a1 += (double)Jca[(size_t)(KD + c) * N + o] * xv;
    }
  if (V.sens_off) {
    const int si = V.o_sensor[o];
    const int soff = si >= 0 ? V.sens_off[si] : -1;
    if (soff >= 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double xv = x[soff + c];
        a0 += V.Jsens[(size_t)c * N + o] * xv;
        a1 += V.Jsens[(size_t)(6 + c) * N + o] * xv;
      }
    }
  }
  pair_store(jx, o, a0, a1);  // c-order, coalesced
}

// Model cost change -(J step) . (r + J step / 2) from what the back-substitution left behind: jx = J_c y_c (p-order)
// is still in place, so J step = -(jx + J_p y_p) needs only the point columns, the residual and jx (10 doubles per
// observation instead of 28). Lane per point over its contiguous p-order segment; y_p = dpv (not negated).
__global__ void __launch_bounds__(256) ba_model_from_jx_kernel(View V, const double* __restrict__ jx,
                                                              const double* __restrict__ dpv,
                                                              double* __restrict__ partials) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  double acc = 0.0;
  if (j < V.n_points) {
    const size_t N = (size_t)V.n_obs;
    const int off = V.pt_off[j];
    double y[3] = {0.0, 0.0, 0.0};
    if (off >= 0) { y[0] = dpv[off]; y[1] = dpv[off + 1]; y[2] = dpv[off + 2]; }
    for (int o = V.pt_ptr[j]; o < V.pt_ptr[j + 1]; ++o) {
      const double2 j2 = pair_load(jx, V.a2c[o]);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        double m = r ? j2.y : j2.x;
        if (off >= 0)
          m += V.Jpt[(size_t)(r * 3) * N + o] * y[0] + V.Jpt[(size_t)(r * 3 + 1) * N + o] * y[1] +
               V.Jpt[(size_t)(r * 3 + 2) * N + o] * y[2];
        m = -m;
        acc -= m * (V.res_p[r * N + o] + 0.5 * m);
      }
    }
  }
  acc = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------
// Camera-side reductions: one wave per chunk of a parameter block's observation list
// ------------------------------------------------------------------------------------------

// fp32 operator copy of the same column (never for variable sensor_from_rig blocks: the fp32 operator is
// not enabled for problems that have them)
__device__ __forceinline__ const float* blk_col32(const View& V, int kind, int r, int c) {
  const size_t N = (size_t)V.n_obs;
  return kind == 0 ? V.Jpose32 + (size_t)(r * PD + c) * N : V.Jcam32 + (size_t)(r * V.kd + c) * N;
}
__device__ __forceinline__ const double* blk_col(const View& V, int kind, int r, int c) {
  const size_t N = (size_t)V.n_obs;
  if (kind == 2) return V.Jsens + (size_t)(r * 6 + c) * N;  // variable sensor_from_rig block
  return kind == 0 ? V.Jpose + (size_t)(r * PD + c) * N : V.Jcam + (size_t)(r * V.kd + c) * N;
}

// y_b += J_b^T v  (v: 2 rows per observation). With DIAG: also diag_b += colsq(J_b).
// DIAG (gradient pass): v is the c-order residual in two planes. Otherwise v is the c-order pair vector of an
// implicit product (one 16-byte load per observation).
template <bool DIAG, int BD, typename JT = double>
__global__ void __launch_bounds__(64) ba_block_jtv_kernel(View V, const double* __restrict__ v,
                                                         double* __restrict__ y, double* __restrict__ diag) {
  if (V.stop && *V.stop) return;
  const int ch = blockIdx.x;
  const int b = V.chunk_blk[ch];
  const int kind = V.blk_kind[b], dim = V.blk_dim[b], off = V.blk_off[b];
  const size_t N = (size_t)V.n_obs;
  double acc[BD], dacc[BD];
#pragma unroll
  for (int c = 0; c < BD; ++c) acc[c] = dacc[c] = 0.0;
  // two observations per lane and trip (o, o + 64): twice the loads in flight; the accumulation order
  // of a lane stays o, o + 64, o + 128, ... as in the rolled loop
  const int end = V.chunk_end[ch];
  for (int o = V.chunk_beg[ch] + threadIdx.x; o < end; o += 128) {
    const int o2 = o + 64;
    const bool two = o2 < end;
    const int oz = two ? o2 : o;
    double v0, v1, w0, w1;
    if (DIAG) {
      v0 = v[o]; v1 = v[N + o];
      w0 = v[oz]; w1 = v[N + oz];
    } else {
      const double2 p0 = pair_load(v, o), p1 = pair_load(v, oz);
      v0 = p0.x; v1 = p0.y;
      w0 = p1.x; w1 = p1.y;
    }
    double j0[BD], j1[BD], k0[BD], k1[BD];
#pragma unroll
    for (int c = 0; c < BD; ++c)
      if (c < dim) {
        if constexpr (sizeof(JT) == 4) {
          const float* c0 = blk_col32(V, kind, 0, c);
          const float* c1 = blk_col32(V, kind, 1, c);
          j0[c] = (double)c0[o]; j1[c] = (double)c1[o];
          k0[c] = (double)c0[oz]; k1[c] = (double)c1[oz];
        } else {
          const double* c0 = blk_col(V, kind, 0, c);
          const double* c1 = blk_col(V, kind, 1, c);
          j0[c] = c0[o]; j1[c] = c1[o];
          k0[c] = c0[oz]; k1[c] = c1[oz];
        }
      }
#pragma unroll
    for (int c = 0; c < BD; ++c)
      if (c < dim) {
        acc[c] += j0[c] * v0 + j1[c] * v1;
        if (DIAG) dacc[c] += j0[c] * j0[c] + j1[c] * j1[c];
        if (two) {
          acc[c] += k0[c] * w0 + k1[c] * w1;
          if (DIAG) dacc[c] += k0[c] * k0[c] + k1[c] * k1[c];
        }
      }
  }
  (void)off;
#pragma unroll
  for (int c = 0; c < BD; ++c)
    if (c < dim) {
      const double s = wave_sum(acc[c]);
      if (threadIdx.x == 0) V.cpart[(size_t)ch * BD * BD + c] = s;
      if (DIAG) {
        const double d = wave_sum(dacc[c]);
        if (threadIdx.x == 0) V.cpart[(size_t)ch * BD * BD + BD + c] = d;
      }
    }
}

// A block with thousands of chunks -- ONE camera shared by every image of a 1 000-image problem has 4 000 -- makes every
// finalize kernel below a single thread walking thousands of dependent loads (1.3 ms each at BA-1 with shared intrinsics:
// 60 % of that solve, profiles/r05_ba_shared_intrinsics_kernel_stats_before.csv). For such HEAVY blocks this kernel first
// sums the first `width` entries of all the block's rows into its first row: one workgroup per (heavy block, 64 or 16
// entries), the threads of an entry stride over the rows, their partial sums are added in thread order -- a fixed tree,
// the same bits on every run. The finalize kernels then read that one row (View::blk_fin_end).
constexpr int kHeavyChunks = 64;  // (development switch COLMAP_AMD_BA_HEAVY_CHUNKS: the tests lower it to reach the path)
__global__ void __launch_bounds__(1024) ba_cpart_heavy_reduce_kernel(View V, int width) {
  __shared__ double part[1024];
  const int b = V.heavy_blk[blockIdx.x];
  const int epw = width <= 16 ? 16 : 64;            // entries per workgroup
  const int groups = 1024 / epw;
  const int el = threadIdx.x % epw, g = threadIdx.x / epw;
  const int e = el + epw * blockIdx.y;
  const int bb = V.bd * V.bd;
  const int ch0 = V.blk_chunk_ptr[b], ch1 = V.blk_chunk_ptr[b + 1];
  double s = 0.0;
  if (e < width) {
    // eight rows per round trip (a thread's 60-odd rows used to be one dependent load each), added in row order
    constexpr int U = 8;
    for (int ch = ch0 + g; ch < ch1; ch += U * groups) {
      double row[U];
#pragma unroll
      for (int k = 0; k < U; ++k) row[k] = ch + k * groups < ch1 ? V.cpart[(size_t)(ch + k * groups) * bb + e] : 0.0;
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (ch + k * groups < ch1) s += row[k];
    }
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (g == 0 && e < width) {
    double t = 0.0;
    for (int k = 0; k < groups; ++k) t += part[k * epw + el];
    V.cpart[(size_t)ch0 * bb + e] = t;
  }
}

// y_b = sum over the block's chunks, in chunk order (deterministic); lane per block
template <bool DIAG>
__global__ void ba_block_vec_finalize_kernel(View V, double* __restrict__ y, double* __restrict__ diag) {
  // thread per (block, component) -- a lane per block walked its components' loads one after the other
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = t / V.bd, c = t - b * V.bd;
  if (b >= V.n_blk) return;
  const int dim = V.blk_dim[b], off = V.blk_off[b];
  if (c >= dim) return;
  double s = 0.0, d = 0.0;
  for (int ch = V.blk_chunk_ptr[b]; ch < V.blk_fin_end[b]; ++ch) {
    s += V.cpart[(size_t)ch * V.bd * V.bd + c];
    if (DIAG) d += V.cpart[(size_t)ch * V.bd * V.bd + V.bd + c];
  }
  y[off + c] = s;  // every camera-side entry belongs to exactly one block: no memset before, no accumulate
  if (DIAG) diag[off + c] = d;
}

// q_b = Dc_b^2 x_b + sum over the block's chunks (the tail of an implicit product on a single GPU without
// priors: ba_block_vec_finalize_kernel<false> + ba_dsq_x_kernel + ba_add_kernel in one launch, same operations)
__global__ void ba_block_vec_finalize_q_kernel(View V, const double* __restrict__ Dc, const double* __restrict__ x,
                                               double* __restrict__ q) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = t / V.bd, c = t - b * V.bd;
  if (b >= V.n_blk) return;
  const int dim = V.blk_dim[b], off = V.blk_off[b];
  if (c >= dim) return;
  double s = 0.0;
  for (int ch = V.blk_chunk_ptr[b]; ch < V.blk_fin_end[b]; ++ch) s += V.cpart[(size_t)ch * V.bd * V.bd + c];
  q[off + c] = Dc[off + c] * Dc[off + c] * x[off + c] + s;
}

// M_b (+)= sum over the block's chunks of the dim x dim partials; lane per block
template <bool ACCUMULATE>
__global__ void ba_block_mat_finalize_kernel(View V, double* __restrict__ M) {
  // thread per (block, entry): a lane per block walked dim^2 x chunks dependent loads one after the other (37 us for
  // the 2 000 blocks of 1 000 images); the chunk order of the sum is unchanged
  const int bb = V.bd * V.bd;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = t / bb, e = t - b * bb;
  if (b >= V.n_blk) return;
  const int dim = V.blk_dim[b];
  if (e >= dim * dim) return;
  double* Mb = M + V.blk_moff[b];
  double s = 0.0;
  for (int ch = V.blk_chunk_ptr[b]; ch < V.blk_fin_end[b]; ++ch) s += V.cpart[(size_t)ch * bb + e];
  Mb[e] = ACCUMULATE ? Mb[e] + s : s;
}

// Schur-Jacobi diagonal blocks on the f64 matrix cores.
//
// M_b = B_bb - sum_j W_bj C_j^-1 W_bj^T with W_bj = sum_{o in (b,j)} J_b,o^T E_o. For an observation
// that is the only one of its point in block b (every pose block of a COLMAP track, every
// intrinsics block of a per-image camera) the point's term is J_b,o^T G_o J_b,o with the 2 x 2
// G_o = E_o C_j^-1 E_o^T, so the block is ONE Gram-like contraction
//     M_b = sum_o J_b,o^T (I - G_o) J_b,o
// -- A = a 4-row slab of J_b (two observations x two residual rows), B = (I - G) applied to the
// same slab, v_mfma_f64_16x16x4_f64 accumulates the 16 x 16 tile (columns >= dim are zero). G_o is
// computed where C^-1 is local (ba_obs_schur_g_kernel, p-order) and stored in c-order. Observation
// pairs of one point inside one block (shared intrinsics, rig frames) add their cross terms in
// ba_block_schur_cross_kernel; the self term is already in (I - G).
// Lane l of a wave holds column i = l & 15 and slab row k = l >> 4 (k = 2 * observation in slab +
// residual row). C/D layout: col = l & 15, row = (l >> 4) + 4 * reg.
typedef double v4f64 __attribute__((ext_vector_type(4)));

// G_o = E_o C_j^-1 E_o^T (g00, g01, g11), lane per observation in p-order, stored at the c-order
// position as a record {g00, g01, g11, 0}; constant points (no point block) have G = 0.
__global__ void __launch_bounds__(256) ba_obs_schur_g_kernel(View V, const double* __restrict__ Cinv,
                                                             double* __restrict__ G) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= V.n_obs) return;
  const size_t N = (size_t)V.n_obs;
  const int c = V.a2c[a];
  const int j = V.o_pt[c];
  double g00 = 0.0, g01 = 0.0, g11 = 0.0;
  if (V.pt_off[j] >= 0) {
    const double* Ci = Cinv + 9 * (size_t)j;
    const double e00 = V.Jpt[a], e01 = V.Jpt[N + a], e02 = V.Jpt[2 * N + a];
    const double e10 = V.Jpt[3 * N + a], e11 = V.Jpt[4 * N + a], e12 = V.Jpt[5 * N + a];
    // T = E C^-1 (2 x 3)
    const double t00 = e00 * Ci[0] + e01 * Ci[3] + e02 * Ci[6], t01 = e00 * Ci[1] + e01 * Ci[4] + e02 * Ci[7],
                 t02 = e00 * Ci[2] + e01 * Ci[5] + e02 * Ci[8];
    const double t10 = e10 * Ci[0] + e11 * Ci[3] + e12 * Ci[6], t11 = e10 * Ci[1] + e11 * Ci[4] + e12 * Ci[7],
                 t12 = e10 * Ci[2] + e11 * Ci[5] + e12 * Ci[8];
    g00 = t00 * e00 + t01 * e01 + t02 * e02;
    g01 = t00 * e10 + t01 * e11 + t02 * e12;
    g11 = t10 * e10 + t11 * e11 + t12 * e12;
  }
  // one 32-byte record per observation at its c-order position (a whole sector per lane; three planes meant three
  // scattered 8-byte stores, each a partial write of its own sector)
  double2* rec = reinterpret_cast<double2*>(G + 4 * (size_t)c);
  rec[0] = make_double2(g00, g01);
  rec[1] = make_double2(g11, 0.0);
}

// The contraction with its operands staged through LDS: per trip a wave loads 32 consecutive observations of every
// Jacobian column of the block (and of G) as contiguous 256-byte segments -- half a wave per (row, column) pair --
// and the 16 slabs of the trip feed the matrix core from LDS (operands loaded lane by lane would touch 16 different
// columns per load instruction).
constexpr int GRAM_TRIP = 32;
constexpr int GRAM_WAVES = 4;
template <int BD>  // widest block of the problem: bounds the prefetch registers (6, 8 or 16 column pairs per lane)
__global__ void __launch_bounds__(64 * GRAM_WAVES, BD <= 8 ? 4 : 2) ba_block_gram_lds_kernel(View V, const double* __restrict__ G) {
  // One workgroup per chunk, FOUR waves, wave w taking the trips w, w + 4, ... of the chunk with its own LDS tile and
  // accumulator; the four partial tiles are added in wave order at the end (a fixed tree). One wave per chunk left
  // ~2 waves per SIMD on the chip (a chunk is up to 2 048 observations, a camera one or two chunks), each a serial
  // chain of 64 trips of (LDS round trip + 16 dependent-issue matrix-core instructions): latency, not bandwidth.
  __shared__ double sJ[GRAM_WAVES][2][16][GRAM_TRIP + 1];  // [wave][row][column][observation], padded against bank conflicts
  __shared__ double sG[GRAM_WAVES][3][GRAM_TRIP + 1];
  const int ch = blockIdx.x;
  const int b = V.chunk_blk[ch];
  const int kind = V.blk_kind[b], dim = V.blk_dim[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, k = lane >> 4;  // column, row-in-slab
  const int r = k & 1, oo = k >> 1;        // residual row, observation within the slab
  const int half = lane >> 5, lo = lane & 31;
  const int beg = V.chunk_beg[ch], end = V.chunk_end[ch];
  v4f64 acc = {0.0, 0.0, 0.0, 0.0};
  const bool col_ok = i < dim;
  // The operands of the wave's next trip are loaded into registers while the matrix core works on this one (a lane's
  // share: one 32-observation segment of <= 16 (row, column) pairs -- pairs cr = half, half + 2, ... -- and
  // up to two entries of G).
  double pj[BD], pg[2];
  auto prefetch = [&](int s) {
    const int n = min(GRAM_TRIP, end - s);
#pragma unroll
    for (int q = 0; q < BD; ++q) {
      const int cr = half + 2 * q;
      pj[q] = (cr < 2 * dim && lo < n) ? blk_col(V, kind, cr & 1, cr >> 1)[s + lo] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {  // the trip's 32 records of G: 1 KB, contiguous
      const int e = lane + 64 * q;
      pg[q] = (e >> 2) < n ? G[4 * (size_t)s + e] : 0.0;
    }
  };
  auto wave_sync = [] {  // the tile is handed from lane to lane of ONE wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  constexpr int STEP = GRAM_WAVES * GRAM_TRIP;
  const int first = beg + wave * GRAM_TRIP;
  if (first < end) prefetch(first);
  for (int s = first; s < end; s += STEP) {
#pragma unroll
    for (int q = 0; q < BD; ++q) {
      const int cr = half + 2 * q;
      if (cr < 2 * dim) sJ[wave][cr & 1][cr >> 1][lo] = pj[q];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = lane + 64 * q;
      if ((e & 3) < 3) sG[wave][e & 3][e >> 2] = pg[q];
    }
    wave_sync();
    if (s + STEP < end) prefetch(s + STEP);
#pragma unroll 4
    for (int u = 0; u < GRAM_TRIP / 2; ++u) {
      const int o = 2 * u + oo;
      double a = 0.0, bb = 0.0;
      if (col_ok) {
        const double j0 = sJ[wave][0][i][o], j1 = sJ[wave][1][i][o];
        const double g00 = sG[wave][0][o], g01 = sG[wave][1][o], g11 = sG[wave][2][o];
        a = r ? j1 : j0;
        bb = r ? j1 - (g01 * j0 + g11 * j1) : j0 - (g00 * j0 + g01 * j1);
      }
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc, 0, 0, 0);
    }
    wave_sync();
  }
  double* part = &sJ[wave][0][0][0];  // the wave's own tile memory (its last trip is behind a wave_sync): [4][64]
  if (wave > 0) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[reg * 64 + lane] = acc[reg];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = k + 4 * reg;
    double t = acc[reg];
#pragma unroll
    for (int w = 1; w < GRAM_WAVES; ++w) t += (&sJ[w][0][0][0])[reg * 64 + lane];
    if (row < dim && i < dim) V.cpart[(size_t)ch * V.bd * V.bd + row * dim + i] = t;
  }
}

// Cross terms - sum_{o != o2 in (b,j)} (J_b,o^T E_o) C_j^-1 (J_b,o2^T E_o2)^T of observation pairs of one
// point inside one block (only launched when such pairs exist). One lane per observation.
// W_o = J_b,o^T E_o (dim x 3) of every observation that has a partner of its point in one of its blocks, stored in
// p-order: the partners of an observation are then NEIGHBOURS in memory (ba_block_schur_cross_kernel walks them), and
// a W is computed once per linearisation instead of once per partner visit.
template <int BD>
__global__ void ba_obs_w_kernel(View V) {
  // a lane per P-ORDER slot: the point columns and the stores of W (wd x 3 doubles per slot, neighbours in memory) are
  // coalesced, only the block's 2 x wd camera-side entries are gathered through a2c (a lane per c-order slot gathered
  // the six point columns AND scattered the 12 .. 24 stores: 370 us at BA-1 with one shared camera)
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= V.n_obs) return;
  const int o = V.a2c[a];
  const unsigned so = V.solo[o];
  const size_t N = (size_t)V.n_obs;
  double e[2][3];
  bool have_e = false;
#pragma unroll
  for (int kind = 0; kind < 3; ++kind) {
    if (V.Wp[kind] == nullptr || ((so >> kind) & 1) || V.a_boff[kind][a] < 0) continue;
    if (!have_e) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) e[r][c] = V.Jpt[(size_t)(r * 3 + c) * N + a];
      have_e = true;
    }
    const int wd = V.wdim[kind];
    double* w = V.Wp[kind] + (size_t)a * wd * 3;
#pragma unroll
    for (int x = 0; x < BD; ++x) {
      if (x >= wd) continue;
      const double j0 = blk_col(V, kind, 0, x)[o], j1 = blk_col(V, kind, 1, x)[o];
#pragma unroll
      for (int c = 0; c < 3; ++c) w[x * 3 + c] = j0 * e[0][c] + j1 * e[1][c];
    }
  }
}

template <int BD>
__global__ void __launch_bounds__(64) ba_block_schur_cross_kernel(View V, const double* __restrict__ Cinv) {
  const int ch = blockIdx.x;
  const int b = V.chunk_blk[ch];
  const int kind = V.blk_kind[b], dim = V.blk_dim[b], boff = V.blk_off[b];
  const size_t N = (size_t)V.n_obs;
  const int* ab = V.a_boff[kind];
  const double* Wk = V.Wp[kind];
  const int wd = V.wdim[kind];
  double acc[BD * BD];
#pragma unroll
  for (int e = 0; e < BD * BD; ++e) acc[e] = 0.0;
  if (ab != nullptr)  // (a kind without pairs: every observation is solo, the partials below are zeros)
  for (int o = V.chunk_beg[ch] + threadIdx.x; o < V.chunk_end[ch]; o += 64) {
    if ((V.solo[o] >> kind) & 1) continue;  // no partner in this block
    const int xi = V.o_pt[o];
    if (V.pt_off[xi] < 0) continue;
    const int a = V.c2a[o];
    const double* Ci = Cinv + 9 * (size_t)xi;
    double W1[BD][3];
#pragma unroll
    for (int x = 0; x < BD; ++x)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        W1[x][c] = (x < dim) ? blk_col(V, kind, 0, x)[o] * V.Jpt[(size_t)c * N + a] +
                                   blk_col(V, kind, 1, x)[o] * V.Jpt[(size_t)(3 + c) * N + a]
                             : 0.0;
    double T[BD][3];  // W1 * Cinv
#pragma unroll
    for (int x = 0; x < BD; ++x)
#pragma unroll
      for (int c = 0; c < 3; ++c) T[x][c] = W1[x][0] * Ci[c] + W1[x][1] * Ci[3 + c] + W1[x][2] * Ci[6 + c];
    for (int a2 = V.pt_ptr[xi]; a2 < V.pt_ptr[xi + 1]; ++a2) {
      if (a2 == a) continue;  // the self term is part of (I - G) in the Gram kernel
      if (ab[a2] != boff) continue;
      const double* w2 = Wk + (size_t)a2 * wd * 3;  // the partner's W (ba_obs_w_kernel: the same expression, the same bits)
#pragma unroll
      for (int y = 0; y < BD; ++y) {
        if (y >= dim) continue;
        const double W2[3] = {w2[y * 3], w2[y * 3 + 1], w2[y * 3 + 2]};
#pragma unroll
        for (int x = 0; x < BD; ++x)
          if (x < dim) acc[x * BD + y] -= T[x][0] * W2[0] + T[x][1] * W2[1] + T[x][2] * W2[2];
      }
    }
  }
#pragma unroll
  for (int x = 0; x < BD; ++x)
#pragma unroll
    for (int y = 0; y < BD; ++y)
      if (x < dim && y < dim) {
        const double sx = wave_sum(acc[x * BD + y]);
        if (threadIdx.x == 0) V.cpart[(size_t)ch * BD * BD + x * dim + y] = sx;
      }
}

// ------------------------------------------------------------------------------------------
// Image-sharded solves: the cross-rank part of the Schur-Jacobi blocks of SHARED intrinsics.
// For an intrinsics block b and a point p let W_{b,p} = sum over the observations o of p that use b of
// J_b,o^T J_p,o (dim_b x 3). The block is M_b = B_b - sum_p W_{b,p} C_p^-1 W_{b,p}^T. A rank sees only its own
// observations: its G term plus its pair term is B_b^r - sum_p W^r C^-1 W^r^T, and the sum of that over the
// ranks misses every pair of observations of one point that sit on DIFFERENT ranks. Correction, for the
// (point, block) incidences whose observations span more than one rank (the host lists them; every rank sees the
// whole problem): all-reduce W, then
//   M_b += sum_p W^r C^-1 W^r^T                      (every rank, its own part: undoes what it subtracted)
//   M_b -= sum_{p : p mod world = rank} W C^-1 W^T    (the exact term, each incidence on one rank)
// before the all-reduce of M. The image-sharded solve then has the single-GPU preconditioner, CG trajectory and
// iteration counts (tests/test_ba_gpu.py: test_three_rank_sharded_solve_with_shared_intrinsics).
// ------------------------------------------------------------------------------------------
struct IncView {
  int n;                 // incidences that span ranks
  const int* pt;         // [n] point
  const int* blk;        // [n] block
  const int* ptr;        // [n + 1] this rank's observations of the incidence (c-order indices) ...
  const int* obs;        // ... as a CSR list
  // The incidences are sorted by block; a block's run is cut into chunks of <= kIncChunk of them (fixed-order sums:
  // ba_inc_correct_kernel writes one partial per chunk, ba_inc_finalize_kernel adds a block's partials in chunk order)
  int n_chunks;
  const int* chunk_blk;  // [n_chunks]
  const int* chunk_beg;  // [n_chunks + 1] first incidence of the chunk (chunk_beg[c + 1] = its end)
  const int* blk_chunk;  // [n_blk + 1] chunks of every block
  double* part;          // [n_chunks][KDT * KDT] partial sums
};
constexpr int kIncChunk = 128;
template <int KDT>
__global__ void ba_inc_w_kernel(View V, IncView I, double* __restrict__ W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I.n) return;
  const int dim = V.blk_dim[I.blk[i]];
  const size_t N = (size_t)V.n_obs;
  double w[KDT][3];
#pragma unroll
  for (int x = 0; x < KDT; ++x) w[x][0] = w[x][1] = w[x][2] = 0.0;
  for (int k = I.ptr[i]; k < I.ptr[i + 1]; ++k) {
    const int o = I.obs[k], a = V.c2a[o];
#pragma unroll
    for (int x = 0; x < KDT; ++x)
      if (x < dim) {
        const double j0 = blk_col(V, 1, 0, x)[o], j1 = blk_col(V, 1, 1, x)[o];
#pragma unroll
        for (int c = 0; c < 3; ++c) w[x][c] += j0 * V.Jpt[(size_t)c * N + a] + j1 * V.Jpt[(size_t)(3 + c) * N + a];
      }
  }
#pragma unroll
  for (int x = 0; x < KDT; ++x)
#pragma unroll
    for (int c = 0; c < 3; ++c) W[((size_t)i * KDT + x) * 3 + c] = w[x][c];
}
// One workgroup per chunk of incidences of ONE block, thread per entry (x, y) of the block: the thread walks the
// chunk's incidences in list order and writes its partial sum -- no atomics, the order of every sum is fixed by the
// host-built lists (a solve is reproducible run to run whatever the hardware's timing).
template <int KDT>
__global__ void __launch_bounds__(KDT * KDT) ba_inc_correct_kernel(View V, IncView I, const double* __restrict__ Cinv,
                                                                 const double* __restrict__ Wloc, const double* __restrict__ Wtot,
                                                                 int rank, int world) {
  const int ch = blockIdx.x;
  const int b = I.chunk_blk[ch], dim = V.blk_dim[b];
  const int x = threadIdx.x / KDT, y = threadIdx.x % KDT;
  double acc = 0.0;
  if (x < dim && y < dim) {
    for (int i = I.chunk_beg[ch]; i < I.chunk_beg[ch + 1]; ++i) {
      const int xi = I.pt[i];
      if (V.pt_off[xi] < 0) continue;  // a constant point has no C^-1: its observations do not couple
      const double* Ci = Cinv + 9 * (size_t)xi;
      const bool mine = xi % world == rank;
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && !mine) break;
        const double* Wp = (pass == 0 ? Wloc : Wtot) + (size_t)i * KDT * 3;
        const double t0 = Wp[x * 3 + 0] * Ci[0] + Wp[x * 3 + 1] * Ci[3] + Wp[x * 3 + 2] * Ci[6];
        const double t1 = Wp[x * 3 + 0] * Ci[1] + Wp[x * 3 + 1] * Ci[4] + Wp[x * 3 + 2] * Ci[7];
        const double t2 = Wp[x * 3 + 0] * Ci[2] + Wp[x * 3 + 1] * Ci[5] + Wp[x * 3 + 2] * Ci[8];
        const double term = t0 * Wp[y * 3 + 0] + t1 * Wp[y * 3 + 1] + t2 * Wp[y * 3 + 2];
        acc += pass == 0 ? term : -term;
      }
    }
  }
  I.part[(size_t)ch * KDT * KDT + threadIdx.x] = acc;
}
// M_b += the block's chunk partials, in chunk order; thread per (block, entry)
template <int KDT>
__global__ void ba_inc_finalize_kernel(View V, IncView I, double* __restrict__ M) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = t / (KDT * KDT), e = t % (KDT * KDT);
  if (b >= V.n_blk) return;
  const int c0 = I.blk_chunk[b], c1 = I.blk_chunk[b + 1];
  if (c0 == c1) return;
  const int dim = V.blk_dim[b], x = e / KDT, y = e % KDT;
  if (x >= dim || y >= dim) return;
  double s = 0.0;
  for (int c = c0; c < c1; ++c) s += I.part[(size_t)c * KDT * KDT + e];
  M[V.blk_moff[b] + x * dim + y] += s;
}

// ------------------------------------------------------------------------------------------
// Single GPU: the pair terms of the Schur-Jacobi blocks per INCIDENCE instead of per pair.
// For a point p and a block b that holds t >= 2 of p's observations the cross terms are
//   - sum_{o != o2} W_o C^-1 W_o2^T  =  - ( Ws C^-1 Ws^T - sum_o W_o C^-1 W_o^T ),   Ws = sum_o W_o,
// t + 1 products instead of t (t - 1): ba_block_schur_cross_kernel walks every partner of every observation (O(t^2) per
// incidence, 1.26 ms at BA-1 with one shared camera). The host lists the incidences sorted by block (PairView = the
// IncView layout, `obs` holding p-order observation indices), W_o comes from the p-order buffer of ba_obs_w_kernel (an
// incidence's members are neighbours there). One workgroup per chunk of <= kPairChunk incidences of ONE block, thread per
// entry (x, y), partial per chunk; ba_pair_finalize_kernel adds a block's partials with a fixed tree. No atomics.
// (Small chunks: a workgroup walks its incidences one after the other with dim^2 of its KDT^2 lanes busy -- what makes it
// fast is many workgroups in flight, 6 250 at BA-1 with one shared camera.)
// ------------------------------------------------------------------------------------------
constexpr int kPairChunk = 32;
template <int KDT>
__global__ void __launch_bounds__(KDT * KDT) ba_pair_cross_kernel(View V, IncView I, const double* __restrict__ Cinv) {
  const int ch = blockIdx.x;
  const int b = I.chunk_blk[ch], dim = V.blk_dim[b], kind = V.blk_kind[b];
  const int x = threadIdx.x / KDT, y = threadIdx.x % KDT;
  const double* Wk = V.Wp[kind];
  const int ws = V.wdim[kind] * 3;
  double acc = 0.0;
  if (x < dim && y < dim) {
    for (int i = I.chunk_beg[ch]; i < I.chunk_beg[ch + 1]; ++i) {
      const double* Ci = Cinv + 9 * (size_t)I.pt[i];
      double sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0}, self = 0.0;
      for (int k = I.ptr[i]; k < I.ptr[i + 1]; ++k) {
        const double* w = Wk + (size_t)I.obs[k] * ws;
        const double wx0 = w[x * 3], wx1 = w[x * 3 + 1], wx2 = w[x * 3 + 2];
        const double wy0 = w[y * 3], wy1 = w[y * 3 + 1], wy2 = w[y * 3 + 2];
        sx[0] += wx0; sx[1] += wx1; sx[2] += wx2;
        sy[0] += wy0; sy[1] += wy1; sy[2] += wy2;
        const double t0 = wx0 * Ci[0] + wx1 * Ci[3] + wx2 * Ci[6];
        const double t1 = wx0 * Ci[1] + wx1 * Ci[4] + wx2 * Ci[7];
        const double t2 = wx0 * Ci[2] + wx1 * Ci[5] + wx2 * Ci[8];
        self += t0 * wy0 + t1 * wy1 + t2 * wy2;
      }
      const double t0 = sx[0] * Ci[0] + sx[1] * Ci[3] + sx[2] * Ci[6];
      const double t1 = sx[0] * Ci[1] + sx[1] * Ci[4] + sx[2] * Ci[7];
      const double t2 = sx[0] * Ci[2] + sx[1] * Ci[5] + sx[2] * Ci[8];
      acc -= (t0 * sy[0] + t1 * sy[1] + t2 * sy[2]) - self;
    }
  }
  I.part[(size_t)ch * KDT * KDT + threadIdx.x] = acc;
}
// M_b += the partials of block b's chunks: one workgroup per block that has pair incidences (I.pair_blk), 64 entries per
// grid.y slice, 16 threads per entry striding over the chunks, their sums added in thread order (a fixed tree).
template <int KDT>
__global__ void __launch_bounds__(1024) ba_pair_finalize_kernel(View V, IncView I, const int* __restrict__ pair_blk,
                                                                double* __restrict__ M) {
  __shared__ double part[1024];
  const int b = pair_blk[blockIdx.x];
  const int el = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int e = el + 64 * blockIdx.y;
  const int c0 = I.blk_chunk[b], c1 = I.blk_chunk[b + 1];
  double s = 0.0;
  if (e < KDT * KDT)
    for (int c = c0 + g; c < c1; c += 16) s += I.part[(size_t)c * KDT * KDT + e];
  part[threadIdx.x] = s;
  __syncthreads();
  const int dim = V.blk_dim[b], x = e / KDT, y = e % KDT;
  if (g == 0 && e < KDT * KDT && x < dim && y < dim) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += part[k * 64 + el];
    M[V.blk_moff[b] + x * dim + y] += t;
  }
}

// M_b += Dc^2 on the diagonal, then invert (Gauss-Jordan with partial pivoting); lane per block
template <int BD>
__global__ void __launch_bounds__(64) ba_block_invert_kernel(View V, const double* __restrict__ Dc, const double* __restrict__ M,
                                       double* __restrict__ Minv) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= V.n_blk) return;
  const int n = V.blk_dim[b], off = V.blk_off[b];
  double A[BD][2 * BD];
  if constexpr (BD <= 8) {
    // The same Gauss-Jordan elimination with partial pivoting, every loop unrolled to the template width and
    // predicated on n, the row exchange written as selects: all indices are compile-time constants, so the
    // augmented matrix lives in registers (the rolled version below keeps it in scratch: 80 us for 2 000 blocks).
#pragma unroll
    for (int i = 0; i < BD; ++i) {
#pragma unroll
      for (int j = 0; j < BD; ++j) A[i][j] = (i < n && j < n) ? M[V.blk_moff[b] + i * n + j] : (i == j ? 1.0 : 0.0);
#pragma unroll
      for (int j = 0; j < BD; ++j) A[i][BD + j] = (i == j) ? 1.0 : 0.0;
      if (i < n) A[i][i] += Dc[off + i] * Dc[off + i];
    }
#pragma unroll
    for (int c = 0; c < BD; ++c) {
      if (c < n) {
        int piv = c;
        double best = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < BD; ++r)
          if (r < n && fabs(A[r][c]) > best) { best = fabs(A[r][c]); piv = r; }
#pragma unroll
        for (int r = c + 1; r < BD; ++r) {
          const bool sw = piv == r;
#pragma unroll
          for (int j = 0; j < 2 * BD; ++j) {
            const double t = A[c][j], u = A[r][j];
            A[c][j] = sw ? u : t;
            A[r][j] = sw ? t : u;
          }
        }
        const double inv = 1.0 / A[c][c];
#pragma unroll
        for (int j = 0; j < 2 * BD; ++j) A[c][j] *= inv;
#pragma unroll
        for (int r = 0; r < BD; ++r) {
          if (r == c || r >= n) continue;
          const double f = A[r][c];
#pragma unroll
          for (int j = 0; j < 2 * BD; ++j) A[r][j] -= f * A[c][j];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < BD; ++i)
#pragma unroll
      for (int j = 0; j < BD; ++j)
        if (i < n && j < n) Minv[V.blk_moff[b] + i * n + j] = A[i][BD + j];
    return;
  }
  for (int i = 0; i < BD; ++i)
    for (int j = 0; j < 2 * BD; ++j) A[i][j] = 0.0;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) A[i][j] = M[V.blk_moff[b] + i * n + j];
    A[i][i] += Dc[off + i] * Dc[off + i];
    A[i][BD + i] = 1.0;
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
    if (piv != c)
      for (int j = 0; j < 2 * BD; ++j) { const double t = A[c][j]; A[c][j] = A[piv][j]; A[piv][j] = t; }
    const double inv = 1.0 / A[c][c];
    for (int j = 0; j < 2 * BD; ++j) A[c][j] *= inv;
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = A[r][c];
      for (int j = 0; j < 2 * BD; ++j) A[r][j] -= f * A[c][j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) Minv[V.blk_moff[b] + i * n + j] = A[i][BD + j];
}

// ------------------------------------------------------------------------------------------
// Small vector kernels (camera-side vectors are a few thousand entries)
// ------------------------------------------------------------------------------------------
__global__ void ba_lm_diag_kernel(int n, const double* __restrict__ diag, double radius, double lo, double hi,
                                  double* __restrict__ D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) D[i] = sqrt(fmin(fmax(diag[i], lo), hi) / radius);
}
__global__ void ba_scale_kernel(int n, const double* __restrict__ diag, int enable, double* __restrict__ s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) s[i] = enable ? 1.0 / (1.0 + sqrt(diag[i])) : 1.0;
}
__global__ void ba_add_kernel(int n, const double* __restrict__ x, double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] += x[i];
}
__global__ void ba_dsq_x_kernel(int n, const double* __restrict__ D, const double* __restrict__ x,
                                double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = D[i] * D[i] * x[i];
}
// z_b = Minv_b r_b, lane per block over many workgroups; rho = r.z as one partial per workgroup
// (fixed tree inside a workgroup, partials added in index order by pcg_rho: deterministic).
__global__ void __launch_bounds__(256) ba_pcg_precond_kernel(View V, const double* __restrict__ Minv,
                                                             const double* __restrict__ r,
                                                             double* __restrict__ z, double* __restrict__ part) {
  double rho = 0.0;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < V.n_blk) {
    const int n = V.blk_dim[b], off = V.blk_off[b];
    const double* Mi = Minv + V.blk_moff[b];
    for (int i = 0; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += Mi[i * n + j] * r[off + j];
      z[off + i] = s;
      rho += s * r[off + i];
    }
  }
  rho = block_sum(rho);
  if (threadIdx.x == 0) part[blockIdx.x] = rho;
}
__device__ __forceinline__ double pcg_rho(const double* __restrict__ part, int nparts) {
  double rho = 0.0;
  for (int w = 0; w < nparts; ++w) rho += part[w];
  return rho;
}
// p = z + (rho / rho_last) p   (first iteration: p = z)
__global__ void ba_pcg_dir_kernel(int n, const double* __restrict__ scalars, const double* __restrict__ part,
                                  int nparts, int first, const double* __restrict__ z, double* __restrict__ p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  p[i] = first ? z[i] : z[i] + (pcg_rho(part, nparts) / scalars[S_RHO_LAST]) * p[i];
}

// ---------------------------------------------------------------------------
// Pipelined PCG (single GPU, no priors): three small multi-workgroup kernels per iteration around the three
// streaming kernels of the implicit product, the stopping test on the device, the host one iteration behind.
//   dir_k   (thread per entry)  closes iteration k-1 -- Q = sum of its partials, the stopping test of Ceres'
//           CG (zeta = k (Q_k - Q_{k-1}) / Q_k < eta), the iteration's scalars into a pinned host slot -- and, unless
//           it stopped, p = z + (rho_k / rho_{k-1}) p;
//   tail_k  (lane per block)    q_b = Dc_b^2 p_b + sum of the block's J_b^T v chunk partials, partials of p.q;
//   step_k  (lane per block)    alpha = rho / pq, x += alpha p, r -= alpha q, partials of Q = -x.(b + r) / 2,
//           z_b = Minv_b r_b, partials of rho' = r.z.
// Sums over workgroups are added by every wave that needs them in one fixed order (pcg_sum: strided lanes, then the
// xor tree): deterministic, the same bits everywhere.
// Partials alternate between two banks by iteration parity, so a kernel never reads what its own grid is writing.
// The host enqueues iteration k+1 before it looks at iteration k; once the device has set `stop` every later kernel
// (the streaming kernels through View::stop) returns at entry.
// ---------------------------------------------------------------------------
struct PcgHostSlot {
  double rho, pq, Q;
  int stop, iter;
};
struct PcgDev {
  double* part;        // [2 banks][3: pq, rho, Q][nparts]
  int nparts;
  int* stop;           // device flag
  PcgHostSlot* host;   // [2] pinned, device-visible
  double* qhist;       // [2] Q of the last two iterations
};
// (every wave of every workgroup adds the partials alike -- lane l takes the entries l, l + 64, ..., then the fixed
//  xor tree of wave_sum: one load round trip whatever nparts is, and the same bits in every wave. All 64 lanes of
//  the calling wave must be here.)
constexpr int PCGP_T = 64;  // lanes (= blocks) per workgroup of the init / tail / step kernels: 4 x the CUs of 256
__device__ __forceinline__ double pcg_sum(const double* __restrict__ part, int nparts) {
  double s = 0.0;
  for (int w = (int)(threadIdx.x & 63); w < nparts; w += 64) s += part[w];
  return wave_sum(s);
}
// x = 0, r = b, z = Minv r, partials of rho_1 into bank 1 (component loops unrolled to the block width like the step
// kernel's: the sums in the rolled order)
template <int BD>
__global__ void __launch_bounds__(PCGP_T) ba_pcgp_init_kernel(View V, PcgDev D, const double* __restrict__ Minv,
                                                           const double* __restrict__ rhs, double* __restrict__ x,
                                                           double* __restrict__ r, double* __restrict__ z) {
  double rho = 0.0;
  const int b = blockIdx.x * PCGP_T + threadIdx.x;
  if (b < V.n_blk) {
    const int n = V.blk_dim[b], off = V.blk_off[b];
    const double* Mi = Minv + V.blk_moff[b];
    double bv[BD];
#pragma unroll
    for (int i = 0; i < BD; ++i) bv[i] = i < n ? rhs[off + i] : 0.0;
    double mi[BD][BD];
    if constexpr (BD <= 8) {
#pragma unroll
      for (int i = 0; i < BD; ++i)
#pragma unroll
        for (int j = 0; j < BD; ++j) mi[i][j] = (i < n && j < n) ? Mi[i * n + j] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < BD; ++i)
      if (i < n) { x[off + i] = 0.0; r[off + i] = bv[i]; }
#pragma unroll
    for (int i = 0; i < BD; ++i) {
      if (i < n) {
        double sacc = 0.0;
        if constexpr (BD <= 8) {
#pragma unroll
          for (int j = 0; j < BD; ++j)
            if (j < n) sacc += mi[i][j] * bv[j];
        } else {
#pragma unroll
          for (int j = 0; j < BD; ++j)
            if (j < n) sacc += Mi[i * n + j] * bv[j];
        }
        z[off + i] = sacc;
        rho += sacc * bv[i];
      }
    }
  }
  rho = block_sum(rho);
  if (threadIdx.x == 0) D.part[(1 * 3 + 1) * D.nparts + blockIdx.x] = rho;
  if (blockIdx.x == 0 && threadIdx.x == 0) { *D.stop = 0; D.qhist[0] = 0.0; D.qhist[1] = 0.0; }
}
__global__ void ba_pcgp_dir_kernel(int n, PcgDev D, int k, int max_iter, double q_tol, const double* __restrict__ z,
                                   double* __restrict__ p) {
  if (*D.stop) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const double* bank_prev = D.part + (size_t)((k - 1) & 1) * 3 * D.nparts;   // what iteration k-1 consumed / produced
  const double* bank = D.part + (size_t)(k & 1) * 3 * D.nparts;
  const double rho_new = pcg_sum(bank + D.nparts, D.nparts);                // rho_k
  bool stop = false;
  double rho_prev = 0.0, pq = 0.0, Q1 = 0.0;
  if (k == 1) {
    stop = rho_new == 0.0;                                                    // zero right-hand side: nothing to solve
  } else {
    rho_prev = pcg_sum(bank_prev + D.nparts, D.nparts);                       // rho_{k-1}
    pq = pcg_sum(bank_prev, D.nparts);
    Q1 = pcg_sum(bank_prev + 2 * D.nparts, D.nparts);
    const double Q0 = D.qhist[k & 1];                                         // Q_{k-2}
    const int it = k - 1;
    if (!(rho_prev > 0.0) || !isfinite(rho_prev) || !(pq > 0.0) || !isfinite(pq)) stop = true;
    else if ((double)it * (Q1 - Q0) / Q1 < q_tol) stop = true;
    else if (it >= max_iter) stop = true;
  }
  if (i == 0) {
    PcgHostSlot h;
    h.rho = rho_prev; h.pq = pq; h.Q = Q1; h.stop = stop ? 1 : 0; h.iter = k - 1;
    D.host[(k - 1) & 1] = h;
    if (k > 1) D.qhist[(k - 1) & 1] = Q1;
    __threadfence_system();
  }
  if (stop) {
    // every workgroup decides alike from the same partials; the flag is for the kernels behind this one. No
    // workgroup may return before all have read it as 0, which the kernel boundary cannot give: workgroups that
    // start late would see 1 and skip -- harmless, they would have stopped as well.
    if (i == 0) *D.stop = 1;
    return;
  }
  if (i >= n) return;
  p[i] = k == 1 ? z[i] : z[i] + (rho_new / rho_prev) * p[i];
}
// (tail and step kernels: a lane per block, every loop over the block's components unrolled to the template width and
//  predicated on its dimension -- rolled, each trip waited for its own loads: 6 - 12 dependent round trips per lane and
//  launch; the order of every sum is the rolled loops', so the results are bit-identical)
// `reduced` (point-sharded solves): J_c^T v of every block, already summed over the block's chunks AND over the ranks
// (ba_block_vec_finalize_kernel + all-reduce) -- the tail then only adds D^2 p and takes p.q; null: this GPU's chunk
// partials are the whole sum.
template <int BD>
__global__ void __launch_bounds__(PCGP_T) ba_pcgp_tail_kernel(View V, PcgDev D, int k, const double* __restrict__ Dc,
                                                           const double* __restrict__ p, double* __restrict__ q,
                                                           const double* __restrict__ reduced) {
  if (*D.stop) return;
  const int bd2 = V.bd * V.bd;
  double pq = 0.0;
  const int b = blockIdx.x * PCGP_T + threadIdx.x;
  if (b < V.n_blk) {
    const int dim = V.blk_dim[b], off = V.blk_off[b];
    const int ch0 = V.blk_chunk_ptr[b], ch1 = V.blk_fin_end[b];
    double sacc[BD], d[BD], pv[BD];
#pragma unroll
    for (int c = 0; c < BD; ++c) {
      sacc[c] = 0.0;
      d[c] = c < dim ? Dc[off + c] : 0.0;
      pv[c] = c < dim ? p[off + c] : 0.0;
    }
    if (reduced) {
#pragma unroll
      for (int c = 0; c < BD; ++c) sacc[c] = c < dim ? reduced[off + c] : 0.0;
    } else {
      for (int ch = ch0; ch < ch1; ch += 4) {  // four chunks' rows per round trip, added in chunk order
        double row[4][BD];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < BD; ++c) row[k][c] = (ch + k < ch1 && c < dim) ? V.cpart[(size_t)(ch + k) * bd2 + c] : 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ch + k < ch1) {
#pragma unroll
            for (int c = 0; c < BD; ++c) sacc[c] += row[k][c];
          }
      }
    }
#pragma unroll
    for (int c = 0; c < BD; ++c) {
      if (c < dim) {
        const double qv = d[c] * d[c] * pv[c] + sacc[c];
        q[off + c] = qv;
        pq += pv[c] * qv;
      }
    }
  }
  pq = block_sum(pq);
  if (threadIdx.x == 0) D.part[(size_t)(k & 1) * 3 * D.nparts + blockIdx.x] = pq;
}
template <int BD>
__global__ void __launch_bounds__(PCGP_T) ba_pcgp_step_kernel(View V, PcgDev D, int k, const double* __restrict__ Minv,
                                                           const double* __restrict__ rhs, const double* __restrict__ p,
                                                           const double* __restrict__ q, double* __restrict__ x,
                                                           double* __restrict__ r, double* __restrict__ z) {
  if (*D.stop) return;
  double* bank = D.part + (size_t)(k & 1) * 3 * D.nparts;
  double* bank_next = D.part + (size_t)((k + 1) & 1) * 3 * D.nparts;
  const double alpha = pcg_sum(bank + D.nparts, D.nparts) / pcg_sum(bank, D.nparts);
  double Q = 0.0, rho = 0.0;
  const int b = blockIdx.x * PCGP_T + threadIdx.x;
  if (b < V.n_blk) {
    const int n = V.blk_dim[b], off = V.blk_off[b];
    const double* Mi = Minv + V.blk_moff[b];
    double xv[BD], pv[BD], rv[BD], qv[BD], bv[BD];
#pragma unroll
    for (int i = 0; i < BD; ++i) {
      const bool ok = i < n;
      xv[i] = ok ? x[off + i] : 0.0;
      pv[i] = ok ? p[off + i] : 0.0;
      rv[i] = ok ? r[off + i] : 0.0;
      qv[i] = ok ? q[off + i] : 0.0;
      bv[i] = ok ? rhs[off + i] : 0.0;
    }
    double mi[BD][BD];
    if constexpr (BD <= 8) {
#pragma unroll
      for (int i = 0; i < BD; ++i)
#pragma unroll
        for (int j = 0; j < BD; ++j) mi[i][j] = (i < n && j < n) ? Mi[i * n + j] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < BD; ++i) {
      if (i < n) {
        const double xn = xv[i] + alpha * pv[i];
        const double rn = rv[i] - alpha * qv[i];
        x[off + i] = xn;
        r[off + i] = rn;
        rv[i] = rn;
        Q += -0.5 * xn * (bv[i] + rn);
      }
    }
#pragma unroll
    for (int i = 0; i < BD; ++i) {
      if (i < n) {
        double sacc = 0.0;
        if constexpr (BD <= 8) {
#pragma unroll
          for (int j = 0; j < BD; ++j)
            if (j < n) sacc += mi[i][j] * rv[j];
        } else {  // (the 16-wide tier: 256 matrix entries per lane do not fit in registers)
#pragma unroll
          for (int j = 0; j < BD; ++j)
            if (j < n) sacc += Mi[i * n + j] * rv[j];
        }
        z[off + i] = sacc;
        rho += sacc * rv[i];
      }
    }
  }
  Q = block_sum(Q);
  rho = block_sum(rho);
  if (threadIdx.x == 0) {
    bank[2 * D.nparts + blockIdx.x] = Q;
    bank_next[D.nparts + blockIdx.x] = rho;
  }
}

__global__ void __launch_bounds__(1024) ba_dot_kernel(int n, const double* __restrict__ a,
                                                      const double* __restrict__ b, double* __restrict__ out) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) v += a[i] * b[i];
  v = block_sum(v);
  if (threadIdx.x == 0) *out = v;
}
// pq = p.q ; alpha = rho / pq ; x += alpha p ; r -= alpha q ; Q = -0.5 x (b + r); publishes rho
// (for the host and as the next iteration's rho_last)
__global__ void __launch_bounds__(1024) ba_pcg_update_kernel(int n, double* __restrict__ scalars,
                                                             const double* __restrict__ part, int nparts,
                                                             const double* __restrict__ p,
                                                             const double* __restrict__ q,
                                                             const double* __restrict__ b, double* __restrict__ x,
                                                             double* __restrict__ r) {
  double pq = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) pq += p[i] * q[i];
  pq = block_sum(pq);
  const double rho = pcg_rho(part, nparts);
  double Q = 0.0;
  const double alpha = rho / pq;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double xn = x[i] + alpha * p[i];
    const double rn = r[i] - alpha * q[i];
    x[i] = xn;
    r[i] = rn;
    Q += -0.5 * xn * (b[i] + rn);
  }
  Q = block_sum(Q);
  if (threadIdx.x == 0) {
    scalars[S_Q] = Q;
    scalars[S_PQ] = pq;
    scalars[S_RHO] = rho;
    scalars[S_RHO_LAST] = rho;
  }
}
// y = a * x / s  (s may be null)
__global__ void ba_axpby_kernel(int n, double a, const double* __restrict__ x, const double* __restrict__ s,
                                double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = a * x[i] * (s ? s[i] : 1.0);
}

// x_plus = Plus(x, step): quaternion (x) translation, subset of intrinsics, points -- ONE launch for all parameter
// blocks (workgroups are dealt to points, poses, cameras, sensors in that order), and the step is read through a
// StepSrc, so that the vector kernels that used to prepare it are gone:
//   tf 0: step = a            tf 1: step = (-1 * a) / s   (projected-gradient test: a = scaled gradient, s = column scale)
//   tf 3: step = (-a) * s     (candidate: a = the solver's y, s = column scale)          -- the same roundings as
// two vector kernels (y = a x / s, y = a x s) applied one after the other, which this replaces.
// MAXDIFF: also max |x_plus - x| over everything -> scalars[S_GMAX] (replaces three ba_maxdiff launches).
struct StepSrc {
  const double* a;
  const double* s;
  int tf;
};
__device__ __forceinline__ double step_val(const StepSrc& S, int k) {
  const double x = S.a[k];
  return S.tf == 0 ? x : S.tf == 1 ? (-1.0 * x) / S.s[k] : (-1.0 * x) * S.s[k];
}
__device__ __forceinline__ double plus_quat_trans(const double* q, double* o, const double d[6], bool rotc, int fix) {
  for (int c = 0; c < 7; ++c) o[c] = q[c];
  const double n = rotc ? 0.0 : sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (n != 0.0) {
    const double s = sin(n) / n;
    const double dx = s * d[0], dy = s * d[1], dz = s * d[2], dw = cos(n);
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    o[0] = dw * x + dx * w + dy * z - dz * y;
    o[1] = dw * y - dx * z + dy * w + dz * x;
    o[2] = dw * z + dx * y - dy * x + dz * w;
    o[3] = dw * w - dx * x - dy * y - dz * z;
  }
  int k = rotc ? 0 : 3;
  for (int c = 0; c < 3; ++c) {
    if (c == fix) continue;
    o[4 + c] += d[k++];
  }
  double m = 0.0;
  for (int c = 0; c < 7; ++c) m = fmax(m, fabs(o[c] - q[c]));
  return m;
}
template <bool MAXDIFF>
__global__ void __launch_bounds__(128) ba_apply_all_kernel(View V, StepSrc Sc, StepSrc Sp, const double* __restrict__ Pin,
                                                           double* __restrict__ P2, const double* __restrict__ Cin,
                                                           double* __restrict__ C2, const double* __restrict__ Xin,
                                                           double* __restrict__ X2, const double* __restrict__ Sin,
                                                           double* __restrict__ S2) {
  const int nb_pt = (V.n_points + 127) / 128, nb_pose = (V.n_poses + 127) / 128, nb_cam = (V.n_cams + 127) / 128;
  int blk = blockIdx.x;
  double m = 0.0;
  if (blk < nb_pt) {
    const int j = blk * 128 + threadIdx.x;
    if (j < V.n_points) {
      const int off = V.pt_off[j];
      for (int c = 0; c < 3; ++c) {
        const double xin = Xin[3 * (size_t)j + c];
        const double xo = xin + (off >= 0 ? step_val(Sp, off + c) : 0.0);
        X2[3 * (size_t)j + c] = xo;
        m = fmax(m, fabs(xo - xin));
      }
    }
  } else if ((blk -= nb_pt) < nb_pose) {
    const int i = blk * 128 + threadIdx.x;
    if (i < V.n_poses) {
      const double* q = Pin + 7 * (size_t)i;
      double* o = P2 + 7 * (size_t)i;
      const int off = V.pose_off[i];
      if (off < 0) {
        for (int c = 0; c < 7; ++c) o[c] = q[c];
      } else {
        const int pf = V.pose_fix[i];
        const bool rotc = pf >= 4;
        const int fix = pf < 0 ? -1 : ((pf & 3) == 3 ? -1 : (pf & 3));
        const int dim = V.pose_dim[i];
        double d[6];
        for (int c = 0; c < 6; ++c) d[c] = c < dim ? step_val(Sc, off + c) : 0.0;
        m = plus_quat_trans(q, o, d, rotc, fix);
      }
    }
  } else if ((blk -= nb_pose) < nb_cam) {
    const int k = blk * 128 + threadIdx.x;
    if (k < V.n_cams) {
      for (int c = 0; c < BA_CAM_STRIDE; ++c) C2[BA_CAM_STRIDE * (size_t)k + c] = Cin[BA_CAM_STRIDE * (size_t)k + c];
      const int off = V.cam_off[k];
      if (off >= 0)
        for (int d = 0; d < V.cam_dim[k]; ++d) {
          const int idx = V.cam_var[V.kd * k + d];
          const double cin = Cin[BA_CAM_STRIDE * (size_t)k + idx];
          const double co = cin + step_val(Sc, off + d);
          C2[BA_CAM_STRIDE * (size_t)k + idx] = co;
          m = fmax(m, fabs(co - cin));
        }
    }
  } else {
    blk -= nb_cam;
    const int i = blk * 128 + threadIdx.x;
    if (i < V.n_sensors) {
      const double* q = Sin + 7 * (size_t)i;
      double* o = S2 + 7 * (size_t)i;
      const int off = V.sens_off ? V.sens_off[i] : -1;
      if (off < 0) {
        for (int c = 0; c < 7; ++c) o[c] = q[c];
      } else {
        double d[6];
        for (int c = 0; c < 6; ++c) d[c] = step_val(Sc, off + c);
        m = plus_quat_trans(q, o, d, false, -1);
      }
    }
  }
  if (MAXDIFF) {
    // one atomic per workgroup, and only from a workgroup that can still raise the maximum (3 000 waves hammering one
    // address cost 37 us at BA-1; the max is order-independent, so skipping a value that is not above it changes nothing)
    __shared__ double wmax[2];
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      m = fmax(wmax[0], wmax[1]);
      const double cur = __longlong_as_double((long long)__atomic_load_n(
          reinterpret_cast<const unsigned long long*>(V.scalars + S_GMAX), __ATOMIC_RELAXED));
      if (m > cur) atomic_max_pos(V.scalars + S_GMAX, m);
    }
  }
}
__global__ void ba_renorm_sensor_quat_kernel(View V, double* __restrict__ sensors) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.n_sensors || !V.sens_off || V.sens_off[i] < 0) return;
  double* q = sensors + 7 * (size_t)i;
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int c = 0; c < 4; ++c) q[c] /= n;
}
// point sharding: zero the variable points another rank owns (point index % world != rank)
__global__ void ba_keep_own_points_kernel(View V, int rank, int world, double* __restrict__ points) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points || V.pt_off[j] < 0 || j % world == rank) return;
  points[3 * (size_t)j] = points[3 * (size_t)j + 1] = points[3 * (size_t)j + 2] = 0.0;
}

__global__ void ba_renorm_quat_kernel(View V, double* __restrict__ poses) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.n_poses || V.pose_off[i] < 0) return;
  double* q = poses + 7 * (size_t)i;
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int c = 0; c < 4; ++c) q[c] /= n;
}

// ------------------------------------------------------------------------------------------
// Host-side solver
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// Position priors (PosePriorBundleAdjuster, bundle_adjustment_ceres.cc:900-1038;
// AbsolutePosePositionPriorCostFunctor / AbsoluteRigPosePositionPriorCostFunctor,
// cost_functions/pose_prior.h:76-129). A prior is a 3-residual block on a pose block and, for an image
// that is not the reference sensor of its frame, on its sensor_from_rig block. It has no point block:
// it adds to the camera side of the normal equations directly. There are at most as many priors as
// images, so the kernels are small; sums run in a fixed order (one lane per target block walks its
// priors, single-workgroup tree reductions for the scalars) to keep the solve bit-reproducible.
// ------------------------------------------------------------------------------------------
struct PriorView {
  int n;                     // active priors
  const int *pose, *sens;    // [n] pose block index; sensor_from_rig index or -1
  const double *pos, *A;     // [n][3] position, [n][9] left sqrt information (row-major)
  const int *po, *so;        // [n] tangent offsets (-1: constant block)
  const int *pdim;           // [n] pose tangent width (0 when constant)
  double *r;                 // [3][n] weighted, loss-corrected residual
  double *J;                 // [3][12][n] tangent columns: pose (pdim), then sensor (6), column scaled
  double *jx;                // [3][n] J x of the current product
  int loss_type;
  double loss_scale;
  // targets: (block, prior, first column) sorted by block; tb_ptr over the distinct blocks
  int n_tblk;
  const int *tb_blk, *tb_ptr, *tg_prior, *tg_base;
};

// r0 = position + R(q_r)^T (t_r + R(q_s)^T t_s) and its ambient Jacobians (3 x 7 each, row-major)
__device__ __forceinline__ void prior_residual(const double* pos, const double* pose, const double* sens, double r0[3],
                                               double* Jpose, double* Jsens) {
  double w[3] = {pose[4], pose[5], pose[6]};
  double Rs[9], Jqs[12];
  if (sens) {
    const double qsc[4] = {-sens[0], -sens[1], -sens[2], sens[3]};
    double v[3];
    quat_rotate(qsc, sens + 4, v, Jsens ? Jqs : nullptr);
    w[0] += v[0]; w[1] += v[1]; w[2] += v[2];
    quat_to_rot(sens, Rs);
  }
  const double qc[4] = {-pose[0], -pose[1], -pose[2], pose[3]};
  double v[3], Jq[12];
  quat_rotate(qc, w, v, Jpose ? Jq : nullptr);
  r0[0] = pos[0] + v[0]; r0[1] = pos[1] + v[1]; r0[2] = pos[2] + v[2];
  if (!Jpose) return;
  double Rr[9];
  quat_to_rot(pose, Rr);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Jpose[7 * r + c] = -Jq[4 * r + c];  // d conj(q) / d q
    Jpose[7 * r + 3] = Jq[4 * r + 3];
    for (int c = 0; c < 3; ++c) Jpose[7 * r + 4 + c] = Rr[3 * c + r];  // R_r^T
  }
  if (sens && Jsens) {
    double tmp[21];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 4; ++c) {
        const double a = Rr[r] * Jqs[c] + Rr[3 + r] * Jqs[4 + c] + Rr[6 + r] * Jqs[8 + c];
        tmp[7 * r + c] = c < 3 ? -a : a;
      }
      for (int c = 0; c < 3; ++c) tmp[7 * r + 4 + c] = Rr[r] * Rs[3 * c] + Rr[3 + r] * Rs[3 * c + 1] + Rr[6 + r] * Rs[3 * c + 2];
    }
    for (int e = 0; e < 21; ++e) Jsens[e] = tmp[e];
  }
}

// One workgroup: linearise every prior (JAC: residual + Jacobians), add the summed cost to *cost_slot
template <bool JAC>
__global__ void __launch_bounds__(256) ba_prior_linearize_kernel(View V, PriorView Q, const double* __restrict__ poses,
                                                                 const double* __restrict__ sensors,
                                                                 double* __restrict__ cost_slot) {
  __shared__ double red[256];
  double cost = 0.0;
  for (int k = threadIdx.x; k < Q.n; k += 256) {
    const int pi = Q.pose[k], si = Q.sens[k];
    const double* pose = poses + 7 * (size_t)pi;
    const double* sens = si >= 0 ? sensors + 7 * (size_t)si : nullptr;
    const int pdim = Q.pdim[k], so = Q.so[k], po = Q.po[k];
    double r0[3], Jpose[21], Jsens[21];
    prior_residual(Q.pos + 3 * (size_t)k, pose, sens, r0, JAC ? Jpose : nullptr, (JAC && so >= 0) ? Jsens : nullptr);
    const double* A = Q.A + 9 * (size_t)k;
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = A[3 * i] * r0[0] + A[3 * i + 1] * r0[1] + A[3 * i + 2] * r0[2];
    const double sq_norm = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    double rho[3];
    loss_eval(Q.loss_type, Q.loss_scale, sq_norm, rho);
    cost += 0.5 * rho[0];
    if (JAC) {
      double Jt[3][12];
      for (int i = 0; i < 3; ++i)
        for (int d = 0; d < 12; ++d) Jt[i][d] = 0.0;
      if (pdim > 0) {
        const double x = pose[0], y = pose[1], z = pose[2], w = pose[3];
        const double PJ[12] = {w, z, -y, -z, w, x, y, -x, w, -x, -y, -z};
        const int pf = V.pose_fix[pi];
        const bool rotc = pf >= 4;
        const int fix = pf < 0 ? -1 : ((pf & 3) == 3 ? -1 : (pf & 3));
        for (int i = 0; i < 3; ++i) {
          int d = 0;
          if (!rotc) {
            for (int c = 0; c < 3; ++c)
              Jt[i][c] = Jpose[7 * i] * PJ[c] + Jpose[7 * i + 1] * PJ[3 + c] + Jpose[7 * i + 2] * PJ[6 + c] +
                         Jpose[7 * i + 3] * PJ[9 + c];
            d = 3;
          }
          for (int c = 0; c < 3; ++c) {
            if (c == fix) continue;
            Jt[i][d++] = Jpose[7 * i + 4 + c];
          }
        }
      }
      if (so >= 0) {
        const double x = sens[0], y = sens[1], z = sens[2], w = sens[3];
        const double PJ[12] = {w, z, -y, -z, w, x, y, -x, w, -x, -y, -z};
        for (int i = 0; i < 3; ++i)
          for (int c = 0; c < 3; ++c) {
            Jt[i][pdim + c] = Jsens[7 * i] * PJ[c] + Jsens[7 * i + 1] * PJ[3 + c] + Jsens[7 * i + 2] * PJ[6 + c] +
                              Jsens[7 * i + 3] * PJ[9 + c];
            Jt[i][pdim + 3 + c] = Jsens[7 * i + 4 + c];
          }
      }
      const int wdt = pdim + (so >= 0 ? 6 : 0);
      double J[3][12];
      for (int i = 0; i < 3; ++i)
        for (int d = 0; d < 12; ++d)
          J[i][d] = d < wdt ? A[3 * i] * Jt[0][d] + A[3 * i + 1] * Jt[1][d] + A[3 * i + 2] * Jt[2][d] : 0.0;
      if (Q.loss_type != BA_LOSS_TRIVIAL) {  // ceres::internal::Corrector on the 3-residual block
        const double sqrt_rho1 = sqrt(rho[1]);
        double residual_scaling = sqrt_rho1, alpha_sq_norm = 0.0;
        if (!(sq_norm == 0.0 || rho[2] <= 0.0)) {
          const double D = 1.0 + 2.0 * sq_norm * rho[2] / rho[1];
          const double alpha = 1.0 - sqrt(D);
          residual_scaling = sqrt_rho1 / (1.0 - alpha);
          alpha_sq_norm = alpha / sq_norm;
        }
        for (int d = 0; d < wdt; ++d) {
          const double rtj = r[0] * J[0][d] + r[1] * J[1][d] + r[2] * J[2][d];
          for (int i = 0; i < 3; ++i) J[i][d] = sqrt_rho1 * (J[i][d] - alpha_sq_norm * r[i] * rtj);
        }
        for (int i = 0; i < 3; ++i) r[i] *= residual_scaling;
      }
      for (int i = 0; i < 3; ++i) {
        Q.r[(size_t)i * Q.n + k] = r[i];
        for (int d = 0; d < 12; ++d) {
          double sc = 1.0;
          if (d < pdim) sc = V.scale_c[po + d];
          else if (d < wdt) sc = V.scale_c[so + d - pdim];
          Q.J[((size_t)i * 12 + d) * Q.n + k] = J[i][d] * sc;
        }
      }
    }
  }
  red[threadIdx.x] = cost;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *cost_slot += red[0];
}

// jx_k = J_k x (3 per prior)
__global__ void ba_prior_jx_kernel(PriorView Q, const double* __restrict__ x) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Q.n) return;
  const int po = Q.po[k], so = Q.so[k], pdim = Q.pdim[k];
  for (int i = 0; i < 3; ++i) {
    double v = 0.0;
    for (int d = 0; d < pdim; ++d) v += Q.J[((size_t)i * 12 + d) * Q.n + k] * x[po + d];
    if (so >= 0)
      for (int d = 0; d < 6; ++d) v += Q.J[((size_t)i * 12 + pdim + d) * Q.n + k] * x[so + d];
    Q.jx[(size_t)i * Q.n + k] = v;
  }
}

// Lane per target block, its priors in list order.
// MODE 0: g += J^T r, diag += column norms; MODE 1: M_b += J^T J; MODE 2: y += J^T jx
template <int MODE>
__global__ void ba_prior_accumulate_kernel(View V, PriorView Q, double* __restrict__ out, double* __restrict__ diag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Q.n_tblk) return;
  const int b = Q.tb_blk[t];
  const int off = V.blk_off[b], dim = V.blk_dim[b];
  for (int e = Q.tb_ptr[t]; e < Q.tb_ptr[t + 1]; ++e) {
    const int k = Q.tg_prior[e], base = Q.tg_base[e];
    for (int i = 0; i < 3; ++i) {
      const double ri = MODE == 0 ? Q.r[(size_t)i * Q.n + k] : (MODE == 2 ? Q.jx[(size_t)i * Q.n + k] : 0.0);
      for (int x = 0; x < dim; ++x) {
        const double jx = Q.J[((size_t)i * 12 + base + x) * Q.n + k];
        if (MODE == 0) { out[off + x] += jx * ri; diag[off + x] += jx * jx; }
        if (MODE == 2) out[off + x] += jx * ri;
        if (MODE == 1)
          for (int y = 0; y < dim; ++y) out[V.blk_moff[b] + x * dim + y] += jx * Q.J[((size_t)i * 12 + base + y) * Q.n + k];
      }
    }
  }
}

// model cost change of the priors: - (J step) . (r + J step / 2), added to *slot (one workgroup)
__global__ void __launch_bounds__(256) ba_prior_model_kernel(PriorView Q, const double* __restrict__ step,
                                                             double* __restrict__ slot) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int k = threadIdx.x; k < Q.n; k += 256) {
    const int po = Q.po[k], so = Q.so[k], pdim = Q.pdim[k];
    for (int i = 0; i < 3; ++i) {
      double m = 0.0;
      for (int d = 0; d < pdim; ++d) m += Q.J[((size_t)i * 12 + d) * Q.n + k] * step[po + d];
      if (so >= 0)
        for (int d = 0; d < 6; ++d) m += Q.J[((size_t)i * 12 + pdim + d) * Q.n + k] * step[so + d];
      acc -= m * (Q.r[(size_t)i * Q.n + k] + 0.5 * m);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *slot += red[0];
}

// ------------------------------------------------------------------------------------------
// DENSE_SCHUR tier (ceres::DENSE_SCHUR as CreateSolverOptions selects it for <= 50 images,
// bundle_adjustment_ceres.cc:203-213): S is formed column by column through the implicit operator
// (S e_i), then factored and solved by one workgroup. n <= 1024.
// ------------------------------------------------------------------------------------------
__global__ void ba_unit_vector_kernel(int n, int i, double* __restrict__ e) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) e[k] = k == i ? 1.0 : 0.0;
}

// in-place lower Cholesky of the column-major (= row-major, S is symmetric) n x n matrix S, then
// x = S^-1 b. A non-positive pivot yields NaNs: the LM loop rejects the step like a failed LLT.
__global__ void __launch_bounds__(1024) ba_dense_cholesky_solve_kernel(int n, double* __restrict__ S,
                                                                       const double* __restrict__ b,
                                                                       double* __restrict__ x) {
  const int tid = threadIdx.x, T = blockDim.x;
  // S(i, j) = S[j * n + i]: column j is what the j-th operator product wrote
  for (int k = 0; k < n; ++k) {
    if (tid == 0) S[(size_t)k * n + k] = sqrt(S[(size_t)k * n + k]);
    __syncthreads();
    const double d = S[(size_t)k * n + k];
    for (int i = k + 1 + tid; i < n; i += T) S[(size_t)k * n + i] /= d;
    __syncthreads();
    // trailing update of the lower triangle: column j, rows i >= j
    const int m = n - k - 1;
    for (int e = tid; e < m * m; e += T) {
      const int j = k + 1 + e / m, i = k + 1 + e % m;
      if (i >= j) S[(size_t)j * n + i] -= S[(size_t)k * n + i] * S[(size_t)k * n + j];
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += T) x[i] = b[i];
  __syncthreads();
  for (int k = 0; k < n; ++k) {  // L y = b
    if (tid == 0) x[k] /= S[(size_t)k * n + k];
    __syncthreads();
    const double yk = x[k];
    for (int i = k + 1 + tid; i < n; i += T) x[i] -= S[(size_t)k * n + i] * yk;
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {  // L^T x = y
    if (tid == 0) x[k] /= S[(size_t)k * n + k];
    __syncthreads();
    const double xk = x[k];
    for (int i = tid; i < k; i += T) x[i] -= S[(size_t)i * n + k] * xk;
    __syncthreads();
  }
}

template <typename T>
struct Buf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    release();
    n = count;
    hipError_t e_alloc = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
    if (e_alloc == hipErrorOutOfMemory) {  // memory cached by the PatchMatch buffer pool is not "in use"
      (void)hipGetLastError();
      pm_release_cached_memory();
      e_alloc = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
    }
    BA_HIP(e_alloc);
    BA_HIP(hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T)));
  }
  T* upload(const std::vector<T>& h) {  // returns the device pointer: an upload and its view field are one statement
    alloc(h.size());
    if (!h.empty()) BA_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }
  // non-owning window into another buffer (sub-vectors of one all-reduce payload)
  void alias(T* ptr, size_t count) {
    release();
    p = ptr;
    n = count;
    owns = false;
  }
  void release() {
    if (p && owns) (void)hipFree(p);
    p = nullptr;
    n = 0;
    owns = true;
  }
  bool owns = true;
  ~Buf() { release(); }
};

// Owning stream / event handles: created in place, destroyed with their owner, converted to the raw handle on use.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  void create() { BA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  void create_lowest_priority() {
    int prio_least = 0, prio_greatest = 0;
    BA_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    BA_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio_least));
  }
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  void create(bool timing = true) { BA_HIP(timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
};

inline int grid_for(size_t n, int block) { return (int)((n + block - 1) / block); }

// sync + check after every launch; read per launch (an atomic load unless some switch is set), so that
// colmap_amd_set_switch("COLMAP_AMD_BA_DEBUG", "1") takes effect whenever it is called
static inline bool ba_debug() { return dev_switch_int("COLMAP_AMD_BA_DEBUG", 0) != 0; }
#define BA_LAUNCH(kernel, grid, block, stream, ...)                                    \
  do {                                                                                 \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                   \
    if (ba_debug()) {                                                                  \
      hipError_t e_ = hipStreamSynchronize(stream);                                    \
      if (e_ == hipSuccess) e_ = hipGetLastError();                                    \
      std::fprintf(stderr, "[ba] %s grid=%d -> %s\n", #kernel, (int)(grid).x, hipGetErrorString(e_)); \
      if (e_ != hipSuccess) throw std::runtime_error(std::string("kernel failed: ") + #kernel); \
    }                                                                                  \
  } while (0)

// The three width tiers <KD, BD> of a problem (see the constants at the top of the file), as types whose widths
// instantiate the kernels. KDT: the width of the pair / incidence kernels (KD_MAX serves both narrow tiers).
template <int KD_, int BD_, int KDT_>
struct Tier {
  static constexpr int kd = KD_, bd = BD_, kdt = KDT_;
};
struct CovHandle;

struct Solver {
  const ba_options& opt;
  ba_problem& prob;
  Comm& comm;
  View V{};
  const std::chrono::steady_clock::time_point t_entry = std::chrono::steady_clock::now();  // setup_seconds counts from here
  Stream st;
  // topology
  Buf<int> o_sensor, sens_off;
  Buf<double> sensors, sensors2, Jsens;
  Buf<int> o_pose, o_cam, o_pt, pose_off, pose_dim, pose_fix, cam_off, cam_dim, cam_var, cam_model, pt_off,
      pt_ptr, blk_off, blk_dim, blk_kind, blk_moff, chunk_blk, chunk_beg, chunk_end, blk_chunk_ptr, blk_fin_end, heavy_blk, c2a, a2c, tile_pt;
  Buf<int4> tile_info;
  int n_heavy = 0;
  Buf<int> a_pose, a_cam, a_pt, a_sensor;  // p-order topology for the point-side linearisation pass
  Buf<double> a_xy;
  bool split_linearize = true;
  Buf<float> Jpose32, Jcam32, Jpt32;
  bool op32 = false;  // PCG operator streams the fp32 copies
  int plain_model = -1;  // >= 0: every camera has this model (SIMPLE_PINHOLE / PINHOLE / SIMPLE_RADIAL), no rig observations, trivial loss, no fp32 copies
  bool pcg_all_ranks_have_work = false;  // sharded solves: every rank has observations and chunk lists (agreed in run())
  Buf<unsigned char> solo;
  Buf<double> o_xy, poses, cams, points, poses2, cams2, points2, Jpose, Jcam, Jpt, res, res_p, scale_c, scale_p,
      scalars, gc, gp, diag_c, diag_p, Dc, Dp, Cinv, M, Minv, rhs, x, r, z, pdir, q, dp, jx, v, stepc, stepp, partials, cpart, Craw, tbuf, tmpc, Gobs, pcg_part, maxbuf;
  Buf<double> lin_sums;  // [g_c | diag_c | g_p | diag_p | E^T E]: one all-reduce per linearisation
  // image-sharded solves: (point, shared intrinsics block) incidences whose observations span ranks (ba_inc_* kernels)
  Buf<int> inc_pt, inc_blk, inc_ptr, inc_obs, inc_chunk_blk, inc_chunk_beg, inc_blk_chunk;
  Buf<double> inc_part;
  Buf<double> inc_wloc, inc_wtot;
  IncView IV{};
  IncView PV{};  // single GPU: (point, block) incidences with >= 2 observations in the block (ba_pair_cross_kernel)
  Buf<int> pv_pt, pv_blk, pv_ptr, pv_mem, pv_chunk_blk, pv_chunk_beg, pv_blk_chunk, pv_pair_blk;
  Buf<double> pv_part;
  int n_pair_blk = 0;
  // pipelined PCG (pcg_pipelined): partial sums, stop flag, Q history on the device; per-iteration scalars in pinned
  // host memory the device writes directly; events of two iterations in flight
  Buf<double> pcgp_part, pcgp_qhist;
  Buf<int> pcgp_stop;
  PcgHostSlot* pcgp_host = nullptr;      // [2], hipHostMalloc
  PcgHostSlot* pcgp_host_dev = nullptr;  // the same, as the device sees it
  Event pcgp_ev_dir[2], pcgp_ev_s0[2], pcgp_ev_s1[2];
  Buf<double> Sdense;  // exact tiers: the reduced camera system, n_c x n_c
  Buf<double> chol_linv, chol_tmp;  // blocked Cholesky workspace (ba_schur_explicit.h)
  Buf<int> chol_info;
  bool dense_by_products = false;   // legacy formation (n_c operator products): image-sharded solves only
  double factor_ms = 0.0;
  // position priors
  Buf<int> pr_pose, pr_sens, pr_po, pr_so, pr_pdim, pr_tb_blk, pr_tb_ptr, pr_tg_prior, pr_tg_base;
  Buf<double> pr_pos, pr_A, pr_r, pr_J, pr_jx;
  PriorView Q{};
  bool use_dense = false;
  bool use_priors() const { return Q.n > 0 && comm.rank == 0; }  // sums are all-reduced: one rank contributes them
  Buf<int> a_boff[3];
  Buf<double> Wp[3];
  int width_tier = TIER_NARROW;  // <KD, BD> of this problem, chosen in build()
  int kd = 4, bd = PD;           // its intrinsics tangent width / widest camera-side block
  // the host-built layout (ba_layout.h). After build() only its small maps are left: offsets and dimensions, blk_of_*,
  // blk_off / blk_moff, the priors' po / so; keep_obs_maps (set before build(): the step probe) keeps obs_of_a and a2c
  ba_layout::Layout lay;
  bool keep_obs_maps = false;
  Event ev0, ev1, ev2, ev3;
  Stream st_chol;  // second stream + events of the Cholesky lookahead (exact tiers)
  ba_explicit::PairLists pair_lists;  // pair-major formation of the exact tiers (built with the solve's other structures)
  Event ev_chol_panel, ev_chol_u2;

  Solver(ba_problem& p_, const ba_options& o_, Comm& c_) : opt(o_), prob(p_), comm(c_) {
    st.create();
    for (Event* e : {&ev0, &ev1, &ev2, &ev3}) e->create();
  }
  ~Solver() {
    if (pcgp_host) (void)hipHostFree(pcgp_host);
    ba_explicit::free_pair_lists(pair_lists);
  }
  bool points_local() const { return comm.world == 1 || comm.by_point; }  // a point's observations are all on this rank

  // f(Tier<...>{}) for the width tier of this problem: the one place that maps it to template instantiations
  template <typename F>
  void with_tier(F&& f) const {
    switch (width_tier) {
      case TIER_NARROW: f(Tier<4, PD, KD_MAX>{}); return;
      case TIER_MAX: f(Tier<KD_MAX, KD_MAX, KD_MAX>{}); return;
      case TIER_WIDE: f(Tier<KD_WIDE, KD_WIDE, KD_WIDE>{}); return;
    }
    throw std::runtime_error("unknown width tier " + std::to_string(width_tier));
  }

  // Before a finalize kernel: the heavy blocks' rows summed into their first row (ba_cpart_heavy_reduce_kernel).
  // `width` = the entries of a row the finalize kernel is going to read.
  void heavy_reduce(int width) {
    if (n_heavy <= 0) return;
    const int epw = width <= 16 ? 16 : 64;
    BA_LAUNCH(ba_cpart_heavy_reduce_kernel, dim3(n_heavy, (width + epw - 1) / epw), dim3(1024), st, V, width);
  }

  double scalar(int slot) {
    double v = 0.0;
    BA_HIP(hipMemcpyAsync(&v, scalars.p + slot, sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP(hipStreamSynchronize(st));
    return v;
  }
  // all scalar slots with ONE copy and ONE synchronisation (single-GPU solves read two results per sync point)
  void scalars_to_host(double* h) {
    BA_HIP(hipMemcpyAsync(h, scalars.p, sizeof(double) * NSCALAR, hipMemcpyDeviceToHost, st));
    BA_HIP(hipStreamSynchronize(st));
  }
  double scalar_sum(int slot) {  // value summed over ranks
    comm.allreduce(scalars.p + slot, 1, st);
    return scalar(slot);
  }
  // max over ranks of a non-negative scalar through the sum transport: every rank contributes its
  // value in its own slot of a zeroed world-sized vector. Only point sharding needs it (there a
  // rank sees the gradient of its own points only; with image sharding all vectors are replicated).
  double scalar_max(int slot) {
    if (comm.world == 1 || !comm.by_point) return scalar(slot);
    BA_HIP(hipMemsetAsync(maxbuf.p, 0, sizeof(double) * comm.world, st));
    BA_HIP(hipMemcpyAsync(maxbuf.p + comm.rank, scalars.p + slot, sizeof(double), hipMemcpyDeviceToDevice, st));
    comm.allreduce(maxbuf.p, comm.world, st);
    std::vector<double> h(comm.world);
    BA_HIP(hipMemcpyAsync(h.data(), maxbuf.p, sizeof(double) * comm.world, hipMemcpyDeviceToHost, st));
    BA_HIP(hipStreamSynchronize(st));
    return *std::max_element(h.begin(), h.end());
  }
  void zero_scalar(int slot) { BA_HIP(hipMemsetAsync(scalars.p + slot, 0, sizeof(double), st)); }

  // Reduced program: active observations (>= 1 variable block), tangent offsets, CSR structures -- the layout is
  // built on the host (ba_layout.h), then uploaded.
  int build(ba_result* res_out) {
    const ba_problem& p = prob;
    // COLMAP_AMD_BA_TIMING=1 (development switch): where the set-up time goes, to stderr
    const bool timing = dev_switch_int("COLMAP_AMD_BA_TIMING", 0) != 0;
    auto t_stage = std::chrono::steady_clock::now();
    auto stage = [&](const char* name) {
      if (!timing) return;
      const auto now = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[ba set-up] %-14s %8.2f ms\n", name, 1e3 * std::chrono::duration<double>(now - t_stage).count());
      t_stage = now;
    };
    ba_layout::LayoutParams lp;
    lp.rank = comm.rank; lp.world = comm.world; lp.by_point = comm.by_point;
    lp.chunk = chunk_size();
    lp.heavy_chunks = std::max(dev_switch_int("COLMAP_AMD_BA_HEAVY_CHUNKS", kHeavyChunks), 1);
    lp.tile_pts = TILE_PTS; lp.tile_obs = TILE_OBS;
    lp.inc_chunk = kIncChunk; lp.pair_chunk = kPairChunk;
    lp.pair_incidences = dev_switch_int("COLMAP_AMD_BA_PAIR_INCIDENCES", 1) != 0;
    lp.stage = stage;
    lay = ba_layout::make_layout(p, lp);
    // <KD, BD> of this problem (see the constants at the top of the file)
    width_tier = ba_layout::pick_tier(lay);
    with_tier([&](auto t) { kd = t.kd; bd = t.bd; });
    split_linearize = dev_switch_int("COLMAP_AMD_BA_SPLIT_LINEARIZE", 1) != 0;  // read per solve: tests toggle it
    res_out->num_residuals = (int32_t)(2 * lay.n_active_global) + 3 * lay.n_priors();
    res_out->num_effective_parameters = lay.n_c + lay.n_p;
    if (lay.n_var_sensors > 0 && comm.world > 1)
      throw std::runtime_error("refine_sensor_from_rig is not supported by the sharded solve");
    if (lay.n_active_global == 0) return 0;
    if (lay.n == 0)
      throw std::runtime_error("rank " + std::to_string(comm.rank) + " holds no observation: use fewer ranks "
                               "than images");
    upload_layout();
    allocate_work_buffers();
    const int64_t n_active_global = lay.n_active_global;
    lay.release_observation_arrays(keep_obs_maps);  // (a 20 M-observation solve does not hold them through the LM loop)
    stage("upload+alloc");
    // uploads / memsets above ran on the NULL stream, the solve runs on a non-blocking stream
    BA_HIP(hipDeviceSynchronize());
    return (int)std::min<int64_t>(n_active_global, 1 << 30);
  }

  // The layout's arrays to the device, every view field beside its upload
  void upload_layout() {
    const ba_problem& p = prob;
    const ba_layout::Layout& L = lay;
    const bool has_sensors = L.has_sensors;
    V.n_obs = L.n; V.n_poses = p.num_poses; V.n_cams = p.num_cams; V.n_points = p.num_points;
    V.n_c = L.n_c; V.n_p = L.n_p; V.n_blk = L.n_blk(); V.n_chunks = (int)L.chunk_blk.size();
    V.kd = kd;
    V.bd = bd;
    V.o_pose = o_pose.upload(L.o_pose); V.o_cam = o_cam.upload(L.o_cam); V.o_pt = o_pt.upload(L.o_pt);
    V.o_xy = o_xy.upload(L.o_xy);
    V.o_sensor = nullptr; V.sensors = nullptr; V.sens_off = nullptr;
    V.n_sensors = has_sensors ? p.num_sensors : 0;
    if (has_sensors) {
      V.o_sensor = o_sensor.upload(L.o_sensor);
      V.sensors = sensors.upload(std::vector<double>(p.sensors, p.sensors + (size_t)7 * p.num_sensors));
      sensors2.alloc(sensors.n);
      BA_HIP(hipMemcpy(sensors2.p, sensors.p, sizeof(double) * sensors.n, hipMemcpyDeviceToDevice));
      if (L.n_var_sensors > 0) V.sens_off = sens_off.upload(L.sens_off);
    }
    V.pose_off = pose_off.upload(L.pose_off); V.pose_dim = pose_dim.upload(L.pose_dim); V.pose_fix = pose_fix.upload(L.pose_fix);
    V.cam_off = cam_off.upload(L.cam_off); V.cam_dim = cam_dim.upload(L.cam_dim);
    {
      std::vector<int> h_cam_var((size_t)p.num_cams * kd, 0);  // the tier's row stride
      for (int k = 0; k < p.num_cams; ++k)
        for (int d = 0; d < L.cam_nvar[k]; ++d) h_cam_var[(size_t)k * kd + d] = L.cam_var[(size_t)k * BA_CAM_STRIDE + d];
      V.cam_var = cam_var.upload(h_cam_var);
    }
    V.cam_model = cam_model.upload(std::vector<int>(p.cam_model, p.cam_model + p.num_cams));
    V.pt_off = pt_off.upload(L.pt_off); V.pt_ptr = pt_ptr.upload(L.pt_ptr);
    V.blk_off = blk_off.upload(L.blk_off); V.blk_dim = blk_dim.upload(L.blk_dim);
    V.blk_kind = blk_kind.upload(L.blk_kind); V.blk_moff = blk_moff.upload(L.blk_moff);
    // position priors (ba_prior_* kernels)
    Q = PriorView{};
    Q.n = L.n_priors();
    if (Q.n > 0) {
      Q.pose = pr_pose.upload(L.pr_pose); Q.sens = pr_sens.upload(L.pr_sens);
      Q.po = pr_po.upload(L.pr_po); Q.so = pr_so.upload(L.pr_so); Q.pdim = pr_pdim.upload(L.pr_pdim);
      Q.pos = pr_pos.upload(L.pr_pos); Q.A = pr_A.upload(L.pr_A);
      Q.n_tblk = (int)L.tb_blk.size();
      Q.tb_blk = pr_tb_blk.upload(L.tb_blk); Q.tb_ptr = pr_tb_ptr.upload(L.tb_ptr);
      Q.tg_prior = pr_tg_prior.upload(L.tg_prior); Q.tg_base = pr_tg_base.upload(L.tg_base);
      Q.loss_type = p.prior_loss_type; Q.loss_scale = p.prior_loss_scale;
    }
    // image sharding: the incidences that span ranks (ba_inc_* kernels)
    IV = IncView{};
    if (L.inc.n() > 0) {
      IV.n = L.inc.n();
      IV.pt = inc_pt.upload(L.inc.pt); IV.blk = inc_blk.upload(L.inc.blk);
      IV.ptr = inc_ptr.upload(L.inc.ptr); IV.obs = inc_obs.upload(L.inc.obs);
      IV.n_chunks = (int)L.inc.chunk_blk.size();
      IV.chunk_blk = inc_chunk_blk.upload(L.inc.chunk_blk); IV.chunk_beg = inc_chunk_beg.upload(L.inc.chunk_beg);
      IV.blk_chunk = inc_blk_chunk.upload(L.inc.blk_chunk);
    }
    // pairs of observations of one point inside one block: p-order block offsets per kind (ba_obs_w_kernel /
    // ba_block_schur_cross_kernel), only for the kinds that have such pairs
    for (int kind = 0; kind < 3; ++kind) {
      V.wdim[kind] = kind == 1 ? kd : 6;
      V.a_boff[kind] = L.n_paired_kind[kind] > 0 ? a_boff[kind].upload(L.a_boff[kind]) : nullptr;
    }
    // single GPU: the pair incidences themselves (ba_pair_cross_kernel)
    PV = IncView{};
    n_pair_blk = 0;
    if (L.pairs.n() > 0) {
      PV.n = L.pairs.n();
      PV.pt = pv_pt.upload(L.pairs.pt); PV.blk = pv_blk.upload(L.pairs.blk);
      PV.ptr = pv_ptr.upload(L.pairs.ptr); PV.obs = pv_mem.upload(L.pairs.obs);
      PV.n_chunks = (int)L.pairs.chunk_blk.size();
      PV.chunk_blk = pv_chunk_blk.upload(L.pairs.chunk_blk); PV.chunk_beg = pv_chunk_beg.upload(L.pairs.chunk_beg);
      PV.blk_chunk = pv_blk_chunk.upload(L.pairs.blk_chunk);
      pv_pair_blk.upload(L.pairs.blocks);
      n_pair_blk = (int)L.pairs.blocks.size();
    }
    V.chunk_blk = chunk_blk.upload(L.chunk_blk); V.chunk_beg = chunk_beg.upload(L.chunk_beg);
    V.chunk_end = chunk_end.upload(L.chunk_end);
    V.c2a = c2a.upload(L.c2a); V.a2c = a2c.upload(L.a2c); V.solo = solo.upload(L.solo);
    V.tile_pt = tile_pt.upload(L.tile_pt);
    V.n_tiles = (int)L.tile_pt.size() - 1;
    {
      std::vector<int4> h_tile_info(std::max<size_t>(L.tile_pt.size(), 2) - 1, make_int4(0, 0, 0, 0));
      for (size_t t = 0; t + 1 < L.tile_pt.size(); ++t) {
        const int q0 = L.tile_pt[t], q1 = L.tile_pt[t + 1];
        h_tile_info[t] = make_int4(q0, q1, L.pt_ptr[q0], L.pt_ptr[q1] - L.pt_ptr[q0]);
      }
      V.tile_info = tile_info.upload(h_tile_info);
    }
    // (the explicit Schur formation reads the p-order topology too, whatever the linearisation does)
    V.a_pose = a_pose.upload(L.a_pose); V.a_cam = a_cam.upload(L.a_cam); V.a_pt = a_pt.upload(L.a_pt);
    V.a_xy = a_xy.upload(L.a_xy);
    V.a_sensor = has_sensors ? a_sensor.upload(L.a_sensor) : nullptr;
    V.blk_chunk_ptr = blk_chunk_ptr.upload(L.blk_chunk_ptr);
    V.blk_fin_end = blk_fin_end.upload(L.blk_fin_end);
    V.n_heavy = n_heavy = (int)L.heavy.size();
    V.heavy_blk = heavy_blk.upload(L.heavy.empty() ? std::vector<int>(1, 0) : L.heavy);
    V.poses = poses.upload(std::vector<double>(p.poses, p.poses + 7 * (size_t)p.num_poses));
    V.cams = cams.upload(std::vector<double>(p.cams, p.cams + BA_CAM_STRIDE * (size_t)p.num_cams));
    V.points = points.upload(std::vector<double>(p.points, p.points + 3 * (size_t)p.num_points));
  }

  // Everything the solve writes: Jacobian planes, per-chunk partials, the vectors of the LM / PCG loops
  void allocate_work_buffers() {
    const ba_problem& p = prob;
    const ba_layout::Layout& L = lay;
    const int n = L.n, n_c = L.n_c, poff = L.n_p, n_blk = L.n_blk();
    const size_t N = (size_t)n;
    if (Q.n > 0) {
      pr_r.alloc(3 * (size_t)Q.n); pr_J.alloc(36 * (size_t)Q.n); pr_jx.alloc(3 * (size_t)Q.n);
      Q.r = pr_r.p; Q.J = pr_J.p; Q.jx = pr_jx.p;
    }
    if (IV.n > 0) {
      inc_part.alloc((size_t)IV.n_chunks * KD_WIDE * KD_WIDE);
      IV.part = inc_part.p;
      inc_wloc.alloc((size_t)IV.n * KD_WIDE * 3); inc_wtot.alloc((size_t)IV.n * KD_WIDE * 3);
    }
    for (int kind = 0; kind < 3; ++kind) {  // room for the W's of the kinds with pairs
      V.Wp[kind] = nullptr;
      if (L.n_paired_kind[kind] <= 0) continue;
      Wp[kind].alloc(N * V.wdim[kind] * 3);
      V.Wp[kind] = Wp[kind].p;
    }
    if (PV.n > 0) {
      pv_part.alloc((size_t)PV.n_chunks * KD_WIDE * KD_WIDE);
      PV.part = pv_part.p;
    }
    cpart.alloc((size_t)V.n_chunks * bd * bd);
    poses2.alloc(poses.n); cams2.alloc(cams.n); points2.alloc(points.n);
    Jpose.alloc(2 * PD * N); Jcam.alloc(2 * (size_t)kd * N); Jpt.alloc(6 * N); res.alloc(2 * N); res_p.alloc(2 * N);
    jx.alloc(2 * N); v.alloc(2 * N); Gobs.alloc(4 * N);
    if (L.n_var_sensors > 0) Jsens.alloc(12 * N);
    V.Jsens = L.n_var_sensors > 0 ? Jsens.p : nullptr;
    {
      op32 = opt.operator_precision == BA_OPERATOR_F32 && L.n_var_sensors == 0 && V.n_tiles > 0 && comm.world == 1;
      if (op32) { Jpose32.alloc(2 * PD * N); Jcam32.alloc(2 * (size_t)kd * N); Jpt32.alloc(6 * N); }
      V.Jpose32 = op32 ? Jpose32.p : nullptr;
      V.Jcam32 = op32 ? Jcam32.p : nullptr;
      V.Jpt32 = op32 ? Jpt32.p : nullptr;
    }
    {
      plain_model = -1;
      const bool plain_ok = dev_switch_int("COLMAP_AMD_BA_PLAIN_LINEARIZE", 1) != 0 && !op32 && !L.has_sensors &&
                            opt.loss_type == BA_LOSS_TRIVIAL && p.num_cams > 0;
      if (plain_ok) {
        const int m0 = p.cam_model[0];
        bool same = m0 == BA_SIMPLE_PINHOLE || m0 == BA_PINHOLE || m0 == BA_SIMPLE_RADIAL;
        for (int k = 1; same && k < p.num_cams; ++k) same = p.cam_model[k] == m0;
        if (same) plain_model = m0;
      }
    }
    // gradient, column norms and E^T E of a linearisation are summed over the ranks of a sharded solve in ONE
    // all-reduce: they live back to back in `lin_sums` [g_c | diag_c | g_p | diag_p | E^T E] (point sharding
    // reduces the camera-side prefix only)
    lin_sums.alloc(2 * (size_t)n_c + 2 * (size_t)poff + 6 * (size_t)p.num_points);
    gc.alias(lin_sums.p, n_c); diag_c.alias(lin_sums.p + n_c, n_c);
    gp.alias(lin_sums.p + 2 * (size_t)n_c, poff); diag_p.alias(lin_sums.p + 2 * (size_t)n_c + poff, poff);
    Craw.alias(lin_sums.p + 2 * (size_t)n_c + 2 * (size_t)poff, 6 * (size_t)p.num_points);
    scale_c.alloc(n_c); scale_p.alloc(poff);
    Dc.alloc(n_c); Dp.alloc(poff); rhs.alloc(n_c); x.alloc(n_c); r.alloc(n_c); z.alloc(n_c); pdir.alloc(n_c);
    q.alloc(n_c); dp.alloc(poff); stepc.alloc(n_c); stepp.alloc(poff);
    Cinv.alloc(9 * (size_t)p.num_points); M.alloc(L.moff_total); Minv.alloc(L.moff_total);
    tbuf.alloc(poff); tmpc.alloc(n_c);
    scalars.alloc(NSCALAR);
    pcg_part.alloc((size_t)grid_for(n_blk, 256) + 1);
    partials.alloc((size_t)std::max(grid_for(n, 256), std::max(p.num_points, 1)) + 1);  // one slot per linearise workgroup / point tile
    if (opt.loss_type < BA_LOSS_TRIVIAL || opt.loss_type > BA_LOSS_HUBER)
      throw std::runtime_error("unknown loss_type " + std::to_string(opt.loss_type));
    if (opt.loss_type != BA_LOSS_TRIVIAL && !(opt.loss_scale > 0.0))
      throw std::runtime_error("loss_scale must be positive");
    V.loss_type = opt.loss_type;
    V.loss_scale = opt.loss_scale;
    V.cpart = cpart.p;
    V.Jpose = Jpose.p; V.Jcam = Jcam.p; V.Jpt = Jpt.p; V.res = res.p; V.res_p = res_p.p;
    V.scale_c = scale_c.p; V.scale_p = scale_p.p; V.scalars = scalars.p;
    maxbuf.alloc(std::max(comm.world, 1));
  }

  void launch_linearize(bool jac, const double* P, const double* Cm, const double* X, const double* Sn, int slot) {
    const int g = grid_for(V.n_obs, 256);
    if (split_linearize && width_tier == TIER_NARROW && plain_model >= 0) {
      // one camera model, no rig observations, trivial loss, no fp32 copies: the PLAIN instantiations (same bits)
      auto launch = [&](auto tag) {
        constexpr int M = decltype(tag)::value;
        if (jac) {
          BA_LAUNCH((ba_linearize_kernel<true, 4, false, M>), dim3(g), dim3(256), st, V, P, Cm, X, Sn, partials.p);
          // (the point side stays generic: its PLAIN instantiation -- 48 registers, eight waves per SIMD -- measured
          //  88 us against 79 at BA-1; same bits either way)
          BA_LAUNCH((ba_linearize_point_kernel<4>), dim3(g), dim3(256), st, V, P, Cm, X, Sn);
        } else {
          BA_LAUNCH((ba_linearize_kernel<false, 4, true, M>), dim3(g), dim3(256), st, V, P, Cm, X, Sn, partials.p);
        }
      };
      if (plain_model == BA_SIMPLE_PINHOLE) launch(std::integral_constant<int, BA_SIMPLE_PINHOLE>{});
      else if (plain_model == BA_PINHOLE) launch(std::integral_constant<int, BA_PINHOLE>{});
      else launch(std::integral_constant<int, BA_SIMPLE_RADIAL>{});
    } else {
      with_tier([&](auto t) {
        if (jac && split_linearize) {  // camera side in c-order, point side in p-order: every store coalesced
          BA_LAUNCH((ba_linearize_kernel<true, t.kd, false>), dim3(g), dim3(256), st, V, P, Cm, X, Sn, partials.p);
          BA_LAUNCH((ba_linearize_point_kernel<t.kd>), dim3(g), dim3(256), st, V, P, Cm, X, Sn);
        } else if (jac) {
          BA_LAUNCH((ba_linearize_kernel<true, t.kd>), dim3(g), dim3(256), st, V, P, Cm, X, Sn, partials.p);
        } else {
          BA_LAUNCH((ba_linearize_kernel<false, t.kd>), dim3(g), dim3(256), st, V, P, Cm, X, Sn, partials.p);
        }
      });
    }
    BA_LAUNCH(ba_final_sum_kernel, dim3(1), dim3(1024), st, partials.p, g, scalars.p + slot);
    if (use_priors()) {
      if (jac) BA_LAUNCH(ba_prior_linearize_kernel<true>, dim3(1), dim3(256), st, V, Q, P, Sn, scalars.p + slot);
      else BA_LAUNCH(ba_prior_linearize_kernel<false>, dim3(1), dim3(256), st, V, Q, P, Sn, scalars.p + slot);
    }
  }

  // gradient of the (scaled) Jacobian and its squared column norms
  void gradient_and_diag() {
    if (V.n_chunks == 0) {
      BA_HIP(hipMemsetAsync(gc.p, 0, sizeof(double) * std::max(V.n_c, 1), st));
      BA_HIP(hipMemsetAsync(diag_c.p, 0, sizeof(double) * std::max(V.n_c, 1), st));
    } else {
      with_tier([&](auto t) {
        BA_LAUNCH((ba_block_jtv_kernel<true, t.bd>), dim3(V.n_chunks), dim3(64), st, V, res.p, gc.p, diag_c.p);
      });
      heavy_reduce(2 * bd);
      BA_LAUNCH(ba_block_vec_finalize_kernel<true>, dim3(grid_for(V.n_blk * bd, 128)), dim3(128), st, V, gc.p, diag_c.p);
    }
    // (g_p and the point column norms are written for every variable point by either kernel)
    if (V.n_tiles > 0)
      BA_LAUNCH(ba_point_reduce_tiled_kernel<0>, dim3(V.n_tiles), dim3(TILE_PTS), st, V, nullptr, nullptr, gp.p, diag_p.p, Craw.p);
    else {
      BA_LAUNCH(ba_point_grad_kernel, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, gp.p, diag_p.p);
      BA_LAUNCH(ba_point_gram_kernel, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, Craw.p);
    }
    if (use_priors())
      BA_LAUNCH(ba_prior_accumulate_kernel<0>, dim3(grid_for(Q.n_tblk, 64)), dim3(64), st, V, Q, gc.p, diag_c.p);
    // one all-reduce for everything a linearisation sums over ranks (E^T E of the points changes only here).
    // Point sharding: a point's gradient, column norms and E^T E are complete locally -> camera-side prefix only.
    if (comm.by_point) comm.allreduce(lin_sums.p, 2 * (size_t)V.n_c, st);
    else comm.allreduce(lin_sums.p, lin_sums.n, st);
  }

  // y = (sum over ranks of J_c^T v) for this rank's observations, into tmpc
  void block_jtv_reduced(const double* vin, const double* x_for_priors = nullptr) {
    if (V.n_chunks == 0) BA_HIP(hipMemsetAsync(tmpc.p, 0, sizeof(double) * std::max(V.n_c, 1), st));
    if (V.n_chunks > 0) {
      chunk_jtv(vin);
      heavy_reduce(bd);
      BA_LAUNCH(ba_block_vec_finalize_kernel<false>, dim3(grid_for(V.n_blk * bd, 128)), dim3(128), st, V, tmpc.p, nullptr);
    }
    if (x_for_priors && use_priors()) {  // + sum over priors J^T (J x)
      BA_LAUNCH(ba_prior_jx_kernel, dim3(grid_for(Q.n, 64)), dim3(64), st, Q, x_for_priors);
      BA_LAUNCH(ba_prior_accumulate_kernel<2>, dim3(grid_for(Q.n_tblk, 64)), dim3(64), st, V, Q, tmpc.p, nullptr);
    }
    comm.allreduce(tmpc.p, V.n_c, st);
  }

  template <int MODE>
  void point_pass() {
    if (V.n_tiles > 0)
      BA_LAUNCH(ba_point_pass_tiled_kernel<MODE>, dim3(V.n_tiles), dim3(TILE_PTS), st, V, Cinv.p, jx.p, gp.p, v.p, dp.p);
    else
      BA_LAUNCH(ba_point_pass_kernel<MODE>, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, Cinv.p, jx.p, gp.p,
                v.p, dp.p);
  }

  // q = S x = (B + Dc^2) x - E C^-1 E^T x
  // `inexact`: called by the CG iteration (may stream the fp32 operator copies); the exact formation by
  // operator products passes false.
  void schur_multiply(const double* xin, double* qout, bool inexact = false) {
    if (comm.world == 1 && !use_priors() && V.n_chunks > 0 && V.n_obs > 0) {
      // single GPU, no priors: nothing sits between J_c^T v and the block sums -> one tail kernel
      schur_streams(xin, inexact && op32);
      heavy_reduce(bd);
      BA_LAUNCH(ba_block_vec_finalize_q_kernel, dim3(grid_for(V.n_blk * bd, 128)), dim3(128), st, V, Dc.p, xin, qout);
      return;
    }
    if (V.n_obs > 0) obs_jx(xin);
    if (points_local()) {
      point_pass<0>();
    } else {
      BA_HIP(hipMemsetAsync(tbuf.p, 0, sizeof(double) * std::max(V.n_p, 1), st));
      BA_LAUNCH(ba_point_t_kernel, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, jx.p, tbuf.p);
      comm.allreduce(tbuf.p, V.n_p, st);
      BA_LAUNCH(ba_point_apply_kernel<0>, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, Cinv.p, jx.p, gp.p,
                tbuf.p, v.p, dp.p);
    }
    block_jtv_reduced(v.p, xin);
    BA_LAUNCH(ba_dsq_x_kernel, dim3(grid_for(V.n_c, 256)), dim3(256), st, V.n_c, Dc.p, xin, qout);
    BA_LAUNCH(ba_add_kernel, dim3(grid_for(V.n_c, 256)), dim3(256), st, V.n_c, tmpc.p, qout);
  }

  // what the explicit formation of the exact tiers reads (ba_schur_explicit.h)
  ba_explicit::FormArgs form_args() {
    ba_explicit::FormArgs fa{};
    fa.n_obs = V.n_obs; fa.n_points = V.n_points; fa.n_c = V.n_c; fa.kd = kd;
    fa.Jpose = V.Jpose; fa.Jcam = V.Jcam; fa.Jsens = V.sens_off ? V.Jsens : nullptr; fa.Jpt = V.Jpt;
    fa.Cinv = Cinv.p; fa.a2c = V.a2c; fa.pt_ptr = V.pt_ptr; fa.pt_off = V.pt_off;
    fa.a_pose = V.a_pose; fa.a_cam = V.a_cam; fa.a_sensor = V.sens_off ? V.a_sensor : nullptr;
    fa.a_pt = V.a_pt; fa.n_poses = V.n_poses;
    fa.pose_off = V.pose_off; fa.pose_dim = V.pose_dim; fa.cam_off = V.cam_off; fa.cam_dim = V.cam_dim;
    fa.sens_off = V.sens_off;
    fa.fixed_point = opt.jacobi_scaling != 0;  // columns of norm < 1: integer accumulation, bit-reproducible
    fa.bad = chol_info.p + 1;                  // raised by a term the fixed point cannot hold (NaN, out of bound)
    return fa;  // (pairs: form_reduced_system)
  }

  // Exact tiers: the reduced system of n columns (+ the row of the right-hand side, ba_explicit::factor_solve) and the
  // Cholesky workspace. (The memsets run on the NULL stream: the caller synchronises the device before the first use.)
  void prepare_exact(int n) {
    Sdense.alloc((size_t)n * n + n);
    if (dense_by_products) return;
    chol_linv.alloc(ba_explicit::Workspace{}.linv_doubles(n)); chol_tmp.alloc(n); chol_info.alloc(2);  // [pivot flag, formation flag]
  }
  // Cholesky lookahead (unless COLMAP_AMD_BA_CHOL_LOOKAHEAD=0): the second stream carries bulk trailing updates that run
  // beside the serial chain of small kernels on the main stream: lowest priority, so that a freed workgroup slot goes to
  // the chain first. (The covariance path opens it after its one formation: 5 us of 90 with the second queue open.)
  void open_cholesky_lookahead() {
    if (dev_switch_int("COLMAP_AMD_BA_CHOL_LOOKAHEAD", 1) == 0) return;
    st_chol.create_lowest_priority(); ev_chol_panel.create(false); ev_chol_u2.create(false);
  }
  auto cholesky_workspace() const {  // (no lookahead: its stream and events are null, which is how factor_solve is told)
    ba_explicit::Workspace ws;
    ws.Linv = chol_linv.p; ws.tmp = chol_tmp.p; ws.info = chol_info.p;
    ws.st2 = st_chol; ws.ev_panel = ev_chol_panel; ws.ev_u2 = ev_chol_u2;
    return ws;
  }
  // Pair-major formation: its incidence lists depend on the topology in `fa` only -- built once, with the other
  // per-solve structures, not inside the LM loop (COLMAP_AMD_BA_FORM_PAIRS=0: the point-major kernel)
  void build_pair_lists(const ba_explicit::FormArgs& fa) {
    if (dev_switch_int("COLMAP_AMD_BA_FORM_PAIRS", 1) != 0) (void)ba_explicit::build_pair_lists(fa, pair_lists, st);
  }
  // Sdense = this rank's reduced camera system in the layout of `fa` (pair-major when the lists were built, else one
  // wave per point), with the priors' rows at the given tangent offsets
  void form_reduced_system(ba_explicit::FormArgs fa, const int* prior_pose_off, const int* prior_sens_off) {
    fa.pairs = pair_lists.inc ? &pair_lists : nullptr;
    ba_explicit::form(fa, Sdense.p, st);
    if (use_priors())
      ba_explicit::add_prior_rows(Sdense.p, fa.n_c, Q.J, prior_pose_off, prior_sens_off, Q.pdim, Q.n, fa.fixed_point, fa.bad, st);
    ba_explicit::finish(Sdense.p, fa.n_c, fa.fixed_point, fa.bad, st);
  }

  // DENSE_SCHUR: x = S^-1 rhs with S built from n_c operator products
  int dense_schur() {
    const int n = V.n_c;
    if (Sdense.n < (size_t)n * n + n) throw std::runtime_error("dense Schur buffer");
    if (!dense_by_products) {
      // explicit formation + blocked Cholesky on the f64 matrix cores
      form_reduced_system(form_args(), Q.po, Q.so);
      if (comm.world > 1) comm.allreduce(Sdense.p, (size_t)n * n, st);  // point sharding: partial sums per rank
      ba_explicit::add_lm_diagonal(Sdense.p, n, Dc.p, st);
      double ms = 0.0;
      ba_explicit::factor_solve(Sdense.p, n, rhs.p, x.p, cholesky_workspace(), st, ev0, ev1, &ms);
      factor_ms += ms;
      return 1;
    }
    for (int i = 0; i < n; ++i) {
      BA_LAUNCH(ba_unit_vector_kernel, dim3(grid_for(n, 256)), dim3(256), st, n, i, pdir.p);
      schur_multiply(pdir.p, Sdense.p + (size_t)i * n);
    }
    BA_LAUNCH(ba_dense_cholesky_solve_kernel, dim3(1), dim3(1024), st, n, Sdense.p, rhs.p, x.p);
    return 1;
  }

  // jx = J_c x (c-order pairs), one lane per observation
  template <typename JT = double>
  void obs_jx(const double* xin) {
    with_tier([&](auto t) {
      BA_LAUNCH((ba_obs_jx_kernel<t.kd, JT>), dim3(grid_for(V.n_obs, 256)), dim3(256), st, V, xin, jx.p);
    });
  }

  // J_c^T v of every chunk into its partials (the block sums are left to a finalize kernel), v in c-order pairs
  template <typename JT = double>
  void chunk_jtv(const double* vin) {
    with_tier([&](auto t) {
      BA_LAUNCH((ba_block_jtv_kernel<false, t.bd, JT>), dim3(V.n_chunks), dim3(64), st, V, vin, tmpc.p, nullptr);
    });
  }

  // The three streaming kernels of one implicit product on a single GPU: J_c p (c-order -> p-order),
  // the point pass, J_c^T v into per-chunk partials. The caller finishes the product from the partials.
  void schur_streams(const double* xin, bool use32) {
    if (use32) {  // the inexact inner solve streams the fp32 copies of the columns (fp64 accumulation)
      obs_jx<float>(xin);
      BA_LAUNCH((ba_point_pass_tiled_kernel<0, float>), dim3(V.n_tiles), dim3(TILE_PTS), st, V, Cinv.p, jx.p, gp.p, v.p, dp.p);
      chunk_jtv<float>(v.p);
      return;
    }
    obs_jx(xin);
    point_pass<0>();
    chunk_jtv(v.p);
  }

  int pcg_pipelined(int max_iter, double q_tol) {
    const int n = V.n_c, gv = std::max(grid_for(n, 256), 1), nparts = grid_for(V.n_blk, PCGP_T);
    if (!pcgp_host) {
      BA_HIP(hipHostMalloc((void**)&pcgp_host, 2 * sizeof(PcgHostSlot), hipHostMallocMapped));
      BA_HIP(hipHostGetDevicePointer((void**)&pcgp_host_dev, pcgp_host, 0));
      pcgp_part.alloc((size_t)2 * 3 * nparts);
      pcgp_qhist.alloc(2);
      pcgp_stop.alloc(1);
      for (Event& e : pcgp_ev_dir) e.create(false);
      for (Event* e : {&pcgp_ev_s0[0], &pcgp_ev_s0[1], &pcgp_ev_s1[0], &pcgp_ev_s1[1]}) e->create();
    }
    PcgDev D;
    D.part = pcgp_part.p; D.nparts = nparts; D.stop = pcgp_stop.p; D.host = pcgp_host_dev; D.qhist = pcgp_qhist.p;
    with_tier([&](auto t) {
      BA_LAUNCH(ba_pcgp_init_kernel<t.bd>, dim3(nparts), dim3(PCGP_T), st, V, D, Minv.p, rhs.p, x.p, r.p, z.p);
    });
    V.stop = pcgp_stop.p;  // the streaming kernels of an iteration enqueued past convergence return at entry
    auto enqueue = [&](int k) {
      BA_LAUNCH(ba_pcgp_dir_kernel, dim3(gv), dim3(256), st, n, D, k, max_iter, q_tol, z.p, pdir.p);
      BA_HIP(hipEventRecord(pcgp_ev_dir[k & 1], st));
      BA_HIP(hipEventRecord(pcgp_ev_s0[k & 1], st));
      schur_streams(pdir.p, op32);
      BA_HIP(hipEventRecord(pcgp_ev_s1[k & 1], st));
      heavy_reduce(bd);
      const double* reduced = nullptr;
      if (comm.world > 1) {
        // point sharding: every rank holds J_c^T v of its own observations -- block sums, then ONE all-reduce of the
        // camera-space vector (n_c doubles: 64 KB at BA-1) on the solver's stream. With the RCCL transport nothing
        // here touches the host: the iteration stays enqueued one ahead, the stop flag is computed identically on
        // every rank from the identical reduced vector (an iteration enqueued past convergence still runs its
        // all-reduce on every rank, on stale data nobody reads).
        BA_LAUNCH(ba_block_vec_finalize_kernel<false>, dim3(grid_for(V.n_blk * bd, 128)), dim3(128), st, V, tmpc.p, nullptr);
        comm.allreduce(tmpc.p, (size_t)n, st);
        reduced = tmpc.p;
      }
      with_tier([&](auto t) {
        BA_LAUNCH(ba_pcgp_tail_kernel<t.bd>, dim3(nparts), dim3(PCGP_T), st, V, D, k, Dc.p, pdir.p, q.p, reduced);
        BA_LAUNCH(ba_pcgp_step_kernel<t.bd>, dim3(nparts), dim3(PCGP_T), st, V, D, k, Minv.p, rhs.p, pdir.p, q.p, x.p, r.p, z.p);
      });
    };
    enqueue(1);
    BA_HIP(hipEventSynchronize(pcgp_ev_dir[1]));
    int done = 0;
    if (!pcgp_host[0].stop) {  // (zero right-hand side otherwise)
      for (int k = 1;; ++k) {
        enqueue(k + 1);                                   // its dir kernel closes iteration k
        BA_HIP(hipEventSynchronize(pcgp_ev_dir[(k + 1) & 1]));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pcgp_ev_s0[k & 1], pcgp_ev_s1[k & 1]) == hipSuccess) { g_spmv_ms += ms; g_spmv_launches += 1; }
        const PcgHostSlot h = pcgp_host[k & 1];
        if (h.iter != k) throw std::runtime_error("pipelined PCG: host slot out of step");
        if (h.stop) { done = std::min(k, max_iter); break; }
      }
    }
    V.stop = nullptr;
    return done;
  }

  int pcg(int max_iter, double q_tol) {
    // single GPU, no priors: three small kernels per iteration, stopping test on the device, host one iteration
    // behind -- and point-sharded solves whose ranks all hold observations (pcg_all_ranks_have_work: agreed once per
    // solve, the ranks must take the same path). Prior solves and image-sharded ones (which all-reduce inside the
    // point pass as well) take the step-by-step loop below.
    const bool local_ok = !use_priors() && V.n_chunks > 0 && V.n_obs > 0;
    if (local_ok && points_local() && (comm.world == 1 || pcg_all_ranks_have_work)) {
      ++g_pcg_pipelined_solves;
      return pcg_pipelined(max_iter, q_tol);
    }
    ++g_pcg_stepwise_solves;
    const int n = V.n_c;
    const int gv = grid_for(n, 256);
    BA_HIP(hipMemsetAsync(x.p, 0, sizeof(double) * n, st));
    BA_HIP(hipMemcpyAsync(r.p, rhs.p, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    BA_LAUNCH(ba_dot_kernel, dim3(1), dim3(1024), st, n, rhs.p, rhs.p, scalars.p + S_RHO);
    if (scalar(S_RHO) == 0.0) return 0;
    double Q0 = 0.0;
    int it;
    const int nparts = grid_for(V.n_blk, 256);
    for (it = 1; it <= max_iter; ++it) {
      BA_LAUNCH(ba_pcg_precond_kernel, dim3(nparts), dim3(256), st, V, Minv.p, r.p, z.p, pcg_part.p);
      BA_LAUNCH(ba_pcg_dir_kernel, dim3(gv), dim3(256), st, n, scalars.p, pcg_part.p, nparts, it == 1 ? 1 : 0, z.p, pdir.p);
      BA_HIP(hipEventRecord(ev0, st));
      schur_multiply(pdir.p, q.p, true);
      BA_HIP(hipEventRecord(ev1, st));
      BA_LAUNCH(ba_pcg_update_kernel, dim3(1), dim3(1024), st, n, scalars.p, pcg_part.p, nparts, pdir.p, q.p, rhs.p, x.p, r.p);
      double h[NSCALAR];
      BA_HIP(hipMemcpyAsync(h, scalars.p, sizeof(h), hipMemcpyDeviceToHost, st));
      BA_HIP(hipStreamSynchronize(st));
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) { g_spmv_ms += ms; g_spmv_launches += 1; }
      const double rho = h[S_RHO], pq = h[S_PQ], Q1 = h[S_Q];
      if (!(rho > 0.0) || !std::isfinite(rho) || !(pq > 0.0) || !std::isfinite(pq)) break;
      const double zeta = it * (Q1 - Q0) / Q1;
      if (zeta < q_tol) break;
      Q0 = Q1;
    }
    return std::min(it, max_iter);
  }

  // Plus() of every parameter block in one launch; `tf` says how the step is read (StepSrc), `maxdiff` adds
  // max |x_plus - x| into scalars[S_GMAX]
  void apply_step(const double* sc, const double* sc_scale, const double* sp, const double* sp_scale, int tf, bool maxdiff,
                  double* P2, double* C2, double* X2) {
    const int nb = grid_for(V.n_points, 128) + grid_for(V.n_poses, 128) + grid_for(V.n_cams, 128) +
                   (V.sens_off ? grid_for(V.n_sensors, 128) : 0);
    const StepSrc Sc{sc, sc_scale, tf}, Sp{sp, sp_scale, tf};
    if (maxdiff)
      BA_LAUNCH(ba_apply_all_kernel<true>, dim3(std::max(nb, 1)), dim3(128), st, V, Sc, Sp, poses.p, P2, cams.p, C2, points.p, X2,
                sensors.p, sensors2.p);
    else
      BA_LAUNCH(ba_apply_all_kernel<false>, dim3(std::max(nb, 1)), dim3(128), st, V, Sc, Sp, poses.p, P2, cams.p, C2, points.p, X2,
                sensors.p, sensors2.p);
  }

  // Which tier solves the reduced system: CreateSolverOptions' rule (bundle_adjustment_ceres.cc:203-213, CPU thresholds
  // bundle_adjustment_ceres.h:68-69) on the number of pose blocks; both exact tiers run the explicit reduced system
  void choose_linear_solver(ba_result* out) {
    const int lst = opt.linear_solver_type, nc = V.n_c;
    if (lst < BA_SOLVER_ITERATIVE_SCHUR || lst > BA_SOLVER_SPARSE_SCHUR) throw std::runtime_error("linear_solver_type");
    int tier = lst;
    if (lst == BA_SOLVER_AUTO)
      tier = prob.num_poses <= 50 ? BA_SOLVER_DENSE_SCHUR : (prob.num_poses <= 1000 ? BA_SOLVER_SPARSE_SCHUR : BA_SOLVER_ITERATIVE_SCHUR);
    const bool want_exact = tier == BA_SOLVER_DENSE_SCHUR || tier == BA_SOLVER_SPARSE_SCHUR;
    // an image-sharded solve splits a point's observations over the ranks: only the operator-product formation
    // (every product is all-reduced) is correct there, and only affordable for small systems
    dense_by_products = want_exact && !points_local();
    if (want_exact && dev_switch_int("COLMAP_AMD_BA_DENSE_BY_PRODUCTS", 0) != 0) dense_by_products = true;
    use_dense = want_exact && nc > 0 && nc <= (dense_by_products ? 1024 : 32768);
    out->linear_solver_used = use_dense ? tier : BA_SOLVER_ITERATIVE_SCHUR;
  }

  // column scales of both sides from the squared column norms (jacobi = 0: unit scales)
  void set_scales(int jacobi) {
    BA_LAUNCH(ba_scale_kernel, dim3(std::max(grid_for(V.n_c, 256), 1)), dim3(256), st, V.n_c, diag_c.p, jacobi, scale_c.p);
    BA_LAUNCH(ba_scale_kernel, dim3(std::max(grid_for(V.n_p, 256), 1)), dim3(256), st, V.n_p, diag_p.p, jacobi, scale_p.p);
  }
  // Jacobian, cost, gradient and squared column norms at the current parameters
  void linearize() {
    launch_linearize(true, poses.p, cams.p, points.p, sensors.p, S_COST);
    gradient_and_diag();
  }
  // The first linearisation of a solve (after set_scales(0)): Jacobi scaling from the initial Jacobian, then
  // re-linearised with it
  void initial_linearization() {
    linearize();
    set_scales(opt.jacobi_scaling);
    linearize();
  }
  // Dc, Dp = the LM diagonal at this trust-region radius; Cinv = the inverted damped point blocks
  void damp(double radius) {
    BA_LAUNCH(ba_lm_diag_kernel, dim3(std::max(grid_for(V.n_c, 256), 1)), dim3(256), st, V.n_c, diag_c.p, radius,
              opt.min_lm_diagonal, opt.max_lm_diagonal, Dc.p);
    BA_LAUNCH(ba_lm_diag_kernel, dim3(std::max(grid_for(V.n_p, 256), 1)), dim3(256), st, V.n_p, diag_p.p, radius,
              opt.min_lm_diagonal, opt.max_lm_diagonal, Dp.p);
    BA_LAUNCH(ba_point_blocks_kernel, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, Craw.p, Dp.p, Cinv.p);
  }

  // tiles, points local: the reduced right-hand side's point pass -- which holds E_o and needs C^-1 anyway -- runs inside
  // form_preconditioner() and leaves G_o behind (v is not touched until reduced_rhs())
  bool rhs_pass_fused() const { return V.n_chunks > 0 && V.n_tiles > 0 && points_local(); }

  // Minv = the inverted blocks of the Schur-Jacobi preconditioner. Returns whether its matrix-core kernel ran, between
  // ev2 and ev3 (the caller adds their interval to g_mfma_ms after its next synchronisation)
  bool form_preconditioner() {
    if (V.n_chunks == 0) BA_HIP(hipMemsetAsync(M.p, 0, sizeof(double) * std::max(lay.moff_total, 1), st));
    if (V.n_chunks > 0) {  // (ba_block_mat_finalize_kernel<false> assigns every entry of every block)
      if (rhs_pass_fused())
        BA_LAUNCH((ba_point_pass_tiled_kernel<4>), dim3(V.n_tiles), dim3(TILE_PTS), st, V, Cinv.p, jx.p, gp.p, v.p, dp.p, (double*)nullptr, Gobs.p);
      else
        BA_LAUNCH(ba_obs_schur_g_kernel, dim3(grid_for(V.n_obs, 256)), dim3(256), st, V, Cinv.p, Gobs.p);
      BA_HIP(hipEventRecord(ev2, st));
      with_tier([&](auto t) {
        BA_LAUNCH(ba_block_gram_lds_kernel<t.bd>, dim3(V.n_chunks), dim3(64 * GRAM_WAVES), st, V, Gobs.p);
      });
      BA_HIP(hipEventRecord(ev3, st));
      heavy_reduce(bd * bd);
      BA_LAUNCH(ba_block_mat_finalize_kernel<false>, dim3(grid_for(V.n_blk * bd * bd, 128)), dim3(128), st, V, M.p);
      if (lay.n_paired > 0) {  // observation pairs of a point inside one block: shared intrinsics, rig frames
        with_tier([&](auto t) {
          BA_LAUNCH(ba_obs_w_kernel<t.bd>, dim3(grid_for(V.n_obs, 256)), dim3(256), st, V);
          if (PV.n > 0) {  // per incidence (single GPU)
            BA_LAUNCH(ba_pair_cross_kernel<t.kdt>, dim3(PV.n_chunks), dim3(t.kdt * t.kdt), st, V, PV, Cinv.p);
            BA_LAUNCH(ba_pair_finalize_kernel<t.kdt>, dim3(n_pair_blk, t.kdt * t.kdt / 64), dim3(1024), st, V, PV, pv_pair_blk.p, M.p);
          } else {  // per observation (sharded solves: the local pairs)
            BA_LAUNCH(ba_block_schur_cross_kernel<t.bd>, dim3(V.n_chunks), dim3(64), st, V, Cinv.p);
            heavy_reduce(bd * bd);
            BA_LAUNCH(ba_block_mat_finalize_kernel<true>, dim3(grid_for(V.n_blk * bd * bd, 128)), dim3(128), st, V, M.p);
          }
        });
      }
    }
    if (use_priors())
      BA_LAUNCH(ba_prior_accumulate_kernel<1>, dim3(grid_for(Q.n_tblk, 64)), dim3(64), st, V, Q, M.p, nullptr);
    if (IV.n > 0) {  // image sharding: pairs of observations of a point in a shared intrinsics block on different ranks
      with_tier([&](auto t) {
        const size_t wn = (size_t)IV.n * t.kdt * 3;
        BA_LAUNCH(ba_inc_w_kernel<t.kdt>, dim3(grid_for(IV.n, 128)), dim3(128), st, V, IV, inc_wloc.p);
        BA_HIP(hipMemcpyAsync(inc_wtot.p, inc_wloc.p, sizeof(double) * wn, hipMemcpyDeviceToDevice, st));
        comm.allreduce(inc_wtot.p, wn, st);
        BA_LAUNCH(ba_inc_correct_kernel<t.kdt>, dim3(IV.n_chunks), dim3(t.kdt * t.kdt), st, V, IV, Cinv.p, inc_wloc.p,
                  inc_wtot.p, comm.rank, comm.world);
        BA_LAUNCH(ba_inc_finalize_kernel<t.kdt>, dim3(grid_for((size_t)V.n_blk * t.kdt * t.kdt, 256)), dim3(256), st, V, IV, M.p);
      });
    }
    comm.allreduce(M.p, (size_t)lay.moff_total, st);
    with_tier([&](auto t) {
      BA_LAUNCH(ba_block_invert_kernel<t.bd>, dim3(grid_for(V.n_blk, 64)), dim3(64), st, V, Dc.p, M.p, Minv.p);
    });
    return V.n_chunks > 0;
  }

  // rhs = g_c - E C^-1 g_p  (g_p, C^-1 are global; the J_c^T part is summed over ranks)
  void reduced_rhs() {
    if (!rhs_pass_fused()) point_pass<1>();
    block_jtv_reduced(v.p);
    BA_HIP(hipMemcpyAsync(rhs.p, gc.p, sizeof(double) * V.n_c, hipMemcpyDeviceToDevice, st));
    BA_LAUNCH(ba_add_kernel, dim3(grid_for(V.n_c, 256)), dim3(256), st, V.n_c, tmpc.p, rhs.p);
  }

  // Back-substitution y_p = C^-1 (g_p - E^T y_c), step = -(y_c, y_p), and the model cost change
  // -(J step).(r + J step / 2) into scalars[S_MODEL]
  void back_substitute_and_model_change() {
    if (V.n_obs > 0) obs_jx(x.p);
    // (tiles: the same launch leaves the model cost change's partial sums behind -- columns, jx and y_p are in its registers)
    const bool model_fused = points_local() && V.n_tiles > 0;
    if (model_fused) {
      BA_LAUNCH((ba_point_pass_tiled_kernel<3>), dim3(V.n_tiles), dim3(TILE_PTS), st, V, Cinv.p, jx.p, gp.p, v.p, dp.p, partials.p);
    } else if (points_local()) {
      point_pass<2>();
    } else {
      BA_HIP(hipMemsetAsync(tbuf.p, 0, sizeof(double) * std::max(V.n_p, 1), st));
      BA_LAUNCH(ba_point_t_kernel, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, jx.p, tbuf.p);
      comm.allreduce(tbuf.p, V.n_p, st);
      BA_LAUNCH(ba_point_apply_kernel<2>, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, Cinv.p, jx.p, gp.p,
                tbuf.p, v.p, dp.p);
    }
    // (the negated, unscaled camera-side step: only the priors' model term reads it; Plus() forms its own)
    if (use_priors())
      BA_LAUNCH(ba_axpby_kernel, dim3(std::max(grid_for(V.n_c, 256), 1)), dim3(256), st, V.n_c, -1.0, x.p, nullptr, stepc.p);
    // jx = J_c y_c of the back-substitution is still in place
    if (V.n_tiles == 0)
      BA_LAUNCH(ba_model_from_jx_kernel, dim3(grid_for(V.n_points, 256)), dim3(256), st, V, jx.p, dp.p, partials.p);
    else if (!model_fused)
      BA_LAUNCH(ba_point_reduce_tiled_kernel<1>, dim3(V.n_tiles), dim3(TILE_PTS), st, V, jx.p, dp.p, partials.p, nullptr, nullptr);
    BA_LAUNCH(ba_final_sum_kernel, dim3(1), dim3(1024), st, partials.p, V.n_tiles > 0 ? V.n_tiles : grid_for(V.n_points, 256),
              scalars.p + S_MODEL);
    if (use_priors()) BA_LAUNCH(ba_prior_model_kernel, dim3(1), dim3(256), st, Q, stepc.p, scalars.p + S_MODEL);
  }

  // candidate = Plus(x, step), the Jacobi scaling of the step undone, and its cost into scalars[S_NEWCOST]
  void evaluate_candidate() {
    apply_step(x.p, scale_c.p, dp.p, scale_p.p, 3, false, poses2.p, cams2.p, points2.p);  // step = (-y) * column scale
    launch_linearize(false, poses2.p, cams2.p, points2.p, sensors2.p, S_NEWCOST);
  }

  // The result into the caller's arrays: variable blocks only (constant blocks stay bit-identical)
  void write_back() {
    auto copy_variable = [](double* dst, const std::vector<double>& src, const std::vector<int>& off, int count, size_t stride) {
      for (int i = 0; i < count; ++i)
        if (off[i] >= 0) std::memcpy(dst + stride * i, src.data() + stride * i, stride * sizeof(double));
    };
    BA_LAUNCH(ba_renorm_quat_kernel, dim3(grid_for(V.n_poses, 128)), dim3(128), st, V, poses.p);
    if (comm.world > 1 && comm.by_point) {
      // every rank moved its own points only: zero the others' variable points and sum over ranks
      BA_LAUNCH(ba_keep_own_points_kernel, dim3(grid_for(V.n_points, 128)), dim3(128), st, V, comm.rank, comm.world, points.p);
      comm.allreduce(points.p, 3 * (size_t)V.n_points, st);
    }
    if (V.sens_off) {
      BA_LAUNCH(ba_renorm_sensor_quat_kernel, dim3(grid_for(V.n_sensors, 128)), dim3(128), st, V, sensors.p);
      std::vector<double> hs(sensors.n);
      BA_HIP(hipMemcpyAsync(hs.data(), sensors.p, sizeof(double) * sensors.n, hipMemcpyDeviceToHost, st));
      BA_HIP(hipStreamSynchronize(st));
      copy_variable(prob.sensors, hs, lay.sens_off, prob.num_sensors, 7);
    }
    std::vector<double> hp(poses.n), hc(cams.n), hx(points.n);
    BA_HIP(hipMemcpyAsync(hp.data(), poses.p, sizeof(double) * poses.n, hipMemcpyDeviceToHost, st));
    BA_HIP(hipMemcpyAsync(hc.data(), cams.p, sizeof(double) * cams.n, hipMemcpyDeviceToHost, st));
    BA_HIP(hipMemcpyAsync(hx.data(), points.p, sizeof(double) * points.n, hipMemcpyDeviceToHost, st));
    BA_HIP(hipStreamSynchronize(st));
    copy_variable(prob.poses, hp, lay.pose_off, prob.num_poses, 7);
    copy_variable(prob.cams, hc, lay.cam_off, prob.num_cams, BA_CAM_STRIDE);
    copy_variable(prob.points, hx, lay.pt_off, prob.num_points, 3);
  }

  void run(ba_result* out) {
    out->termination_type = BA_FAILURE;
    if (build(out) == 0) return;
    choose_linear_solver(out);
    if (use_dense) {
      prepare_exact(V.n_c);
      if (!dense_by_products) open_cholesky_lookahead(), build_pair_lists(form_args());
      BA_HIP(hipDeviceSynchronize());  // the allocations' memsets run on the NULL stream
    }
    if (comm.world > 1) {
      // which PCG loop runs must not depend on the rank: one sum over ranks of "this rank could not take the pipelined one"
      const double mine = (!use_priors() && V.n_chunks > 0 && V.n_obs > 0) ? 0.0 : 1.0;
      BA_HIP(hipMemcpyAsync(scalars.p + S_ITER, &mine, sizeof(double), hipMemcpyHostToDevice, st));
      BA_HIP(hipStreamSynchronize(st));
      comm.allreduce(scalars.p + S_ITER, 1, st);
      pcg_all_ranks_have_work = scalar(S_ITER) == 0.0;
    }
    factor_ms = 0.0;
    g_spmv_ms = 0.0; g_spmv_launches = 0;
    g_mfma_ms = 0.0; g_mfma_launches = 0;
    g_pcg_pipelined_solves = 0; g_pcg_stepwise_solves = 0;
    // bytes one implicit-Schur product streams: Jc (2x10) once for jx, Jp (2x3) twice, jx/v, Jc again
    g_spmv_bytes = (long long)V.n_obs * (2 * (PD + kd) * 8 * 2 + 6 * 8 * 2 + 4 * 8 * 3);

    double radius = opt.initial_trust_region_radius, decrease_factor = 2.0;
    int invalid_steps = 0;
    bool need_linearize = true;
    double cost = 0.0;
    auto decrease_radius = [&] { radius /= decrease_factor; decrease_factor *= 2.0; };
    auto terminate = [&](int type, int iterations) { out->termination_type = type; out->num_iterations = iterations; };
    set_scales(0);  // scale = 1 until computed
    BA_HIP(hipStreamSynchronize(st));
    const auto t_start = std::chrono::steady_clock::now();
    out->setup_seconds = std::chrono::duration<double>(t_start - t_entry).count();
    // ceres::IterationCallback as COLMAP uses it (controllers/bundle_adjustment.cc:40-57): asked between two
    // iterations; the parameter blocks hold the last accepted step when it ends the solve
    auto user_stop = [&](int iteration, double cost_now, double cost_change, bool step_ok, double rad, int lin) -> bool {
      if (!opt.iteration_callback) return false;
      ba_iteration_summary sm;
      sm.iteration = iteration; sm.step_is_successful = step_ok ? 1 : 0; sm.linear_solver_iterations = lin;
      sm.cost = cost_now; sm.cost_change = cost_change; sm.trust_region_radius = rad;
      sm.cumulative_time_in_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
      const int rc = opt.iteration_callback(opt.iteration_callback_user, &sm);
      if (rc == BA_CALLBACK_CONTINUE) return false;
      terminate(rc == BA_CALLBACK_TERMINATE ? BA_USER_SUCCESS : BA_USER_FAILURE, iteration);
      return true;
    };

    for (int iter = 0;; ++iter) {
      if (need_linearize) {
        if (iter == 0) initial_linearization();
        else linearize();
        const bool one_sync = comm.world == 1;  // cost and gradient norm read together below
        if (!one_sync) cost = scalar_sum(S_COST);
        // projected-gradient test: ||x - Plus(x, -g)||_inf with the unscaled gradient g = s * g_scaled
        // (the stored Jacobian is column-scaled: g_scaled = s * g, so g = g_scaled / s)
        // (one launch: the step -g / s is formed on the fly, Plus() of all blocks, the max of the differences)
        zero_scalar(S_GMAX);
        apply_step(gc.p, scale_c.p, gp.p, scale_p.p, 1, true, poses2.p, cams2.p, points2.p);
        double gmax;
        if (one_sync) {
          double h[NSCALAR];
          scalars_to_host(h);
          cost = h[S_COST];
          gmax = h[S_GMAX];
        } else {
          gmax = scalar_max(S_GMAX);
        }
        if (iter == 0) out->initial_cost = cost;
        if (gmax <= opt.gradient_tolerance) {
          terminate(BA_CONVERGENCE, iter);
          break;
        }
        need_linearize = false;
        if (iter == 0 && user_stop(0, cost, 0.0, true, radius, 0)) break;
      }
      if (iter >= opt.max_num_iterations) {
        terminate(BA_NO_CONVERGENCE, iter);
        break;
      }
      // the damped system at this radius, its linear solve, the step and its predicted decrease
      damp(radius);
      int lin_iters = 0;
      bool mfma_pending = false;
      if (V.n_c > 0) {
        mfma_pending = form_preconditioner();
        reduced_rhs();
        lin_iters = use_dense ? dense_schur() : pcg(opt.max_linear_solver_iterations, opt.eta);
        out->total_linear_iterations += lin_iters;
      }
      back_substitute_and_model_change();
      // Single GPU: the candidate is evaluated before the model change is known (it is almost always valid; an
      // invalid step wastes one cost evaluation) and both numbers come back with one synchronisation.
      const bool speculate = comm.world == 1;
      double spec_new_cost = 0.0, model_change;
      if (speculate) {
        evaluate_candidate();
        double h[NSCALAR];
        scalars_to_host(h);
        model_change = h[S_MODEL];
        spec_new_cost = h[S_NEWCOST];
      } else {
        model_change = scalar_sum(S_MODEL);  // (synchronises the stream)
      }
      if (mfma_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev2, ev3) == hipSuccess) { g_mfma_ms += ms; g_mfma_launches += 1; }
      }
      bool accepted = false;
      double new_cost = cost;
      if (!(model_change > 0.0) || !std::isfinite(model_change)) {
        if (++invalid_steps >= opt.max_num_consecutive_invalid_steps) {
          terminate(BA_FAILURE, iter + 1);
          break;
        }
        decrease_radius();
      } else {
        invalid_steps = 0;
        new_cost = spec_new_cost;
        if (!speculate) {
          evaluate_candidate();
          new_cost = scalar_sum(S_NEWCOST);
        }
        const double rho = (cost - new_cost) / model_change;
        if (rho > opt.min_relative_decrease) {
          accepted = true;
          std::swap(poses.p, poses2.p); std::swap(cams.p, cams2.p); std::swap(points.p, points2.p);
          if (V.sens_off) std::swap(sensors.p, sensors2.p);
          V.poses = poses.p; V.cams = cams.p; V.points = points.p; V.sensors = sensors.p;
          const double t = 2.0 * rho - 1.0;
          radius = radius / std::max(1.0 / 3.0, 1.0 - t * t * t);
          radius = std::min(opt.max_trust_region_radius, radius);
          decrease_factor = 2.0;
          out->num_successful_steps++;
          need_linearize = true;
          if (opt.function_tolerance > 0 && std::fabs(cost - new_cost) <= opt.function_tolerance * cost) {
            log(out, new_cost, radius, lin_iters);
            terminate(BA_CONVERGENCE, iter + 1);
            break;
          }
        } else {
          decrease_radius();
        }
      }
      log(out, accepted ? new_cost : cost, radius, lin_iters);
      if (radius < opt.min_trust_region_radius) {
        terminate(BA_CONVERGENCE, iter + 1);
        break;
      }
      if (user_stop(iter + 1, accepted ? new_cost : cost, accepted ? cost - new_cost : 0.0, accepted, radius, lin_iters)) break;
    }
    launch_linearize(false, poses.p, cams.p, points.p, sensors.p, S_NEWCOST);
    out->final_cost = scalar_sum(S_NEWCOST);
    out->lm_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    out->factor_seconds = factor_ms * 1e-3;
    write_back();
  }

  int estimate_covariance(const ba_covariance_options& co, CovHandle& h);  // (below, with its kernels)

  void log(ba_result* out, double c, double rad, int lin) {
    if (out->log_cost && out->num_logged < opt.max_log) {
      out->log_cost[out->num_logged] = c;
      if (out->log_radius) out->log_radius[out->num_logged] = rad;
      if (out->log_linear_iters) out->log_linear_iters[out->num_logged] = lin;
      out->num_logged++;
    }
  }
};

// ------------------------------------------------------------------------------------------
// Covariance estimation (include/colmap_amd_ba_covariance.h)
// ------------------------------------------------------------------------------------------

// One pass over the points: the damped, scaled C^-1 = (E_s^T E_s + damping s_p^2)^-1 the formation reads (no LM
// diagonal), and the unscaled covariance s_p C^-1 s_p = (E^T E + damping I)^-1 (row-major 3 x 3 per point).
__global__ void ba_cov_point_kernel(View V, const double* __restrict__ Craw, double damping, double* __restrict__ Cinv,
                                    double* __restrict__ cov) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V.n_points) return;
  const int off = V.pt_off[j];
  if (off < 0) return;
  const double s[3] = {V.scale_p[off], V.scale_p[off + 1], V.scale_p[off + 2]};
  double C[6];
  for (int e = 0; e < 6; ++e) C[e] = Craw[(size_t)e * V.n_points + j];
  C[0] += damping * s[0] * s[0];
  C[3] += damping * s[1] * s[1];
  C[5] += damping * s[2] * s[2];
  const double a = C[0], b = C[1], c = C[2], d = C[3], e = C[4], f = C[5];
  const double A = d * f - e * e, B = c * e - b * f, Cc = b * e - c * d;
  const double id = 1.0 / (a * A + b * B + c * Cc);
  const double m[9] = {A * id, B * id, Cc * id, B * id, (a * f - c * c) * id, (b * c - a * e) * id,
                       Cc * id, (b * c - a * e) * id, (a * d - b * b) * id};
  double* out = Cinv + 9 * (size_t)j;
  double* cv = cov + 9 * (size_t)j;
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) {
      out[3 * r + q] = m[3 * r + q];
      cv[3 * r + q] = s[r] * m[3 * r + q] * s[q];
    }
}

// Diagonal of the covariance system before the factorisation: rows [0, n_o) are the others (+ damping s^2 when they are
// eliminated, damp_o = 0 with BA_COV_ALL), rows [n_o, n_op) the identity rows that pad them to a multiple of 64.
__global__ void ba_cov_diag_kernel(double* __restrict__ S, int n, int n_o, int n_op, double damp_o,
                                   const double* __restrict__ scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_op) return;
  double* d = S + (size_t)i * n + i;
  if (i >= n_o) *d = 1.0;
  else *d += damp_o * scale[i] * scale[i];
}

// Pivots of the factorisation in unscaled units: d_i = (L_ii / s_i)^2.
__global__ void ba_cov_pivot_kernel(const double* __restrict__ S, int n, const double* __restrict__ scale,
                                    double* __restrict__ d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double l = S[(size_t)i * n + i] / scale[i];
  d[i] = l * l;
}

struct CovHandle {
  int device = 0;
  int mode = BA_COV_ALL;
  int n = 0, n_o = 0, n_op = 0;  // factored dimension; others and their padded width (the poses start at n_op)
  int j0 = 0;                    // first 64-block column of X that was inverted
  double* X = nullptr;           // rows / columns [64 j0, n) of L^-1 (device, (n - 64 j0)^2), lower triangular
  double* scale = nullptr;       // [n] Jacobi scales of the rows of X (device; 1 on the padding)
  Stream st;
  Event ev_a, ev_b;
  std::vector<int> pose_off, pose_dim, cam_off, cam_dim, sens_off, sens_dim;  // offsets in X, -1: no result
  std::vector<double> point_cov;  // [num_points][9]
  std::vector<char> point_has;
  double form_ms = 0.0, factor_ms = 0.0, inverse_ms = 0.0, extract_ms = 0.0;
  ~CovHandle() { if (X) (void)hipFree(X); if (scale) (void)hipFree(scale); }
};

double elapsed_ms(hipEvent_t a, hipEvent_t b) {
  BA_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  BA_HIP(hipEventElapsedTime(&ms, a, b));
  return ms;
}

// Sets up the solver's linearisation at the current parameters (Jacobi scales from the same Jacobian, as the LM loop's
// first iteration), then points, formation, factorisation and triangular inverse. Returns BA_COV_OK or
// BA_COV_NOT_ESTIMABLE (g_ba_error holds the message); throws on errors.
int Solver::estimate_covariance(const ba_covariance_options& co, CovHandle& h) {
  const ba_problem& p = prob;
  h.mode = co.params;
  h.pose_off.assign(p.num_poses, -1); h.pose_dim.assign(p.num_poses, 0);
  h.cam_off.assign(p.num_cams, -1); h.cam_dim.assign(p.num_cams, 0);
  h.sens_off.assign(std::max(p.num_sensors, 0), -1); h.sens_dim.assign(std::max(p.num_sensors, 0), 0);
  h.point_cov.assign(9 * (size_t)std::max(p.num_points, 0), 0.0);
  h.point_has.assign(std::max(p.num_points, 0), 0);
  ba_result dummy{};
  if (build(&dummy) == 0) return BA_COV_OK;  // no variable block is observed: every query has no result
  const int nc = V.n_c;
  set_scales(0);
  initial_linearization();
  // 1. points
  Buf<double> pcov;
  pcov.alloc(9 * (size_t)std::max(p.num_points, 1));
  if (p.num_points > 0)
    BA_LAUNCH(ba_cov_point_kernel, dim3(grid_for(p.num_points, 128)), dim3(128), st, V, Craw.p, co.damping, Cinv.p, pcov.p);
  if (co.params != BA_COV_POSES) {
    BA_HIP(hipMemcpyAsync(h.point_cov.data(), pcov.p, sizeof(double) * h.point_cov.size(), hipMemcpyDeviceToHost, st));
    BA_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < p.num_points; ++j) h.point_has[j] = lay.pt_off[j] >= 0;
  }
  if (co.params == BA_COV_POINTS || nc == 0) return BA_COV_OK;
  // 2. the camera-side order of the covariance system: others (intrinsics, then sensor_from_rig blocks, in the solver's
  // order) padded with identity rows to a multiple of 64, then the poses
  const std::vector<int>&pdim = lay.pose_dim, &cdim = lay.cam_dim;
  int n_pd = 0;
  for (int i = 0; i < p.num_poses; ++i) n_pd += lay.pose_off[i] >= 0 ? pdim[i] : 0;
  const int n_o = nc - n_pd;  // the solver's layout: poses [0, n_pd), then intrinsics and sensors
  const int n_op = (n_o + 63) / 64 * 64;
  const int n = n_op + n_pd;
  if (n > 32768)
    throw std::runtime_error("covariance: camera-side dimension " + std::to_string(n) + " exceeds the limit of 32768");
  auto remap = [&](int off) { return off < 0 ? -1 : (off < n_pd ? off + n_op : off - n_pd); };
  std::vector<int> npose(p.num_poses), ncam(p.num_cams), nsens(lay.sens_off.size());
  for (int i = 0; i < p.num_poses; ++i) npose[i] = remap(lay.pose_off[i]);
  for (int k = 0; k < p.num_cams; ++k) ncam[k] = remap(lay.cam_off[k]);
  for (size_t k = 0; k < nsens.size(); ++k) nsens[k] = remap(lay.sens_off[k]);
  std::vector<double> sc_old(std::max(nc, 1)), sc(n, 1.0);
  BA_HIP(hipMemcpyAsync(sc_old.data(), scale_c.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
  BA_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < nc; ++i) sc[remap(i)] = sc_old[i];
  Buf<int> d_pose, d_cam, d_sens, d_po, d_so;
  d_pose.upload(npose); d_cam.upload(ncam);
  if (!nsens.empty()) d_sens.upload(nsens);
  BA_HIP(hipMalloc(reinterpret_cast<void**>(&h.scale), sizeof(double) * n));
  BA_HIP(hipMemcpy(h.scale, sc.data(), sizeof(double) * n, hipMemcpyHostToDevice));
  if (use_priors()) {
    std::vector<int> po(Q.n), so(Q.n);
    for (int k = 0; k < Q.n; ++k) { po[k] = remap(lay.pr_po[k]); so[k] = remap(lay.pr_so[k]); }
    d_po.upload(po); d_so.upload(so);
  }
  prepare_exact(n);
  ba_explicit::FormArgs fa = form_args();
  fa.n_c = n;
  fa.pose_off = d_pose.p; fa.cam_off = d_cam.p;
  fa.sens_off = V.sens_off ? d_sens.p : nullptr;
  BA_HIP(hipDeviceSynchronize());  // (uploads and memsets on the NULL stream)
  build_pair_lists(fa);
  Buf<double> zrhs, xsol, piv;
  zrhs.alloc(n); xsol.alloc(n); piv.alloc(n);
  BA_HIP(hipDeviceSynchronize());
  BA_HIP(hipEventRecord(ev2, st));
  form_reduced_system(fa, d_po.p, d_so.p);
  if (n_op > 0)
    BA_LAUNCH(ba_cov_diag_kernel, dim3(grid_for(n_op, 256)), dim3(256), st, Sdense.p, n, n_o, n_op,
              co.params == BA_COV_ALL ? 0.0 : co.damping, h.scale);
  BA_HIP(hipEventRecord(ev3, st));
  // 3. factorisation (the right-hand side is zero; its solution is not used)
  open_cholesky_lookahead();
  double fms = 0.0;
  ba_explicit::factor_solve(Sdense.p, n, zrhs.p, xsol.p, cholesky_workspace(), st, ev0, ev1, &fms);
  h.form_ms = elapsed_ms(ev2, ev3); h.factor_ms = fms;
  BA_LAUNCH(ba_cov_pivot_kernel, dim3(grid_for(n, 256)), dim3(256), st, Sdense.p, n, h.scale, piv.p);
  std::vector<double> d(n);
  int info[2] = {0, 0};
  BA_HIP(hipMemcpyAsync(d.data(), piv.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  BA_HIP(hipMemcpyAsync(info, chol_info.p, sizeof(info), hipMemcpyDeviceToHost, st));
  BA_HIP(hipStreamSynchronize(st));
  // 4. rank: the columns of the matrix whose inverse is returned (with eliminated others, the poses only)
  int cols = 0, rank = 0;
  for (int i = 0; i < n; ++i) {
    const bool counted = i >= n_op || (co.params == BA_COV_ALL && i < n_o);
    if (!counted) continue;
    ++cols;
    rank += d[i] > 1e-6 ? 1 : 0;  // (a NaN pivot is not counted)
  }
  const bool failed = info[0] != 0;  // a pivot that was not positive (the others' block included)
  if (failed && cols > 0 && rank == cols) --rank;
  if (failed || rank < cols) {
    g_ba_error = "Unable to compute covariance. The Schur complement on pose/other parameters is rank deficient. "
                 "Number of columns: " + std::to_string(cols) + ", rank: " + std::to_string(rank) +
                 ". This is likely due to the pose/other parameters being underconstrained with Gauge ambiguity or "
                 "other degeneracies.";
    return BA_COV_NOT_ESTIMABLE;
  }
  // 5. X = L^-1 (only the poses' block columns when the others were eliminated)
  h.n = n; h.n_o = n_o; h.n_op = n_op;
  h.j0 = co.params == BA_COV_ALL ? 0 : n_op / 64;
  const size_t nx = (size_t)(n - 64 * h.j0);  // only the inverted trailing part is stored
  BA_HIP(hipMalloc(reinterpret_cast<void**>(&h.X), sizeof(double) * std::max<size_t>(nx * nx, 1)));
  BA_HIP(hipEventRecord(ev2, st));
  ba_explicit::tri_inverse(Sdense.p, n, h.j0, chol_linv.p, h.X, st);
  BA_HIP(hipEventRecord(ev3, st));
  h.inverse_ms = elapsed_ms(ev2, ev3);
  for (int i = 0; i < p.num_poses; ++i)
    if (npose[i] >= 0) { h.pose_off[i] = npose[i]; h.pose_dim[i] = pdim[i]; }
  if (co.params == BA_COV_ALL) {
    for (int k = 0; k < p.num_cams; ++k)
      if (ncam[k] >= 0) { h.cam_off[k] = ncam[k]; h.cam_dim[k] = cdim[k]; }
    for (size_t k = 0; k < nsens.size(); ++k)
      if (nsens[k] >= 0) { h.sens_off[k] = nsens[k]; h.sens_dim[k] = 6; }
  }
  return BA_COV_OK;
}

// gpu_index < 0: the calling thread's current device
void select_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    throw std::runtime_error("no HIP device available: the MI355X bundle-adjustment backend has no CPU fallback");
  if (gpu_index >= ndev) throw std::runtime_error("gpu_index out of range");
  if (gpu_index >= 0) BA_HIP(hipSetDevice(gpu_index));
}

bool cov_block(const CovHandle& h, int kind, int index, int* off, int* dim) {
  const std::vector<int>* o = kind == BA_COV_KIND_POSE ? &h.pose_off : kind == BA_COV_KIND_CAMERA ? &h.cam_off
                            : kind == BA_COV_KIND_SENSOR ? &h.sens_off : nullptr;
  const std::vector<int>* d = kind == BA_COV_KIND_POSE ? &h.pose_dim : kind == BA_COV_KIND_CAMERA ? &h.cam_dim : &h.sens_dim;
  if (!o || index < 0 || index >= (int)o->size() || (*o)[index] < 0) return false;
  *off = (*o)[index];
  *dim = (*d)[index];
  return true;
}

}  // namespace

struct ba_covariance {
  CovHandle h;
};

extern "C" {

int32_t ba_abi_version(void) { return COLMAP_AMD_BA_ABI_VERSION; }

void ba_options_init(ba_options* o) {
  // CeresBundleAdjustmentOptions ctor (bundle_adjustment_ceres.cc:102-115) over Ceres defaults
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 100;
  o->max_linear_solver_iterations = 200;
  o->function_tolerance = 0.0;
  o->gradient_tolerance = 1e-4;
  o->parameter_tolerance = 0.0;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->eta = 1e-1;
  o->max_num_consecutive_invalid_steps = 10;
  o->jacobi_scaling = 1;
  o->loss_type = BA_LOSS_TRIVIAL;  // bundle_adjustment_ceres.h:42-51
  o->loss_scale = 1.0;
  o->linear_solver_type = BA_SOLVER_ITERATIVE_SCHUR;
}

static int SolveImpl(ba_problem* problem, const ba_options* options, int32_t gpu_index, const ba_comm* c,
                     ba_result* result) {
  try {
    if (!problem || !options || !result) throw std::runtime_error("null argument");
    double* lc = result->log_cost;
    double* lr = result->log_radius;
    int32_t* ll = result->log_linear_iters;
    std::memset(result, 0, sizeof(*result));
    result->log_cost = lc; result->log_radius = lr; result->log_linear_iters = ll;
    result->termination_type = BA_FAILURE;
    select_device(gpu_index);
    Comm comm;
    if (c) {
      if (c->world_size < 1 || c->rank < 0 || c->rank >= c->world_size) throw std::runtime_error("bad rank / world_size");
      comm.rank = c->rank;
      comm.world = c->world_size;
      comm.fn = c->allreduce;
      comm.user = c->user;
      comm.nccl = reinterpret_cast<ncclComm_t>(c->rccl_comm);
      comm.by_point = c->sharding == BA_SHARD_BY_POINT;
      if (c->sharding != BA_SHARD_BY_IMAGE && c->sharding != BA_SHARD_BY_POINT)
        throw std::runtime_error("ba_comm.sharding must be BA_SHARD_BY_IMAGE or BA_SHARD_BY_POINT");
      if (comm.world > 1 && !comm.nccl && !comm.fn) throw std::runtime_error("ba_comm needs rccl_comm or an allreduce callback");
    }
    Solver s(*problem, *options, comm);
    s.run(result);
    return 0;
  } catch (const std::exception& e) {
    g_ba_error = e.what();
    return 1;
  }
}

int ba_solve(ba_problem* problem, const ba_options* options, int32_t gpu_index, ba_result* result) {
  return SolveImpl(problem, options, gpu_index, nullptr, result);
}

int ba_solve_sharded(ba_problem* problem, const ba_options* options, int32_t gpu_index, const ba_comm* comm,
                     ba_result* result) {
  return SolveImpl(problem, options, gpu_index, comm, result);
}

static int64_t ShardNumObservations(const ba_problem* p, int32_t rank, int32_t world_size, bool by_point) {
  if (!p || world_size < 1 || rank < 0 || rank >= world_size) return -1;
  std::vector<int> cam_nvar(p->num_cams, 0);
  for (int k = 0; k < p->num_cams; ++k) {
    const int P = colmap_amd::camera_models::num_params(p->cam_model[k]);
    if (P < 0) return -1;
    for (int j = 0; j < P; ++j)
      if (!p->cam_const[(size_t)k * BA_CAM_STRIDE + j]) ++cam_nvar[k];
  }
  int64_t n = 0;
  for (int64_t o = 0; o < p->num_obs; ++o)
    if (ba_layout::is_active(*p, cam_nvar.data(), o) && (by_point ? p->obs_point[o] : p->obs_pose[o]) % world_size == rank) ++n;
  return n;
}

int64_t ba_shard_num_observations(const ba_problem* p, int32_t rank, int32_t world_size) {
  return ShardNumObservations(p, rank, world_size, false);
}
int64_t ba_shard_num_observations_by_point(const ba_problem* p, int32_t rank, int32_t world_size) {
  return ShardNumObservations(p, rank, world_size, true);
}

int ba_rccl_unique_id(char id[128]) {
  static_assert(sizeof(ncclUniqueId) <= 128, "ncclUniqueId larger than the ABI buffer");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) { g_ba_error = "ncclGetUniqueId failed"; return 1; }
  std::memset(id, 0, 128);
  std::memcpy(id, &u, sizeof(u));
  return 0;
}

int ba_rccl_comm_create(const char id[128], int32_t rank, int32_t world_size, int32_t gpu_index, void** comm) {
  try {
    if (!comm) throw std::runtime_error("null argument");
    if (gpu_index >= 0) BA_HIP(hipSetDevice(gpu_index));
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclComm_t c = nullptr;
    const ncclResult_t r = ncclCommInitRank(&c, world_size, u, rank);
    if (r != ncclSuccess) throw std::runtime_error(std::string("ncclCommInitRank failed: ") + ncclGetErrorString(r));
    *comm = c;
    return 0;
  } catch (const std::exception& e) {
    g_ba_error = e.what();
    return 1;
  }
}

void ba_rccl_comm_destroy(void* comm) {
  if (comm) (void)ncclCommDestroy(reinterpret_cast<ncclComm_t>(comm));
}

int ba_last_mfma_timing(double* total_ms, int64_t* launches) {
  if (total_ms) *total_ms = g_mfma_ms;
  if (launches) *launches = g_mfma_launches;
  return 0;
}

int ba_last_pcg_loops(int64_t* pipelined_solves, int64_t* stepwise_solves) {
  if (pipelined_solves) *pipelined_solves = g_pcg_pipelined_solves;
  if (stepwise_solves) *stepwise_solves = g_pcg_stepwise_solves;
  return 0;
}

int ba_last_spmv_timing(double* total_ms, int64_t* launches, int64_t* bytes_per_launch) {
  if (total_ms) *total_ms = g_spmv_ms;
  if (launches) *launches = g_spmv_launches;
  if (bytes_per_launch) *bytes_per_launch = g_spmv_bytes;
  return 0;
}

void ba_covariance_options_init(ba_covariance_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->params = BA_COV_ALL;  // BACovarianceOptions (covariance.h)
  o->damping = 1e-8;
}

int ba_estimate_covariance(const ba_problem* problem, const ba_options* options, const ba_covariance_options* cov_options,
                           int32_t gpu_index, ba_covariance** out) {
  if (out) *out = nullptr;
  try {
    if (!problem || !options || !cov_options || !out) throw std::runtime_error("null argument");
    if (cov_options->params < BA_COV_POSES || cov_options->params > BA_COV_ALL)
      throw std::runtime_error("ba_covariance_options.params");
    if (!(cov_options->damping >= 0.0)) throw std::runtime_error("ba_covariance_options.damping must be >= 0");
    select_device(gpu_index);
    auto cov = std::make_unique<ba_covariance>();
    CovHandle& h = cov->h;
    BA_HIP(hipGetDevice(&h.device));
    int rc;
    {
      Comm comm;
      // the solver only reads the problem here: it uploads copies and never writes back
      Solver s(*const_cast<ba_problem*>(problem), *options, comm);
      rc = s.estimate_covariance(*cov_options, h);
    }
    if (rc != BA_COV_OK) return rc;
    h.st.create(); h.ev_a.create(); h.ev_b.create();
    *out = cov.release();
    return BA_COV_OK;
  } catch (const std::exception& e) {
    g_ba_error = e.what();
    return BA_COV_ERROR;
  }
}

int ba_covariance_block_dim(const ba_covariance* cov, int32_t kind, int32_t index, int32_t* dim) {
  if (!cov || !dim) return BA_COV_ERROR;
  int off = 0, d = 0;
  *dim = cov_block(cov->h, kind, index, &off, &d) ? d : 0;
  return *dim > 0 ? BA_COV_OK : BA_COV_NO_RESULT;
}

int ba_covariance_point(const ba_covariance* cov, int32_t index, double out[9]) {
  if (!cov || !out) return BA_COV_ERROR;
  const CovHandle& h = cov->h;
  if (index < 0 || index >= (int)h.point_has.size() || !h.point_has[index]) return BA_COV_NO_RESULT;
  std::memcpy(out, h.point_cov.data() + 9 * (size_t)index, 9 * sizeof(double));
  return BA_COV_OK;
}

int ba_covariance_blocks(ba_covariance* cov, int32_t count, const ba_covariance_pair* pairs, double* out, int32_t* found) {
  try {
    if (!cov || count < 0 || (count > 0 && (!pairs || !out || !found))) throw std::runtime_error("null argument");
    CovHandle& h = cov->h;
    std::vector<ba_explicit::CovPair> req;
    std::vector<int> slot;
    for (int k = 0; k < count; ++k) {
      ba_explicit::CovPair cp{};
      const bool ok = h.X && cov_block(h, pairs[k].kind_a, pairs[k].index_a, &cp.a0, &cp.da) &&
                      cov_block(h, pairs[k].kind_b, pairs[k].index_b, &cp.b0, &cp.db);
      found[k] = ok ? 1 : 0;
      if (ok) {
        cp.a0 -= 64 * h.j0;
        cp.b0 -= 64 * h.j0;
        const int nx = h.n - 64 * h.j0;
        if (cp.a0 < 0 || cp.b0 < 0 || cp.a0 + cp.da > nx || cp.b0 + cp.db > nx || cp.da > 16 || cp.db > 16)
          throw std::runtime_error("covariance: block outside the inverted part");
        req.push_back(cp);
        slot.push_back(k);
      }
    }
    if (req.empty()) return BA_COV_OK;
    BA_HIP(hipSetDevice(h.device));
    Buf<ba_explicit::CovPair> dpairs;
    Buf<double> dout;
    dpairs.upload(req);
    dout.alloc(req.size() * ba_explicit::kCovSlot);
    BA_HIP(hipDeviceSynchronize());  // (uploads on the NULL stream)
    BA_HIP(hipEventRecord(h.ev_a, h.st));
    const int xo = 64 * h.j0;  // X's first row / column (the pose blocks queried lie beyond it)
    ba_explicit::extract_cov_blocks(h.X, h.n - xo, dpairs.p, (int)req.size(), h.scale + xo, dout.p, h.st);
    BA_HIP(hipGetLastError());
    BA_HIP(hipEventRecord(h.ev_b, h.st));
    std::vector<double> hout(dout.n);
    BA_HIP(hipMemcpyAsync(hout.data(), dout.p, sizeof(double) * dout.n, hipMemcpyDeviceToHost, h.st));
    BA_HIP(hipStreamSynchronize(h.st));
    h.extract_ms = elapsed_ms(h.ev_a, h.ev_b);
    for (size_t q = 0; q < req.size(); ++q)
      std::memcpy(out + (size_t)slot[q] * BA_COV_SLOT, hout.data() + q * ba_explicit::kCovSlot,
                  sizeof(double) * req[q].da * req[q].db);
    return BA_COV_OK;
  } catch (const std::exception& e) {
    g_ba_error = e.what();
    return BA_COV_ERROR;
  }
}

int ba_covariance_timing(const ba_covariance* cov, double* form_ms, double* factor_ms, double* inverse_ms,
                         double* extract_ms, int32_t* n, int32_t* n_inv) {
  if (!cov) return BA_COV_ERROR;
  const CovHandle& h = cov->h;
  if (form_ms) *form_ms = h.form_ms;
  if (factor_ms) *factor_ms = h.factor_ms;
  if (inverse_ms) *inverse_ms = h.inverse_ms;
  if (extract_ms) *extract_ms = h.extract_ms;
  if (n) *n = h.n;
  if (n_inv) *n_inv = std::max(h.n - 64 * h.j0, 0);
  return BA_COV_OK;
}

void ba_covariance_destroy(ba_covariance* cov) {
  if (!cov) return;
  (void)hipSetDevice(cov->h.device);
  delete cov;
}

const char* ba_last_error(void) { return g_ba_error.c_str(); }

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Step probe (ba_probe.h): the steps of Solver::run()'s first LM iteration one by one, their results copied out in
// the caller's indexing. Tests only; nothing here launches a kernel or computes.
// ------------------------------------------------------------------------------------------
namespace {

template <typename T>
std::vector<T> probe_fetch(Solver& s, const T* dev, size_t n) {
  std::vector<T> h(n);
  BA_HIP(hipStreamSynchronize(s.st));
  if (n > 0 && dev) BA_HIP(hipMemcpy(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

// a camera-side device vector into the caller's (n_c entries)
void probe_cam_vector(Solver& s, const double* dev, double* out) {
  if (!out || s.V.n_c <= 0) return;
  const std::vector<double> h = probe_fetch(s, dev, (size_t)s.V.n_c);
  std::memcpy(out, h.data(), sizeof(double) * h.size());
}

// a point-side device vector (3 entries at pt_off[j]) into out[3 j ..]
void probe_point_vector(Solver& s, const double* dev, double* out) {
  if (!out || s.V.n_p <= 0) return;
  const std::vector<double> h = probe_fetch(s, dev, (size_t)s.V.n_p);
  for (int j = 0; j < s.prob.num_points; ++j)
    if (s.lay.pt_off[j] >= 0)
      for (int c = 0; c < 3; ++c) out[3 * (size_t)j + c] = h[(size_t)s.lay.pt_off[j] + c];
}

void probe_blocks(Solver& s, const double* dev, double* out, int cap) {
  if (!out || s.lay.moff_total <= 0) return;
  if (s.lay.moff_total > cap) throw std::runtime_error("ba_probe: block_cap too small");
  const std::vector<double> h = probe_fetch(s, dev, (size_t)s.lay.moff_total);
  std::memcpy(out, h.data(), sizeof(double) * h.size());
}

// The stored Jacobian planes (c-order camera side, p-order point side) as one 2 x BA_PROBE_JCOLS block per caller
// observation; `o_of_a` = caller observation of p-order slot a
template <typename JT>
void probe_jacobian(Solver& s, const JT* Jpose, const JT* Jcam, const double* Jsens, const JT* Jpt,
                    const std::vector<int64_t>& o_of_a, const std::vector<int>& a2c, JT* out) {
  if (!out) return;
  const size_t N = (size_t)s.V.n_obs;
  const int kd = s.kd;
  const std::vector<JT> hp = probe_fetch(s, Jpose, 2 * PD * N), hk = probe_fetch(s, Jcam, 2 * (size_t)kd * N),
                        hx = probe_fetch(s, Jpt, 6 * N);
  std::vector<double> hs;
  if (Jsens) hs = probe_fetch(s, Jsens, 12 * N);
  for (size_t a = 0; a < N; ++a) {
    const size_t c = (size_t)a2c[a];
    for (int r = 0; r < 2; ++r) {
      JT* row = out + ((size_t)o_of_a[a] * 2 + r) * BA_PROBE_JCOLS;
      for (int k = 0; k < PD; ++k) row[BA_PROBE_POSE_COL + k] = hp[(size_t)(r * PD + k) * N + c];
      for (int k = 0; k < kd; ++k) row[BA_PROBE_CAM_COL + k] = hk[(size_t)(r * kd + k) * N + c];
      if (Jsens)
        for (int k = 0; k < 6; ++k) row[BA_PROBE_SENS_COL + k] = (JT)hs[(size_t)(r * 6 + k) * N + c];
      for (int k = 0; k < 3; ++k) row[BA_PROBE_PT_COL + k] = hx[(size_t)(r * 3 + k) * N + a];
    }
  }
}

void probe_run(const ba_problem& p_in, const ba_options& opt, ba_probe_io& io) {
  ba_problem p = p_in;  // (the solver holds a reference; write_back() is never called)
  Comm comm;
  Solver s(p, opt, comm);
  ba_result res{};
  io.pcg_iterations = 0; io.pcg_pipelined = -1;
  io.cost = io.s_model = io.s_newcost = 0.0;
  s.keep_obs_maps = true;  // obs_of_a and a2c outlive build()
  const int built = s.build(&res);
  io.n_active = built;
  if (io.obs_active) std::memset(io.obs_active, 0, (size_t)p.num_obs);
  if (built == 0) {
    io.n_c = io.n_p = io.moff_total = 0;
    return;
  }
  const View& V = s.V;
  const int n = V.n_obs, n_c = V.n_c;
  if (n_c > io.vec_stride) throw std::runtime_error("ba_probe: vec_stride too small");
  // ---- path facts
  io.n_c = n_c; io.n_p = V.n_p; io.moff_total = s.lay.moff_total;
  io.width_tier = s.width_tier; io.kd = s.kd; io.bd = s.bd; io.plain_model = s.plain_model;
  io.split_linearize = s.split_linearize ? 1 : 0; io.op32 = s.op32 ? 1 : 0;
  io.n_tiles = V.n_tiles; io.n_chunks = V.n_chunks; io.n_heavy = s.n_heavy; io.pv_n = s.PV.n;
  io.rhs_pass_fused = s.rhs_pass_fused() ? 1 : 0; io.n_priors = s.Q.n; io.n_paired = s.lay.n_paired;
  // ---- maps: the layout's own (host) maps; of the device only its p-order topology is fetched, to check the
  // p-order slot -> caller observation map against it below instead of trusting it
  const ba_layout::Layout& L = s.lay;
  const std::vector<int> a_pose = probe_fetch(s, V.a_pose, (size_t)n), a_cam = probe_fetch(s, V.a_cam, (size_t)n),
                         a_pt = probe_fetch(s, V.a_pt, (size_t)n);
  const std::vector<double> a_xy = probe_fetch(s, V.a_xy, 2 * (size_t)n);
  const std::vector<int64_t>& o_of_a = L.obs_of_a;
  const std::vector<int>& a2c = L.a2c;
  if ((int)o_of_a.size() != n) throw std::runtime_error("ba_probe: active observation count");
  for (int a = 0; a < n; ++a) {
    const int64_t o = o_of_a[a];
    if (a_pose[a] != p.obs_pose[o] || a_cam[a] != p.obs_cam[o] || a_pt[a] != p.obs_point[o] ||
        a_xy[2 * (size_t)a] != p.obs_xy[2 * o] || a_xy[2 * (size_t)a + 1] != p.obs_xy[2 * o + 1])
      throw std::runtime_error("ba_probe: p-order observation map");
    if (io.obs_active) io.obs_active[o] = 1;
  }
  auto moff_of = [&](int blk) { return blk >= 0 ? L.blk_moff[blk] : -1; };
  for (int i = 0; i < p.num_poses; ++i) {
    const int off = L.pose_off[i];
    if (io.pose_off) io.pose_off[i] = off;
    if (io.pose_dim) io.pose_dim[i] = off >= 0 ? L.pose_dim[i] : -1;
    if (io.pose_moff) io.pose_moff[i] = moff_of(L.blk_of_pose[i]);
  }
  for (int k = 0; k < p.num_cams; ++k) {
    const int off = L.cam_off[k];
    if (io.cam_off) io.cam_off[k] = off;
    if (io.cam_dim) io.cam_dim[k] = off >= 0 ? L.cam_dim[k] : -1;
    if (io.cam_moff) io.cam_moff[k] = moff_of(L.blk_of_cam[k]);
  }
  for (int k = 0; k < p.num_sensors; ++k) {
    const int off = L.sens_off[k];
    if (io.sens_off) io.sens_off[k] = off;
    if (io.sens_dim) io.sens_dim[k] = off >= 0 ? 6 : -1;
    if (io.sens_moff) io.sens_moff[k] = moff_of(L.blk_of_sens[k]);
  }
  if (io.pt_off)
    for (int j = 0; j < p.num_points; ++j) io.pt_off[j] = L.pt_off[j];

  // ---- 1. linearisation
  s.set_scales(0);
  s.initial_linearization();
  io.cost = s.scalar(S_COST);
  {
    const std::vector<double> hr = probe_fetch(s, V.res, 2 * (size_t)n), hrp = probe_fetch(s, V.res_p, 2 * (size_t)n);
    for (int a = 0; a < n; ++a)
      for (int r = 0; r < 2; ++r) {
        if (io.res) io.res[2 * o_of_a[a] + r] = hr[(size_t)r * n + a2c[a]];
        if (io.res_p) io.res_p[2 * o_of_a[a] + r] = hrp[(size_t)r * n + a];
      }
  }
  probe_jacobian<double>(s, V.Jpose, V.Jcam, V.sens_off ? V.Jsens : nullptr, V.Jpt, o_of_a, a2c, io.J);
  if (s.op32) probe_jacobian<float>(s, V.Jpose32, V.Jcam32, nullptr, V.Jpt32, o_of_a, a2c, io.J32);
  probe_cam_vector(s, s.gc.p, io.gc); probe_cam_vector(s, s.diag_c.p, io.diag_c); probe_cam_vector(s, s.scale_c.p, io.scale_c);
  probe_point_vector(s, s.gp.p, io.gp); probe_point_vector(s, s.diag_p.p, io.diag_p); probe_point_vector(s, s.scale_p.p, io.scale_p);
  if (io.Craw) {
    const std::vector<double> h = probe_fetch(s, s.Craw.p, 6 * (size_t)p.num_points);
    for (int j = 0; j < p.num_points; ++j)
      for (int e = 0; e < 6; ++e) io.Craw[6 * (size_t)j + e] = h[(size_t)e * p.num_points + j];
  }

  // ---- 2. the damped system
  s.damp(io.radius);
  probe_cam_vector(s, s.Dc.p, io.Dc);
  probe_point_vector(s, s.Dp.p, io.Dp);
  if (io.Cinv) {
    const std::vector<double> h = probe_fetch(s, s.Cinv.p, 9 * (size_t)p.num_points);
    for (int j = 0; j < p.num_points; ++j)
      if (s.lay.pt_off[j] >= 0) std::memcpy(io.Cinv + 9 * (size_t)j, h.data() + 9 * (size_t)j, 9 * sizeof(double));
  }
  if (n_c > 0) {
    s.form_preconditioner();
    probe_blocks(s, s.M.p, io.M, io.block_cap);
    probe_blocks(s, s.Minv.p, io.Minv, io.block_cap);
    s.reduced_rhs();
    probe_cam_vector(s, s.rhs.p, io.rhs);
    // ---- 3. products with the caller's vectors (s.pdir / s.q as staging: pcg() initialises both)
    for (int inexact = 0; inexact < 2; ++inexact)
      for (int i = 0; i < io.num_vectors; ++i) {
        BA_HIP(hipStreamSynchronize(s.st));
        BA_HIP(hipMemcpy(s.pdir.p, io.x_in + (size_t)i * io.vec_stride, sizeof(double) * n_c, hipMemcpyHostToDevice));
        s.schur_multiply(s.pdir.p, s.q.p, inexact != 0);
        if (io.q_out) probe_cam_vector(s, s.q.p, io.q_out + ((size_t)inexact * io.num_vectors + i) * io.vec_stride);
      }
    // ---- 4. the linear solve
    const long long pipelined_before = g_pcg_pipelined_solves, stepwise_before = g_pcg_stepwise_solves;
    io.pcg_iterations = s.pcg(opt.max_linear_solver_iterations, opt.eta);
    io.pcg_pipelined = g_pcg_pipelined_solves > pipelined_before ? 1 : (g_pcg_stepwise_solves > stepwise_before ? 0 : -1);
    probe_cam_vector(s, s.x.p, io.x);
  }
  // ---- 5. the step
  s.back_substitute_and_model_change();
  s.evaluate_candidate();
  {
    double h[NSCALAR];
    s.scalars_to_host(h);
    io.s_model = h[S_MODEL];
    io.s_newcost = h[S_NEWCOST];
  }
  probe_point_vector(s, s.dp.p, io.dp);
  auto fetch_to = [&](const double* dev, size_t count, double* out) {
    if (!out || count == 0) return;
    const std::vector<double> h = probe_fetch(s, dev, count);
    std::memcpy(out, h.data(), sizeof(double) * count);
  };
  fetch_to(s.poses2.p, 7 * (size_t)p.num_poses, io.cand_poses);
  fetch_to(s.cams2.p, BA_CAM_STRIDE * (size_t)p.num_cams, io.cand_cams);
  fetch_to(s.points2.p, 3 * (size_t)p.num_points, io.cand_points);
  if (V.sensors) fetch_to(s.sensors2.p, 7 * (size_t)p.num_sensors, io.cand_sensors);
}

}  // namespace

extern "C" int ba_probe_steps(const ba_problem* problem, const ba_options* options, int32_t gpu_index, ba_probe_io* io) {
  try {
    if (!problem || !options || !io) throw std::runtime_error("null argument");
    select_device(gpu_index);
    probe_run(*problem, *options, *io);
    return 0;
  } catch (const std::exception& e) {
    g_ba_error = e.what();
    return 1;
  }
}
