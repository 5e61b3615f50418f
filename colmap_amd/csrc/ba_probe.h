// Step probe of the iterative tier (INTERNAL: not under include/, not part of the public ABI; the tests' counterpart of
// ba_schur_explicit.h for ba_kernels.hip, defined at the end of that file).
//
// ba_probe_steps() builds a Solver for one GPU (world = 1) and calls its EXISTING step functions in the order
// Solver::run() uses for its first LM iteration:
//   build, set_scales(0), initial_linearization;
//   damp(radius), form_preconditioner, reduced_rhs;                  (the last two only when n_c > 0, as in run())
//   schur_multiply(x_i, q_i, inexact) for every supplied vector, inexact = false, then true;
//   pcg(max_linear_solver_iterations, eta);
//   back_substitute_and_model_change, evaluate_candidate.
// After each group it copies what the step left on the device into the caller's arrays. It launches nothing of its
// own and does no arithmetic: it copies, reads fields and re-indexes on the host. The problem is never written to.
//
// Everything is returned IN THE CALLER'S INDEXING: per caller pose / camera / sensor / point / observation. Arrays
// the caller does not want may be null. Capacities (the caller knows them without knowing the layout):
//   camera-side vectors   vec_stride doubles each, vec_stride >= 6 num_poses + 16 num_cams + 6 num_sensors
//   point-side vectors    3 num_points (entry 3 j + c of caller point j; a constant or unused point keeps its input)
//   M, Minv               block_cap doubles, block_cap >= 36 num_poses + 256 num_cams + 36 num_sensors
//   J, J32                num_obs x 2 x BA_PROBE_JCOLS, row-major: columns [0, 6) pose tangent (the first pose_dim are
//                         used), [6, 22) intrinsics tangent (cam_dim: the variable parameters in ascending order),
//                         [22, 28) sensor_from_rig tangent, [28, 31) point. Column-scaled as stored. Inactive
//                         observations and unused columns are zero.
//   res                   num_obs x 2 (loss-corrected)
//   Craw                  num_points x 6 (xx xy xz yy yz zz), Cinv num_points x 9
// M / Minv of a block: dim x dim row-major at its *_moff.
#pragma once
#include <stdint.h>

#include "../../include/colmap_amd_ba.h"

#define BA_PROBE_JCOLS 31
#define BA_PROBE_POSE_COL 0
#define BA_PROBE_CAM_COL 6
#define BA_PROBE_SENS_COL 22
#define BA_PROBE_PT_COL 28

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ba_probe_io {
  // ---- in
  double radius;          // trust-region radius of damp()
  int32_t num_vectors;    // k camera-side vectors for schur_multiply
  int32_t vec_stride;     // capacity of every camera-side vector below (and the stride of x_in / q_out)
  int32_t block_cap;      // capacity of M / Minv
  int32_t reserved_;
  const double* x_in;     // [k][vec_stride]: the first n_c entries of each are used
  // ---- maps (-1: not variable / not used)
  int32_t *pose_off, *pose_dim, *pose_moff;  // [num_poses]
  int32_t *cam_off, *cam_dim, *cam_moff;     // [num_cams]
  int32_t *sens_off, *sens_dim, *sens_moff;  // [num_sensors]
  int32_t* pt_off;                           // [num_points]
  uint8_t* obs_active;                       // [num_obs]
  // ---- linearisation (after initial_linearization)
  double cost;
  double* res;
  double* res_p;        // the p-order copy of the same residuals (what the point-side kernels read)
  double* J;
  float* J32;             // filled only when op32
  // ---- vectors
  double *gc, *diag_c, *scale_c, *Dc;  // camera side
  double *gp, *diag_p, *scale_p, *Dp;  // point side
  // ---- blocks
  double *Craw, *Cinv, *M, *Minv;
  // ---- right-hand side and products
  double* rhs;
  double* q_out;          // [2][k][vec_stride]: inexact = false, then true
  // ---- solve
  double* x;
  int32_t pcg_iterations;
  int32_t pcg_pipelined;  // 1: pcg() took the pipelined loop, 0: the step-by-step loop, -1: pcg() did not run
  double* dp;
  double s_model, s_newcost;
  double *cand_poses, *cand_cams, *cand_points, *cand_sensors;  // [num_poses][7], [num_cams][BA_CAM_STRIDE], [num_points][3], [num_sensors][7]
  // ---- path facts
  int32_t n_c, n_p, n_active, moff_total;
  int32_t width_tier, kd, bd, plain_model, split_linearize, op32;
  int32_t n_tiles, n_chunks, n_heavy, pv_n, rhs_pass_fused, n_priors;
  int64_t n_paired;
} ba_probe_io;

// 0: ok; 1: an exception was caught (ba_last_error() has its text)
int ba_probe_steps(const ba_problem* problem, const ba_options* options, int32_t gpu_index, ba_probe_io* io);

#ifdef __cplusplus
}
#endif
