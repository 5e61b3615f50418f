/*
 * colmap_amd_ba_covariance.h -- C ABI of the covariance estimation that follows a bundle-adjustment solve.
 *
 * Counterpart of colmap::EstimateBACovariance / BACovariance (reference src/colmap/estimators/covariance.h),
 * for the flattened problem of colmap_amd_ba.h instead of a ceres::Problem. The covariance is evaluated at
 * the current parameter values of the problem, with its variable / constant blocks, SubsetManifold tangent
 * sizes, loss function (corrected Jacobian, as ceres::Problem::Evaluate applies it) and position priors:
 *   points:           cov_p = (E_p^T E_p + damping I)^-1, conditioned on every other block held fixed;
 *   poses and others: S = H_aa - H_ap H_pp^-1 H_pa over the poses and the "other" blocks (variable intrinsics,
 *                     variable sensor_from_rig), the point blocks damped as above. BA_COV_ALL returns blocks of
 *                     S^-1; BA_COV_POSES / BA_COV_POSES_AND_POINTS first eliminate the others,
 *                     S <- S_cc - S_co (S_oo + damping I)^-1 S_oc, and return pose blocks of its inverse.
 * Tangent coordinates as the LM loop uses them: [rotation, translation] for a pose (left-perturbation
 * quaternion manifold), the variable entries of an intrinsics block in parameter order; constant dimensions
 * are omitted. S is formed, factored and inverted on the GPU (colmap_amd/csrc/ba_schur_explicit.hip); the handle
 * keeps L^-1 in device memory, so block queries are GPU launches. The problem's arrays are only read.
 *
 * Returns BA_COV_OK, BA_COV_NOT_ESTIMABLE (the reduced matrix is rank deficient: ba_last_error() states the
 * number of columns and the rank), or BA_COV_ERROR (ba_last_error() holds the message). No CPU fallback.
 */
#ifndef COLMAP_AMD_BA_COVARIANCE_H_
#define COLMAP_AMD_BA_COVARIANCE_H_

#include "colmap_amd_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* BACovarianceOptions::Params (covariance.h) */
enum { BA_COV_POSES = 0, BA_COV_POINTS = 1, BA_COV_POSES_AND_POINTS = 2, BA_COV_ALL = 3 };
/* status codes */
enum { BA_COV_OK = 0, BA_COV_ERROR = 1, BA_COV_NOT_ESTIMABLE = 2, BA_COV_NO_RESULT = 3 };
/* block kinds of a query */
enum { BA_COV_KIND_POSE = 0, BA_COV_KIND_CAMERA = 1, BA_COV_KIND_SENSOR = 2 };

typedef struct ba_covariance_options {
  int32_t params;  /* BA_COV_ALL */
  double damping;  /* 1e-8 */
} ba_covariance_options;

void ba_covariance_options_init(ba_covariance_options* options);

typedef struct ba_covariance ba_covariance; /* opaque; owns device memory until ba_covariance_destroy */

/* options: loss_type / loss_scale and jacobi_scaling are read (the rest of ba_options is ignored).
 * gpu_index: device ordinal, -1 = current. Camera-side dimension limit: 32 768 (the exact tier's). */
int ba_estimate_covariance(const ba_problem* problem, const ba_options* options, const ba_covariance_options* cov_options,
                           int32_t gpu_index, ba_covariance** out);

/* Tangent dimension of a block (kind, index into the problem's poses / cams / sensors) in the result:
 * *dim = 0 when the block is not a variable block of the estimate (BA_COV_NO_RESULT). */
int ba_covariance_block_dim(const ba_covariance* cov, int32_t kind, int32_t index, int32_t* dim);
/* 3 x 3 covariance of point `index` (row-major), or BA_COV_NO_RESULT. */
int ba_covariance_point(const ba_covariance* cov, int32_t index, double out[9]);

typedef struct ba_covariance_pair {
  int32_t kind_a, index_a, kind_b, index_b;
} ba_covariance_pair;
#define BA_COV_SLOT 256 /* doubles per result of ba_covariance_blocks (the widest block has 16 dimensions) */
/* Batched block query, one GPU launch: for pair k, out[k * BA_COV_SLOT ...] receives the row-major
 * dim_a x dim_b cross covariance of the two blocks and found[k] = 1; found[k] = 0 when either block has no
 * result. */
int ba_covariance_blocks(ba_covariance* cov, int32_t count, const ba_covariance_pair* pairs, double* out, int32_t* found);

/* HIP-event times of the estimate (formation of S, factorisation, triangular inverse) and of the last
 * ba_covariance_blocks launch, in milliseconds; n = dimension of the factored matrix (others padded to a
 * multiple of 64, then poses), n_inv = rows / columns of the part that was inverted. */
int ba_covariance_timing(const ba_covariance* cov, double* form_ms, double* factor_ms, double* inverse_ms,
                         double* extract_ms, int32_t* n, int32_t* n_inv);

void ba_covariance_destroy(ba_covariance* cov);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_BA_COVARIANCE_H_ */
