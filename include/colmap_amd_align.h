/*
 * colmap_amd_align.h -- C ABI of model alignment: putting two sparse models (or a model and a list of positions) into
 * one frame by a robustly estimated similarity, and applying a similarity to points (`colmap model_aligner`,
 * `model_comparer`, `model_transformer`, reference exe/model.cc:257-424, 520-631, 1081-1129).
 *
 * Replaces, for data that is already in memory as flat arrays (reference src/colmap):
 *   estimators/alignment.cc:43-181      ReconstructionAlignmentEstimator (Estimate, Residuals)
 *   estimators/alignment.cc:301-342     AlignReconstructionsViaReprojections
 *   estimators/alignment.cc:185-238     AlignReconstructionToLocations (its EstimateSim3dRobust)
 *   estimators/alignment.cc:400-458     AlignReconstructionsViaPoints (its EstimateSim3dRobust)
 *   optim/loransac.h:131-393            LORANSAC::Estimate with InlierSupportMeasurer
 *   optim/ransac.h:167-210              the clamp of max_num_trials and ComputeNumTrials
 *   scene/reconstruction.cc:788-805     Reconstruction::Transform, the points
 * The reference scores one hypothesis after the other on one thread. Every (hypothesis, observation) pair is
 * independent, so a batch of hypotheses is scored against all observations in one launch; the search loop itself
 * (colmap_amd/csrc/align_plan.h) keeps the sequential rules and gives the same report for every batch size. All
 * geometry is double precision, counts are integers, sums run in an order that depends on the data size alone, and
 * there is no CPU path.
 *
 * A Sim3 crosses this interface as 8 doubles in the order of Sim3d::ToFile (geometry/sim3.cc:39-48):
 * scale, qw qx qy qz, tx ty tz; it maps x to scale * (R x) + t.
 */
#ifndef COLMAP_AMD_ALIGN_H_
#define COLMAP_AMD_ALIGN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ALIGN_HYPOTHESIS_TILE: hypotheses one workgroup of a scoring kernel walks with its observations in registers. */
enum { ALIGN_MAX_BATCH = 1024, ALIGN_HYPOTHESIS_TILE = 16 };

/* colmap::Camera (scene/camera.h): model_id is colmap::CameraModelId (sensor/models.h:90-111), num_params the length
 * the caller filled (checked against the model). */
typedef struct align_camera {
  int32_t model_id;
  int32_t width, height;
  int32_t num_params;
  double params[16];
} align_camera;

/* The common registered images of two models (FindCommonRegImageIds) and their common observations: one record per
 * point2D_idx at which BOTH images carry a 3D point (alignment.cc:125-139). The two cameras of an image slot may be
 * of different models. */
typedef struct align_reproj_pair {
  int32_t num_images;               /* common images: the samples of the search */
  int32_t reserved;
  int64_t num_records;
  const align_camera* src_cameras;  /* [num_images] camera of the image in the src model */
  const align_camera* tgt_cameras;  /* [num_images] */
  const double* src_poses;          /* [num_images][7] cam_from_world: qx qy qz qw tx ty tz */
  const double* tgt_poses;          /* [num_images][7] */
  const int32_t* src_num_points2D;  /* [num_images] Image::NumPoints2D, checked to agree (alignment.cc:120) */
  const int32_t* tgt_num_points2D;  /* [num_images] */
  const int32_t* rec_image;         /* [num_records] image slot */
  const double* rec_src_xyz;        /* [num_records][3] the 3D point of the src model's observation */
  const double* rec_tgt_xyz;        /* [num_records][3] */
  const double* rec_src_xy;         /* [num_records][2] measured pixel in the src model */
  const double* rec_tgt_xy;         /* [num_records][2] */
} align_reproj_pair;

/* colmap::RANSACOptions (optim/ransac.h:50-83) and the two thresholds of the reprojection alignment. */
typedef struct align_options {
  double max_error;               /* reprojection: max_reproj_error in pixels (8); positions: max_error */
  double min_inlier_observations; /* reprojection only (0.3): an image is an inlier when at least this share of its
                                     common observations reprojects within max_error both ways */
  double min_inlier_ratio;        /* 0.1; AlignReconstructionsViaReprojections sets 0.2 (alignment.cc:312) */
  double confidence;              /* 0.99 */
  double dyn_num_trials_multiplier; /* 3.0 */
  int32_t min_num_trials;         /* 0 */
  int32_t max_num_trials;         /* INT32_MAX */
  int32_t random_seed;            /* 0; the sample stream is a fixed 64-bit LCG (align_plan.h) */
  int32_t batch_size;             /* hypotheses per launch; 0 = the default. The report does not depend on it. */
} align_options;

/* LORANSAC's Report. inlier_mask is caller-owned, one byte per sample (image slot / point), or null. */
typedef struct align_report {
  int32_t success;
  int32_t reserved;
  int64_t num_trials;
  int64_t num_inliers;   /* support.num_inliers */
  double residual_sum;   /* support.residual_sum; DBL_MAX while no sample has given a model */
  double model[8];       /* tgt_from_src */
  uint8_t* inlier_mask;
  int64_t num_scored;    /* hypotheses scored on the device, those past the stopping trial included */
  int64_t num_launches;
} align_report;

typedef struct align_handle align_handle;

/* RANSACOptions' defaults with max_error = 8, min_inlier_observations = 0.3 (model_comparer, exe/model.cc:525-527). */
void align_options_init(align_options* options);

/* Checks and uploads a model pair once (ReconstructionAlignmentEstimator's constructor). 0 = ok. */
int align_reproj_create(const align_reproj_pair* pair, int32_t gpu_index, align_handle** handle);

/* ReconstructionAlignmentEstimator::Residuals (alignment.cc:94-175) of num_hypotheses models in one launch:
 * inliers[h][i] = observations of image slot i that reproject within max_reproj_error in both directions under
 * hypothesis h; common[i] = observations of slot i (either output may be null). A count does not depend on
 * num_hypotheses or on the position of its hypothesis. 0 = ok. */
int align_reproj_score(align_handle* handle, const double* tgt_from_src, int32_t num_hypotheses, double max_reproj_error,
                       uint32_t* inliers, uint32_t* common);

/* AlignReconstructionsViaReprojections (alignment.cc:301-342): LORANSAC over three-image hypotheses, each the similarity
 * of the three pairs of projection centres. options->min_inlier_ratio is used as given (the reference's caller sets 0.2).
 * Fewer than 3 common images: success = 0, num_trials = 0. 0 = ok (also when success = 0). */
int align_reproj_estimate(align_handle* handle, const align_options* options, align_report* report);

/* Uploads two point sets of equal length (EstimateSim3dRobust's src and tgt). 0 = ok. */
int align_positions_create(const double* src, const double* tgt, int64_t num_points, int32_t gpu_index, align_handle** handle);

/* SimilarityTransformEstimator::Residuals + InlierSupportMeasurer::Evaluate (solvers/similarity_transform.cc,
 * optim/support_measurement.cc:36-51) of num_hypotheses models in one launch: num_inliers[h] and residual_sum[h] over
 * the points with |tgt - (s R src + t)|^2 <= max_error^2. inlier_mask: [num_hypotheses][num_points] bytes or null.
 * The bits of residual_sum[h] do not depend on num_hypotheses or on h. 0 = ok. */
int align_positions_score(align_handle* handle, const double* tgt_from_src, int32_t num_hypotheses, double max_error,
                          int64_t* num_inliers, double* residual_sum, uint8_t* inlier_mask);

/* EstimateSim3dRobust (LORANSAC over three-point similarity hypotheses) on the uploaded point sets. 0 = ok. */
int align_positions_estimate(align_handle* handle, const align_options* options, align_report* report);

void align_destroy(align_handle* handle);

/* ALIGN_HYPOTHESIS_TILE of the loaded library. */
int align_hypothesis_tile(void);

/* new_from_old * X for every row of points[num_points][3], in place: X' = scale * (R X) + t, the point loop of
 * Reconstruction::Transform (scene/reconstruction.cc:788-805). 0 = ok. */
int align_transform_points(double* points, int64_t num_points, const double new_from_old[8], int32_t gpu_index);

/* Where the time of the last call of this thread went: its kernels (HIP events, summed over the launches of a search),
 * and the whole call including the host plan, the copies and the host side of the search. */
void align_last_timing(double* kernel_ms, double* total_ms);

const char* align_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_ALIGN_H_ */
