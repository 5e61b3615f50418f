/*
 * colmap_amd_tvg.h -- C ABI of two-view geometry estimation: geometric verification of the matches of image pairs by a
 * fundamental matrix and a homography (`colmap geometric_verifier`, reference exe/feature.cc and
 * controllers/feature_matching_utils.cc:595-662).
 *
 * Replaces, for matched points that are already in memory as flat arrays (reference src/colmap):
 *   estimators/two_view_geometry.cc:552-640    EstimateTwoViewGeometry, the router            tvg_route, tvg_verify_pairs
 *   estimators/two_view_geometry.cc:245-337    EstimateUncalibratedTwoViewGeometry            tvg_verify_pairs
 *   estimators/two_view_geometry.cc:180-243    EstimateCalibratedHomography (force_H_use)     tvg_verify_pairs
 *   estimators/two_view_geometry.cc:339-382    EstimateMultipleTwoViewGeometries              tvg_verify_pairs
 *   estimators/two_view_geometry.cc:1503-1584  DetectWatermarkMatches, FilterStationaryMatches tvg_verify_pairs
 *   optim/loransac.h:131-393                   LORANSAC::Estimate with InlierSupportMeasurer  tvg_estimate
 *   optim/ransac.h:167-210                     the clamp of max_num_trials, ComputeNumTrials  tvg_estimate
 *   estimators/solvers/fundamental_matrix.cc:47-114, homography_matrix.cc:45-96 (4 points),
 *   solvers/translation_transform.h            the minimal solvers                            tvg_hypothesize
 *   geometry/essential_matrix.cc:168-182, homography_matrix.cc:98-135, translation_transform.h:104-118
 *                                              the residuals and InlierSupportMeasurer::Evaluate  tvg_score
 * The reference runs one pair per CPU thread. Here every (pair, trial, match) triple is evaluated on the GPU: a batch
 * of point sets lives on the device, one lane solves one minimal sample, one lane scores one model against the matches
 * of its set. The sequential rules of the search stay on the host (colmap_amd/csrc/two_view_plan.h) and give the same
 * report for every batch composition and every number of trials per round. There is no CPU path.
 *
 * NOT built: the routes that need an essential matrix or a focal solver (calibrated, shared focal, one-sided focal,
 * spherical, rigs), use_degensac, compute_relative_pose, guided verification. tvg_verify_pairs names the route of
 * every pair and leaves the pairs of an unbuilt route without a result (config TVG_CONFIG_NOT_BUILT).
 *
 * A model crosses this interface as 9 doubles: F and H row-major, a translation in the first two.
 * A sample is a pure function of (random_seed, stream_id, kind, trial), see two_view_solvers.h; random_seed -1 is
 * treated as 0, so results are always reproducible.
 */
#ifndef COLMAP_AMD_TVG_H_
#define COLMAP_AMD_TVG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { TVG_KIND_F = 0, TVG_KIND_H = 1, TVG_KIND_T = 2 };
enum { TVG_MAX_MODELS = 3 }; /* models of one minimal sample */

/* TwoViewGeometry::ConfigurationType (scene/two_view_geometry.h:44-67); NOT_BUILT is not a value of the reference */
enum {
  TVG_CONFIG_UNDEFINED = 0,
  TVG_CONFIG_DEGENERATE = 1,
  TVG_CONFIG_CALIBRATED = 2,
  TVG_CONFIG_UNCALIBRATED = 3,
  TVG_CONFIG_PLANAR = 4,
  TVG_CONFIG_PANORAMIC = 5,
  TVG_CONFIG_PLANAR_OR_PANORAMIC = 6,
  TVG_CONFIG_WATERMARK = 7,
  TVG_CONFIG_MULTIPLE = 8,
  TVG_CONFIG_NOT_BUILT = -1
};

/* the branches of EstimateTwoViewGeometry (two_view_geometry.cc:552-640), in its order */
enum {
  TVG_ROUTE_FORCED_H_DEGENERATE = 0, /* force_H_use with a non-pinhole camera: DEGENERATE (:577-585) */
  TVG_ROUTE_FORCED_H = 1,            /* EstimateCalibratedHomography (:586) */
  TVG_ROUTE_ONE_SIDED_FOCAL = 2,     /* not built (:589-598) */
  TVG_ROUTE_SPHERICAL = 3,           /* not built (:599-603) */
  TVG_ROUTE_SHARED_FOCAL = 4,        /* not built (:604-612) */
  TVG_ROUTE_CALIBRATED = 5,          /* not built (:613-617) */
  TVG_ROUTE_FISHEYE_DEGENERATE = 6,  /* perspective fisheye without a focal prior: DEGENERATE (:618-633) */
  TVG_ROUTE_UNCALIBRATED = 7,        /* EstimateUncalibratedTwoViewGeometry (:634-638) */
  TVG_NUM_ROUTES = 8
};

/* what the router reads of a colmap::Camera */
typedef struct tvg_camera {
  int32_t model_id; /* colmap::CameraModelId */
  int32_t width, height;
  int32_t camera_id;
  int32_t has_prior_focal_length;
} tvg_camera;

/* colmap::RANSACOptions (optim/ransac.h:50-83) */
typedef struct tvg_ransac_options {
  double max_error;
  double min_inlier_ratio;
  double confidence;
  double dyn_num_trials_multiplier;
  int32_t min_num_trials;
  int32_t max_num_trials;
  int32_t random_seed;      /* -1 is treated as 0 */
  int32_t trials_per_round; /* trials of a set hypothesized and scored per round; 0: tvg_trial_round(). The report
                               does not depend on it */
} tvg_ransac_options;

/* colmap::TwoViewGeometryOptions (estimators/two_view_geometry.h:44-131), the options of the built routes */
typedef struct tvg_options {
  tvg_ransac_options ransac;
  int32_t min_num_inliers;
  int32_t detect_watermark;
  int32_t multiple_ignore_watermark;
  int32_t filter_stationary_matches;
  int32_t force_H_use;
  int32_t multiple_models;
  double max_H_inlier_ratio;
  double watermark_min_inlier_ratio;
  double watermark_border_size;
  double watermark_detection_max_error;
  double stationary_matches_max_error;
} tvg_options;

/* LORANSAC::Report of one point set */
typedef struct tvg_report {
  int32_t success;
  int32_t has_model;     /* a best model exists (the reference stores it even without success) */
  int64_t num_trials;    /* the reference's trial counter: stopping trial + 1, or max_num_trials + 1 when exhausted */
  int64_t num_inliers;
  double residual_sum;   /* of the inliers; DBL_MAX while no model has been scored */
  double model[9];
  uint8_t* inlier_mask;  /* in: null or room for the set's matches; out: residual <= max_error^2 of the winner */
  int64_t num_scored;    /* models scored on the device for this set, including what lay past the stopping trial */
  int64_t num_launches;  /* scoring launches the set took part in */
} tvg_report;

typedef struct tvg_handle tvg_handle;

void tvg_ransac_options_init(tvg_ransac_options* options); /* the constructor of TwoViewGeometryOptions (:122-128) */
void tvg_options_init(tvg_options* options);

int tvg_create(int32_t gpu_index, tvg_handle** handle);
void tvg_destroy(tvg_handle* handle);

/* Uploads a batch of point sets; it replaces the handle's previous batch. Set s holds the matches
 * [set_offsets[s], set_offsets[s + 1]) of `points` ([.][4]: x1 y1 x2 y2); on the device every set is stored SoA and
 * padded to whole waves. stream_ids[s] is the caller's 64-bit key of the set: its samples depend on nothing else. */
int tvg_set_points(tvg_handle* handle, int32_t num_sets, const int64_t* set_offsets, const double* points,
                   const uint64_t* stream_ids);

/* One lane per trial draws its sample and solves it. Item i asks for the trials [item_first_trial[i],
 * item_first_trial[i] + item_num_trials[i]) of set item_set[i] (which must hold at least the kind's minimal sample);
 * the outputs run over all trials of all items in item order: num_models [.], models [.][3][9], samples [.][7]
 * (nullable). */
int tvg_hypothesize(tvg_handle* handle, int32_t kind, int32_t random_seed, int32_t num_items, const int32_t* item_set,
                    const int64_t* item_first_trial, const int32_t* item_num_trials, int32_t* num_models, double* models,
                    uint32_t* samples);

/* Scores model m ([9]) against the matches of set model_set[m]: InlierSupportMeasurer::Evaluate with
 * max_residual = max_error^2. inlier_masks (nullable) receives the masks one after the other, each as long as its
 * set. The bits of residual_sum depend on the set and the model alone: one accumulator walks the matches in order. */
int tvg_score(tvg_handle* handle, int32_t kind, double max_error, int32_t num_models, const int32_t* model_set,
              const double* models, int64_t* num_inliers, double* residual_sum, uint8_t* inlier_masks);

/* LORANSAC of one kind over all sets of the handle at once. min_inlier_ratios (nullable): a ratio per set that
 * replaces options->min_inlier_ratio (the homography search of two_view_geometry.cc:283-287). reports: [num_sets]. */
int tvg_estimate(tvg_handle* handle, int32_t kind, const tvg_ransac_options* options, const double* min_inlier_ratios,
                 tvg_report* reports);

/* EstimateTwoViewGeometry for a batch of pairs. Pair p holds the matches [match_offsets[p], match_offsets[p + 1]) of
 * `points`. Outputs per pair: route (TVG_ROUTE_*), config (TVG_CONFIG_*), has_F / F [.][9], has_H / H [.][9];
 * inlier_mask runs over all matches. stats (nullable, [2]): models scored, scoring launches. */
int tvg_verify_pairs(tvg_handle* handle, const tvg_options* options, int32_t num_pairs, const tvg_camera* cameras1,
                     const tvg_camera* cameras2, const int64_t* match_offsets, const double* points,
                     const uint64_t* stream_ids, int32_t* route, int32_t* config, int32_t* has_F, double* F,
                     int32_t* has_H, double* H, uint8_t* inlier_mask, int64_t* stats);

/* host functions */
int tvg_route(const tvg_camera* camera1, const tvg_camera* camera2, const tvg_options* options);
const char* tvg_route_name(int32_t route);
int tvg_route_is_built(int32_t route);
int tvg_draw_sample(int32_t random_seed, uint64_t stream_id, int32_t kind, uint64_t trial, uint32_t num_points,
                    uint32_t sample[7]);

int tvg_model_tile(void);  /* models one workgroup of the scorer walks, one per lane */
int tvg_match_tile(void);  /* matches of one LDS tile of the scorer */
int tvg_trial_round(void); /* default trials of a set per round */

void tvg_last_timing(double* kernel_ms, double* total_ms);
const char* tvg_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* COLMAP_AMD_TVG_H_ */
