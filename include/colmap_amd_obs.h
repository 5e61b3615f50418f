/*
 * colmap_amd_obs.h -- C ABI of observation and point filtering on a sparse model: the outlier removal that sits between
 * two bundle adjustments and before undistortion (`colmap point_filtering`, reference exe/sfm.cc:556-587).
 *
 * Replaces, for a model that is already in memory as flat arrays (reference src/colmap):
 *   sfm/observation_manager.cc:381-393  ObservationManager::FilterAllPoints3D / FilterPoints3D
 *   sfm/observation_manager.cc:496-585  FilterPoints3DWithLargeReprojectionError
 *   sfm/observation_manager.cc:435-494  FilterPoints3DWithSmallTriangulationAngle
 *   sfm/observation_manager.cc:395-407  FilterPoints3DWithShortTracks
 *   sfm/observation_manager.cc:409-433  FilterObservationsWithNegativeDepth
 *   scene/reconstruction.cc:959-975     Reconstruction::UpdatePoint3DErrors
 * The reference walks points and observations one after the other and deletes as it goes. Every point is independent
 * of every other, so each rule has a closed per-point form (colmap_amd/csrc/obs_filter.hip states them); the calls
 * below DECIDE -- one keep byte per observation, one status byte per point -- and the caller applies the deletions
 * (colmap_amd/observation_manager.py, include/colmap_amd/observation_manager.hpp). Everything is computed on the GPU
 * in double precision; there is no CPU path.
 */
#ifndef COLMAP_AMD_OBS_H_
#define COLMAP_AMD_OBS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* colmap::ReprojectionErrorType (sfm/observation_manager.h): the unit of max_reproj_error. */
enum { OBS_ERROR_PIXEL = 0, OBS_ERROR_NORMALIZED = 1, OBS_ERROR_ANGULAR = 2 };

/* The rules obs_filter_all_points3D applies, in the reference's order "errors, then angles". */
enum { OBS_RULE_REPROJ_ERROR = 1, OBS_RULE_TRI_ANGLE = 2 };

/* Status byte of a point. */
enum {
  OBS_POINT_KEPT = 0,
  OBS_POINT_DELETED_ERROR = 1, /* track shorter than 2, or all but at most one observation above max_reproj_error */
  OBS_POINT_DELETED_ANGLE = 2, /* no pair of images with a triangulation angle of min_tri_angle or more */
  OBS_POINT_DELETED_SHORT = 3, /* track shorter than min_track_len */
  OBS_POINT_DELETED_DEPTH = 4  /* removing its negative-depth observations leaves fewer than 2 */
};

typedef struct obs_filter_options {
  double max_reproj_error; /* 4.0; pixels, normalized units or degrees according to error_type */
  double min_tri_angle;    /* 1.5 degrees */
  int32_t min_track_len;   /* 2 */
  int32_t error_type;      /* OBS_ERROR_PIXEL */
  int32_t rules;           /* OBS_RULE_REPROJ_ERROR | OBS_RULE_TRI_ANGLE */
  int32_t reserved;
} obs_filter_options;

/* colmap::Camera (scene/camera.h): model_id is colmap::CameraModelId (sensor/models.h:90-111), num_params the length
 * the caller filled (checked against the model). */
typedef struct obs_camera {
  int32_t model_id;
  int32_t width, height;
  int32_t num_params;
  double params[16];
} obs_camera;

/* A sparse model as flat arrays. Observations are in CSR by point: the observations of point p are
 * obs_offsets[p] .. obs_offsets[p + 1] - 1, in the order of its track. */
typedef struct obs_model {
  int32_t num_cameras;
  int32_t num_images;
  int64_t num_points;
  int64_t num_observations;
  const obs_camera* cameras;   /* [num_cameras] */
  const double* image_poses;   /* [num_images][7] cam_from_world: qx qy qz qw tx ty tz */
  const int32_t* image_camera; /* [num_images] index into cameras */
  const double* points;        /* [num_points][3] */
  const int64_t* obs_offsets;  /* [num_points + 1] */
  const int32_t* obs_image;    /* [num_observations] index into the images */
  const double* obs_xy;        /* [num_observations][2] measured pixel */
} obs_model;

/* Caller-owned outputs; a null pointer skips that output. */
typedef struct obs_result {
  uint8_t* obs_keep;      /* [num_observations] 1 = the observation stays in its track, 0 = it is deleted */
  uint8_t* point_status;  /* [num_points] OBS_POINT_* */
  double* point_error;    /* [num_points] the error the rule assigns to a kept point, -1 where it assigns none */
  uint32_t* point_count;  /* [num_points] filtered observations of the point, as the reference counts them */
  int64_t num_filtered;   /* out: sum of point_count, in point order */
} obs_result;

/* The defaults of `colmap point_filtering` (exe/sfm.cc:561-563) and ReprojectionErrorType::PIXEL. */
void obs_filter_options_init(obs_filter_options* options);

/* ObservationManager::FilterAllPoints3D / FilterPoints3D over the points of `model` (a subset of a reconstruction is a
 * model with fewer points): FilterPoints3DWithLargeReprojectionError(max_reproj_error, error_type), then
 * FilterPoints3DWithSmallTriangulationAngle(min_tri_angle) on what survives. options->rules selects one rule alone.
 * point_error: error_sum / (track length after the deletions) for a point the error rule keeps. 0 = ok. */
int obs_filter_all_points3D(const obs_model* model, const obs_filter_options* options, obs_result* result,
                            int32_t gpu_index);

/* ObservationManager::FilterPoints3DWithShortTracks(options->min_track_len). 0 = ok. */
int obs_filter_short_tracks(const obs_model* model, const obs_filter_options* options, obs_result* result,
                            int32_t gpu_index);

/* ObservationManager::FilterObservationsWithNegativeDepth: observations of non-spherical cameras with
 * cam_from_world.row(2) . [X; 1] < DBL_EPSILON; a track that would fall below 2 takes its point with it. 0 = ok. */
int obs_filter_negative_depth(const obs_model* model, obs_result* result, int32_t gpu_index);

/* Reconstruction::UpdatePoint3DErrors: point_error = mean over the track of sqrt(CalculateSquaredReprojectionError),
 * 0 for an empty track. Nothing is deleted: obs_keep is all 1, point_status all OBS_POINT_KEPT. 0 = ok. */
int obs_point_errors(const obs_model* model, obs_result* result, int32_t gpu_index);

/* Where the time of the last call of this thread went: its kernels (HIP events), and the whole call including the host
 * plan, allocation and the copies in both directions. */
void obs_last_timing(double* kernel_ms, double* total_ms);

const char* obs_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_OBS_H_ */
