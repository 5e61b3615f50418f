/*
 * colmap_amd_sift.h -- C ABI of SIFT feature extraction (`colmap feature_extractor`; reference src/colmap).
 *
 * Replaces SiftGPUFeatureExtractor (feature/sift.cc:552-746) as the GPU extractor, but computes the arithmetic of the
 * reference's VLFeat route, SiftCPUFeatureExtractor::Extract (feature/sift.cc:138-341) over thirdparty/VLFeat/sift.c
 * and imopv.c: the Gaussian scale space, the DoG extrema and their refinement, the gradient planes, the orientation
 * histograms and the 4 x 4 x 8 descriptors. The VLFeat route has one value per input; SiftGPU's does not.
 *
 * The device evaluates + - * / floor and VLFeat's own approximations only. exp (Gaussian taps, the exp(-x) table), pow
 * (the level sigmas, a keypoint's sigma) and sin / cos of a keypoint's angle are the C library's, evaluated on the host
 * (colmap_amd/csrc/sift_plan.h). Rows come out in vl_sift_detect's order: octave, DoG level, raster order of the
 * extremum, orientation index. There is no CPU path.
 */
#ifndef COLMAP_AMD_SIFT_H_
#define COLMAP_AMD_SIFT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SIFT_DESCRIPTOR_DIM = 128, SIFT_NORMALIZATION_L1_ROOT = 0, SIFT_NORMALIZATION_L2 = 1 };
enum { SIFT_STAGE_PYRAMID = 0, SIFT_STAGE_DETECTION = 1, SIFT_STAGE_ORIENTATION = 2, SIFT_STAGE_DESCRIPTOR = 3, SIFT_NUM_STAGES = 4 };

/* SiftExtractionOptions (feature/sift.h:41-101), the members of the built route. */
typedef struct sift_options {
  int32_t max_num_features;     /* 8192 */
  int32_t first_octave;         /* -1 */
  int32_t num_octaves;          /* 4 */
  int32_t octave_resolution;    /* 3 */
  double peak_threshold;        /* 0.02 / 3 */
  double edge_threshold;        /* 10 */
  int32_t max_num_orientations; /* 2 */
  int32_t upright;              /* 0 */
  int32_t normalization;        /* SIFT_NORMALIZATION_L1_ROOT */
  int32_t reserved;
} sift_options;

/* One refined extremum, VlSiftKeypoint (thirdparty/VLFeat/sift.h). */
typedef struct sift_detection {
  int32_t o, ix, iy, is;
  float x, y, s, sigma;
} sift_detection;

typedef struct sift_handle sift_handle;

/* The defaults above. */
void sift_options_init(sift_options* options);

/* SiftExtractionOptions::Check (sift.cc:72-84) plus the limits of the kernels: "" or what is wrong. */
const char* sift_options_check(const sift_options* options);

/* CreateSiftFeatureExtractor / SiftGPUFeatureExtractor::Create (sift.cc:552-640): a handle on one GPU, reused across
 * images of any size; its buffers grow with the largest image seen. 0 = ok. */
int sift_create(int32_t gpu_index, sift_handle** handle);
void sift_destroy(sift_handle* handle);

/* FeatureExtractor::Extract (sift.cc:158-336) of grey[height][width]. The results stay in the handle until the next
 * call. 0 = ok. One case is NOT the reference's: where vl_sift_calc_keypoint_descriptor returns
 * early (a keypoint whose rounded row is the last row of its octave) the reference keeps the descriptor of the row
 * before; here the row's float descriptor and bytes are zero. The tests hold the device to the checker on such rows,
 * not to the reference. */
int sift_extract(sift_handle* handle, const uint8_t* grey, int32_t width, int32_t height, const sift_options* options);

/* Rows of the last result, then copies: keypoints[rows][4] = x, y, scale, orientation (the arguments of the
 * FeatureKeypoint constructor at sift.cc:260-264, x and y with the +0.5 shift), descriptors[rows][128] in UBC order
 * (TransformVLFeatToUBCFeatureDescriptors), float_descriptors[rows][128] as vl_sift_calc_keypoint_descriptor left
 * them (VLFeat order, before L1_ROOT / L2). 0 = ok. */
int64_t sift_num_features(sift_handle* handle);
int sift_copy_keypoints(sift_handle* handle, float* keypoints, int64_t capacity_rows);
int sift_copy_descriptors(sift_handle* handle, uint8_t* descriptors, int64_t capacity_rows);
int sift_copy_float_descriptors(sift_handle* handle, float* descriptors, int64_t capacity_rows);

/* ---- what the tests compare level by level ---- */
/* Octaves of the last extraction; size and octave index `o` of the k-th. */
int32_t sift_num_octaves(sift_handle* handle);
int sift_octave_info(sift_handle* handle, int32_t k, int32_t* width, int32_t* height, int32_t* o);
/* Gaussian level (0 .. S + 2, level 0 is s_min = -1) and DoG level (0 .. S + 1) of octave k, out[height][width]. */
int sift_copy_level(sift_handle* handle, int32_t k, int32_t level, float* out);
int sift_copy_dog(sift_handle* handle, int32_t k, int32_t level, float* out);
/* Gradient plane (0 .. S - 1, plane 0 is level s_min + 1) of octave k, out[height][width][2] = modulus, angle. */
int sift_copy_gradient(sift_handle* handle, int32_t k, int32_t plane, float* out);
/* Extrema found before refinement, refined detections in vl_sift_detect's order, and the orientations
 * vl_sift_calc_keypoint_orientations found for each: counts[n] (0..4) and angles[n][4]. */
int64_t sift_num_candidates(sift_handle* handle, int32_t k);
int64_t sift_num_detections(sift_handle* handle, int32_t k);
int sift_copy_detections(sift_handle* handle, int32_t k, sift_detection* out, int64_t capacity);
int sift_copy_orientations(sift_handle* handle, int32_t k, int32_t* counts, double* angles, int64_t capacity);

/* Sizes of the kernels. pass 0: column pass, 1: row pass of the separable Gaussian; the outputs of one workgroup. */
void sift_conv_tile(int32_t pass, int32_t* tile_x, int32_t* tile_y);
/* Largest half-width of a Gaussian the convolution kernels stage; an option set that needs more is refused. */
int32_t sift_halo_limit(void);
/* Candidates an octave of this size holds before the detection is rerun, and the capacity after `count` overflowed. */
int32_t sift_candidate_capacity(int32_t width, int32_t height, int32_t octave_resolution);
int32_t sift_grown_capacity(int32_t count);
/* Test hook: forces the first candidate capacity of every octave (0: the default). Reruns since creation. */
void sift_set_candidate_capacity(sift_handle* handle, int32_t capacity);
int64_t sift_num_reruns(sift_handle* handle);

/* Times of this thread's last sift_extract in milliseconds. stage_ms[4]: the intervals between HIP events recorded on the
 * stream at the borders of the stages SIFT_STAGE_*, summed over the octaves. An interval is NOT pure kernel time: it
 * also holds the host synchronisations, the copies to the host and the idle gaps inside the stage (the round trip for
 * the candidate count, the compaction of the detections, the assembly of the rows). event_ms is the sum of the four;
 * total_ms is the whole call by the host's clock. */
void sift_last_timing(double* event_ms, double* total_ms, double* stage_ms);

const char* sift_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_SIFT_H_ */
