/*
 * colmap_amd_model.h -- C ABI of the statistics of a dense-stage model: the depth range of every image and the
 * shared-point counts / triangulation angles of every image pair, from which `patch_match_stereo` picks the sources of
 * an `__auto__` line and `stereo_fusion` its overlap lists.
 *
 * Replaces, for a model that is already in memory as flat arrays (reference src/colmap/mvs):
 *   model.cc:178-218  Model::ComputeDepthRanges
 *   model.cc:220-235  Model::ComputeSharedPoints
 *   model.cc:237-277  Model::ComputeTriangulationAngles   (math/math.h:205-224 Percentile,
 *                                                           geometry/triangulation.cc:217-249 CalculateTriangulationAngle)
 *   model.cc:120-171  Model::GetMaxOverlappingImages
 * Everything is computed on the GPU (colmap_amd/csrc/model_stats.hip); there is no CPU path. All counts are exact
 * integers and no float is ever added atomically: the same model gives the same bytes on every run.
 */
#ifndef COLMAP_AMD_MODEL_H_
#define COLMAP_AMD_MODEL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mvs::Model as flat arrays. Tracks are in CSR by point: the track of point p is track_image[track_offsets[p]] ..
 * track_image[track_offsets[p + 1] - 1], in track order; an image may appear more than once in a track. */
typedef struct model_flat {
  int32_t num_images;
  int32_t reserved;
  int64_t num_points;
  int64_t num_observations;     /* == track_offsets[num_points] */
  const float* R;               /* [num_images][9] row-major, what mvs::Image::GetR() holds */
  const float* T;               /* [num_images][3] */
  const float* points;          /* [num_points][3] */
  const int64_t* track_offsets; /* [num_points + 1] */
  const int32_t* track_image;   /* [num_observations] image indices */
} model_flat;

/* Pair statistics in CSR by image: the images that share a point with image i are other[row_offsets[i]] ..
 * other[row_offsets[i + 1] - 1], ascending (the iteration order of the reference's std::map); count[] is the
 * shared-point count and angle[] the requested percentile of the triangulation angles (radians) of the same entry. */
typedef struct model_pairs model_pairs;

/* Model::ComputeDepthRanges: ranges[2 i], ranges[2 i + 1] = (min, max) of image i, (-1, -1) for an image without a
 * sparse point of positive depth. 0 = ok. */
int model_compute_depth_ranges(const model_flat* model, float* ranges /* [num_images][2] */, int32_t gpu_index);

/* Model::ComputeSharedPoints and Model::ComputeTriangulationAngles(percentile) in one call; percentile in [0, 100].
 * *out is freed with model_pairs_free. 0 = ok. */
int model_compute_pair_statistics(const model_flat* model, double percentile, model_pairs** out, int32_t gpu_index);

/* Sizes of a result: num_images rows, num_entries entries over all rows. */
void model_pairs_size(const model_pairs* pairs, int32_t* num_images, size_t* num_entries);

/* Copies a result out; a null pointer skips that array. row_offsets [num_images + 1], the others [num_entries]. */
void model_pairs_get(const model_pairs* pairs, int64_t* row_offsets, int32_t* other, int32_t* count, float* angle);

void model_pairs_free(model_pairs* pairs);

/* Model::GetMaxOverlappingImages(num_images_wanted, min_triangulation_angle_deg): per image the up to
 * num_images_wanted images with the most shared points among those whose 75th-percentile triangulation angle is
 * >= (float)DegToRad(min_triangulation_angle_deg); equal counts in ascending image index. CSR: ptr [num_images + 1],
 * idx [*total] -- what fusion_run takes as overlapping images. With ptr == idx == NULL only *total is written (call
 * once to size idx, once to fill it). 0 = ok. */
int model_get_max_overlapping_images(const model_flat* model, int64_t num_images_wanted,
                                     double min_triangulation_angle_deg, int64_t* ptr, int32_t* idx, size_t* total,
                                     int32_t gpu_index);

/* Where the time of the last call of this thread went: its kernels (HIP events), and the whole call including the host
 * plan, allocation and the copies in both directions. */
void model_last_timing(double* kernel_ms, double* total_ms);

const char* model_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_MODEL_H_ */
