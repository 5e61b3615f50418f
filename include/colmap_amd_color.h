/*
 * colmap_amd_color.h -- C ABI of colour extraction: the colours of a sparse model's 3D points from its source images.
 *
 * Replaces, for images that are already decoded (reference src/colmap):
 *   scene/reconstruction.cc:1122-1184  Reconstruction::ExtractColorsForAllImages -> color_add_image + color_finish
 *   scene/reconstruction.cc:1094-1120  Reconstruction::ExtractColorsForImage     -> color_add_image + color_samples
 *   sensor/bitmap.cc                   Bitmap::InterpolateBilinear               -> the kernel behind color_add_image
 * The caller (colmap_amd/color_extraction.py, the `color_extractor` command, include/colmap_amd/colors.hpp) reads the
 * model and decodes the images. Samples and means are computed on the GPU (colmap_amd/csrc/color_extract.hip); there is
 * no CPU path for them.
 *
 * A handle holds one slot per observation -- three floats and a valid byte, 13 bytes -- so that images can stream
 * through as the host decodes them. Point p owns the slots [ptr[p], ptr[p + 1]); its colour is the mean of its valid
 * samples, added in double IN SLOT ORDER, rounded half away from zero. There is no atomic anywhere: the same calls give
 * the same bytes on every run. color_slot_layout gives the layout the package uses (observations of a point in ascending
 * image id, then point2D index).
 */
#ifndef COLMAP_AMD_COLOR_H_
#define COLMAP_AMD_COLOR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct color_extractor color_extractor;

/* One 13-byte slot per observation on device gpu_index, all invalid. NULL on failure (color_last_error): "no HIP device
 * available" when there is none. */
color_extractor* color_create(int64_t num_observations, int32_t gpu_index);

/* One image: pixels (channels 1 or 3, rows tight; grey is replicated to RGB as Bitmap::Read(as_rgb=true) does),
 * n observations xy[n][2] in COLMAP pixel coordinates (the upper left pixel centre is (0.5, 0.5)) and, for each, the slot
 * its sample is stored in: InterpolateBilinear(x - 1/2, y - 1/2) as a float per channel, valid where the reference
 * returns a value. A slot out of range or given twice (in this call or an earlier one) is an error, and then nothing of
 * the call is stored. 0 = ok. */
int color_add_image(color_extractor* extractor, const uint8_t* data, int32_t width, int32_t height, int32_t channels,
                    int64_t n, const double* xy, const int64_t* slot);

/* Means over slot ranges: point p owns slots [ptr[p], ptr[p+1]), ptr monotone inside [0, num_observations].
 * rgb[num_points][3] = round(sum / count) per channel, count[num_points] (may be NULL) = the valid samples of the
 * point; (0, 0, 0) and 0 for a point without one. Slots never written are invalid. 0 = ok. */
int color_finish(color_extractor* extractor, int64_t num_points, const int64_t* ptr, uint8_t* rgb, int32_t* count);

/* The samples as stored: rgb[num_observations][3] floats and valid[num_observations]; for tests and
 * ExtractColorsForImage. The floats of an invalid slot are 0. 0 = ok. */
int color_samples(color_extractor* extractor, float* rgb, uint8_t* valid);

void color_destroy(color_extractor* extractor);

/* HOST ONLY, callable without a GPU. The slot layout of a model: observation o belongs to point obs_point[o] in
 * [0, num_points) and is point2D obs_point2D[o] of image obs_image[o]. Writes ptr[num_points + 1] and slot[n]: CSR by
 * point, the observations of a point in ascending image id, then point2D index. 0 = ok. */
int color_slot_layout(int64_t num_observations, int64_t num_points, const int64_t* obs_point, const int64_t* obs_image,
                      const int64_t* obs_point2D, int64_t* ptr, int64_t* slot);

/* Where the time of this handle went so far: the sample kernels and the point kernels (HIP events), and the calls
 * including allocation and the copies in both directions. Any pointer may be NULL. */
void color_timing(color_extractor* extractor, double* sample_kernel_ms, double* point_kernel_ms, double* total_ms);

const char* color_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_COLOR_H_ */
