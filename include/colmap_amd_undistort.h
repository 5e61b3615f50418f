/*
 * colmap_amd_undistort.h -- C ABI of image undistortion: the step that turns a sparse model with real lenses
 * into the pinhole dense workspace PatchMatch and fusion start from.
 *
 * Replaces, for inputs that are already in memory (reference src/colmap):
 *   image/undistortion.cc:58-264    UndistortCamera            -> undistort_camera (host only)
 *   image/undistortion.cc:266-301   UndistortImage             -> undistort_images
 *   image/warp.cc:72-165            WarpImageBetweenCameras    -> the kernels behind undistort_images
 *   image/undistortion.cc:334-381   the observation loop of UndistortReconstruction -> undistort_points
 *   image/undistortion.cc:384-445   RectifyStereoCameras       -> undistort_rectify_cameras (host only)
 *   image/undistortion.cc:447-490   RectifyAndUndistortStereoImages -> undistort_rectify_images
 *   image/warp.cc:196-272           WarpImageWithHomographyBetweenCameras -> undistort_warp_homography
 * The caller (colmap_amd/undistortion.py, the `image_undistorter` command, include/colmap_amd/undistortion.hpp) does
 * the file reading and writing of controllers/undistorters.cc. Pixels and observations are computed on the GPU
 * (colmap_amd/csrc/undistort.hip); there is no CPU path for them. All geometry is double precision.
 * Difference to the reference: the indirect path (target much smaller than the source) and the resize of spherical
 * images shrink with the triangle filter defined in colmap_amd/csrc/undistort.hip, not OpenImageIO's.
 */
#ifndef COLMAP_AMD_UNDISTORT_H_
#define COLMAP_AMD_UNDISTORT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* colmap::Camera (scene/camera.h): model_id is colmap::CameraModelId (sensor/models.h:90-111), params in the order
 * of the model's ParamsInfo. */
typedef struct undistort_cam {
  int32_t model_id;
  int32_t width, height;
  int32_t reserved;
  double params[16];
} undistort_cam;

enum { UNDISTORT_NEAREST = 0, UNDISTORT_BILINEAR = 1 }; /* WarpImageOptions::Interpolation (image/warp.h) */

/* colmap::UndistortCameraOptions (image/undistortion.h:38-71) with its WarpImageOptions (image/warp.h) inline. */
typedef struct undistort_options {
  double blank_pixels;          /* 0 */
  double min_scale;             /* 0.2 */
  double max_scale;             /* 2.0 */
  int32_t max_image_size;       /* -1 */
  int32_t interpolation;        /* UNDISTORT_BILINEAR */
  double roi_min_x, roi_min_y;  /* 0, 0 */
  double roi_max_x, roi_max_y;  /* 1, 1 */
  double max_cam_point_norm;    /* -1 */
  double direct_warp_min_scale; /* 0.5 */
} undistort_options;

/* One image of undistort_images: the distorted camera, its pixels (height * width * channels bytes, channels 1 = grey
 * or 3 = RGB, rows tight) and a caller-owned output buffer of out_capacity bytes. On return out_camera is the
 * undistorted camera and out holds out_camera.height * out_camera.width * channels bytes. undistort_camera predicts
 * out_camera for a perspective camera; a spherical one keeps its model and is only resized to max_image_size. */
typedef struct undistort_image {
  undistort_cam camera;
  const uint8_t* data;
  int32_t channels;
  int32_t reserved;
  uint8_t* out;
  size_t out_capacity;
  undistort_cam out_camera;
} undistort_image;

/* The member initialisers of UndistortCameraOptions / WarpImageOptions. */
void undistort_options_init(undistort_options* options);

/* UndistortCamera (image/undistortion.cc:58-264), with its option checks (:60-76, :137). HOST ONLY: the border trace
 * is 2 (W + H) points; callable without a GPU. 0 = ok. */
int undistort_camera(const undistort_options* options, const undistort_cam* camera, undistort_cam* undistorted);

/* Camera::CamFromImg (sensor/models.h CameraModelCamFromImg) for n pixels xy [n][2] -> uv [n][2]; NaN where the
 * reference returns no value. HOST ONLY (what undistort_camera traces the border with). 0 = ok. */
int undistort_cam_from_img(const undistort_cam* camera, const double* xy, int64_t n, double* uv);

/* UndistortImage (image/undistortion.cc:266-301) for n images on device gpu_index: direct warp, or warp at source
 * resolution + shrink when ShouldWarpDirectly (image/warp.cc:72-89) says so. Blank pixels are 0. Fails with
 * "no HIP device available" when there is none. 0 = ok. */
int undistort_images(const undistort_options* options, int32_t num_images, undistort_image* images, int32_t gpu_index);

/* The observation loop of UndistortReconstruction (image/undistortion.cc:334-381) for the n observations xy [n][2]
 * of one camera, in place: xy -> CamFromImg(distorted) -> ImgFromCam(undistorted); NaN where either has no value
 * (:362-379); a spherical camera scales linearly (:343-359). On device gpu_index. 0 = ok. */
int undistort_points(const undistort_cam* distorted, const undistort_cam* undistorted, double* xy, int64_t n,
                     int32_t gpu_index);

/* RectifyStereoCameras (image/undistortion.cc:384-445). Both cameras SIMPLE_PINHOLE or PINHOLE, else an error.
 * cam2_from_cam1 as row-major R[9], t[3]. Outputs row-major H1[9], H2[9], Q[16]. HOST ONLY. 0 = ok. */
int undistort_rectify_cameras(const undistort_cam* camera1, const undistort_cam* camera2, const double* R,
                              const double* t, double* H1, double* H2, double* Q);

/* One stereo pair of undistort_rectify_images. Both images are filled in like undistort_image (camera, data, channels,
 * out, out_capacity); on return out_camera of both is UndistortCamera(options, image1.camera) and Q the
 * disparity-to-depth matrix of the pair, row-major. */
typedef struct undistort_stereo_pair {
  undistort_image image1, image2; /* out_camera of both = UndistortCamera(options, image1.camera) */
  double R[9], t[3];              /* cam2_from_cam1 */
  double Q[16];                   /* out */
} undistort_stereo_pair;

/* RectifyAndUndistortStereoImages (image/undistortion.cc:447-490) for n pairs on device gpu_index: the undistorted
 * camera comes from camera 1 only (:462), H1 and H2 from RectifyStereoCameras of that camera with itself (:475-476),
 * both images are warped with the inverse homography in front of the target camera (image/warp.cc:196-250).
 * Difference to the reference: when ShouldWarpDirectly is false for a source camera, the reference enlarges the canvas
 * to the source's size but leaves H and the target camera unscaled, which is not a scaled version of the direct result.
 * Here the indirect path is the consistent one: the target camera is rescaled to the source's size (as
 * WarpImageBetweenCameras does, image/warp.cc:103-106), the homography is conjugated with that pixel scaling
 * S = diag(sx, sy, 1) -- S Hinv S^-1 in front of the rescaled camera, i.e. Hinv diag(1/sx, 1/sy, 1) in front of the target
 * camera --, the warp runs at source size and the result is shrunk with the library's triangle filter. 0 = ok. */
int undistort_rectify_images(const undistort_options* options, int32_t num_pairs, undistort_stereo_pair* pairs,
                             int32_t gpu_index);

/* WarpImageWithHomographyBetweenCameras (image/warp.cc:196-272), direct path only: image->camera is the source,
 * target_camera a PINHOLE camera, Hinv row-major maps a target pixel (x + 1/2, y + 1/2, 1) to the pixel the target camera
 * unprojects; a pixel whose third coordinate is 0 is 0. image->out takes target height * width * channels bytes. 0 = ok. */
int undistort_warp_homography(const undistort_options* options, const double* Hinv, const undistort_cam* target_camera,
                              undistort_image* image, int32_t gpu_index);

/* Bitmap::Rescale as this library does it (the triangle filter of colmap_amd/csrc/undistort.hip) on device
 * gpu_index: src [src_height][src_width][channels] -> dst [dst_height][dst_width][channels]. 0 = ok. */
int undistort_resize(const uint8_t* src, int32_t src_width, int32_t src_height, int32_t channels, uint8_t* dst,
                     int32_t dst_width, int32_t dst_height, int32_t gpu_index);

/* Where the time of the last undistort_images or undistort_rectify_images of this thread went: its kernels (HIP events), and the whole call
 * including allocation and the copies in both directions. */
void undistort_last_timing(double* kernel_ms, double* total_ms);

const char* undistort_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_UNDISTORT_H_ */
