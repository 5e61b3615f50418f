// undistortion.hpp -- C++ host side of image undistortion (reference image/undistortion.h: UndistortCameraOptions,
// UndistortCamera, UndistortImage, UndistortReconstruction, RectifyStereoCameras, RectifyAndUndistortStereoImages;
// image/warp.h: WarpImageOptions) over the C ABI of
// colmap_amd_undistort.h. Header-only, standard library only.
//
//   colmap_amd::UndistortCameraOptions options;
//   colmap_amd::Camera pinhole = colmap_amd::UndistortCamera(options, camera);          // host only, no GPU needed
//   colmap_amd::Bitmap out; colmap_amd::Camera out_camera;
//   colmap_amd::UndistortImage(options, bitmap, camera, &out, &out_camera);             // on the GPU
//
// Errors are std::runtime_error carrying undistort_last_error().
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../colmap_amd_undistort.h"
#include "camera.hpp"

namespace colmap_amd {

struct WarpImageOptions {  // image/warp.h
  enum class Interpolation { kNearestNeighbor = UNDISTORT_NEAREST, kBilinear = UNDISTORT_BILINEAR };
  Interpolation interpolation = Interpolation::kBilinear;
  double direct_warp_min_scale = 0.5;
};

struct UndistortCameraOptions {  // image/undistortion.h:38-71
  double blank_pixels = 0.0;
  double min_scale = 0.2;
  double max_scale = 2.0;
  int max_image_size = -1;
  double roi_min_x = 0.0;
  double roi_min_y = 0.0;
  double roi_max_x = 1.0;
  double roi_max_y = 1.0;
  double max_cam_point_norm = -1;
  WarpImageOptions warp_options;
  int gpu_index = 0;  // (MI355X) the device the pixels and observations are computed on
};

struct Bitmap {  // 8-bit grey (channels 1) or RGB (channels 3), rows tight
  int width = 0, height = 0, channels = 1;
  std::vector<uint8_t> data;
};

namespace undistort_detail {
inline undistort_options ToC(const UndistortCameraOptions& o) {
  undistort_options c;
  undistort_options_init(&c);
  c.blank_pixels = o.blank_pixels;
  c.min_scale = o.min_scale;
  c.max_scale = o.max_scale;
  c.max_image_size = o.max_image_size;
  c.interpolation = static_cast<int>(o.warp_options.interpolation);
  c.roi_min_x = o.roi_min_x;
  c.roi_min_y = o.roi_min_y;
  c.roi_max_x = o.roi_max_x;
  c.roi_max_y = o.roi_max_y;
  c.max_cam_point_norm = o.max_cam_point_norm;
  c.direct_warp_min_scale = o.warp_options.direct_warp_min_scale;
  return c;
}
inline undistort_cam ToC(const Camera& cam) {
  undistort_cam c = {};
  if (cam.params.size() > 16) throw std::runtime_error("camera with more than 16 parameters");
  c.model_id = cam.model_id;
  c.width = cam.width;
  c.height = cam.height;
  for (size_t i = 0; i < cam.params.size(); ++i) c.params[i] = cam.params[i];
  return c;
}
inline Camera FromC(const undistort_cam& c) {  // of a camera the library wrote: a known model
  Camera cam;
  cam.model_id = c.model_id;
  cam.width = c.width;
  cam.height = c.height;
  const camera_models::ModelInfo* info = camera_models::model_info(c.model_id);
  if (!info) throw std::runtime_error("unknown camera model id " + std::to_string(c.model_id));
  cam.params.assign(c.params, c.params + info->num_params);
  return cam;
}
inline void Check(int rc) {
  if (rc != 0) throw std::runtime_error(undistort_last_error());
}
}  // namespace undistort_detail

// UndistortCamera (image/undistortion.cc:58-264): host only.
inline Camera UndistortCamera(const UndistortCameraOptions& options, const Camera& camera) {
  const undistort_options o = undistort_detail::ToC(options);
  const undistort_cam c = undistort_detail::ToC(camera);
  undistort_cam u;
  undistort_detail::Check(undistort_camera(&o, &c, &u));
  return undistort_detail::FromC(u);
}

// UndistortImage (image/undistortion.cc:266-301) on device options.gpu_index.
inline void UndistortImage(const UndistortCameraOptions& options, const Bitmap& distorted_bitmap,
                           const Camera& distorted_camera, Bitmap* undistorted_bitmap, Camera* undistorted_camera) {
  if (distorted_camera.width != distorted_bitmap.width || distorted_camera.height != distorted_bitmap.height ||
      distorted_bitmap.data.size() != static_cast<size_t>(distorted_bitmap.width) * distorted_bitmap.height * distorted_bitmap.channels)
    throw std::runtime_error("the bitmap does not match its camera");
  const undistort_options o = undistort_detail::ToC(options);
  undistort_image im = {};
  im.camera = undistort_detail::ToC(distorted_camera);
  im.data = distorted_bitmap.data.data();
  im.channels = distorted_bitmap.channels;
  // the output is never larger than max_scale times the source in either direction (and a spherical image never grows)
  const double s = distorted_camera.IsSpherical() ? 1.0 : std::max(1.0, options.max_scale);
  const size_t cap = static_cast<size_t>(std::ceil(s * distorted_camera.width)) *
                     static_cast<size_t>(std::ceil(s * distorted_camera.height)) * distorted_bitmap.channels;
  undistorted_bitmap->data.resize(cap);
  im.out = undistorted_bitmap->data.data();
  im.out_capacity = cap;
  undistort_detail::Check(undistort_images(&o, 1, &im, options.gpu_index));
  *undistorted_camera = undistort_detail::FromC(im.out_camera);
  undistorted_bitmap->width = im.out_camera.width;
  undistorted_bitmap->height = im.out_camera.height;
  undistorted_bitmap->channels = distorted_bitmap.channels;
  undistorted_bitmap->data.resize(static_cast<size_t>(im.out_camera.width) * im.out_camera.height * distorted_bitmap.channels);
}

// RectifyStereoCameras (image/undistortion.cc:384-445): host only. cam2_from_cam1 as a row-major rotation R[9] and a
// translation t[3]; H1, H2 (3x3) and Q (4x4) row-major.
inline void RectifyStereoCameras(const Camera& camera1, const Camera& camera2, const double* R, const double* t,
                                 double (*H1)[9], double (*H2)[9], double (*Q)[16]) {
  const undistort_cam c1 = undistort_detail::ToC(camera1), c2 = undistort_detail::ToC(camera2);
  undistort_detail::Check(undistort_rectify_cameras(&c1, &c2, R, t, *H1, *H2, *Q));
}

// RectifyAndUndistortStereoImages (image/undistortion.cc:447-490) on device options.gpu_index.
inline void RectifyAndUndistortStereoImages(const UndistortCameraOptions& options, const Bitmap& distorted_image1,
                                            const Bitmap& distorted_image2, const Camera& distorted_camera1,
                                            const Camera& distorted_camera2, const double* R, const double* t,
                                            Bitmap* undistorted_image1, Bitmap* undistorted_image2,
                                            Camera* undistorted_camera, double (*Q)[16]) {
  const Bitmap* in[2] = {&distorted_image1, &distorted_image2};
  const Camera* cams[2] = {&distorted_camera1, &distorted_camera2};
  Bitmap* out[2] = {undistorted_image1, undistorted_image2};
  for (int s = 0; s < 2; ++s)
    if (cams[s]->width != in[s]->width || cams[s]->height != in[s]->height ||
        in[s]->data.size() != static_cast<size_t>(in[s]->width) * in[s]->height * in[s]->channels)
      throw std::runtime_error("the bitmap does not match its camera");
  const undistort_options o = undistort_detail::ToC(options);
  const Camera target = UndistortCamera(options, distorted_camera1);
  undistort_stereo_pair pair = {};
  undistort_image* im[2] = {&pair.image1, &pair.image2};
  for (int s = 0; s < 2; ++s) {
    im[s]->camera = undistort_detail::ToC(*cams[s]);
    im[s]->data = in[s]->data.data();
    im[s]->channels = in[s]->channels;
    out[s]->data.resize(static_cast<size_t>(target.width) * target.height * in[s]->channels);
    im[s]->out = out[s]->data.data();
    im[s]->out_capacity = out[s]->data.size();
  }
  for (int i = 0; i < 9; ++i) pair.R[i] = R[i];
  for (int i = 0; i < 3; ++i) pair.t[i] = t[i];
  undistort_detail::Check(undistort_rectify_images(&o, 1, &pair, options.gpu_index));
  *undistorted_camera = undistort_detail::FromC(pair.image1.out_camera);
  for (int s = 0; s < 2; ++s) {
    out[s]->width = pair.image1.out_camera.width;
    out[s]->height = pair.image1.out_camera.height;
    out[s]->channels = in[s]->channels;
  }
  for (int i = 0; i < 16; ++i) (*Q)[i] = pair.Q[i];
}

// UndistortReconstruction (image/undistortion.cc:303-382) over caller arrays: cameras[i] is rewritten to PINHOLE (or a
// resized spherical camera) unless it is kept unchanged (:316-318); the observations of every image -- xy[k] holds
// x0 y0 x1 y1 ... of an image whose camera is cameras[camera_of_image[k]] -- are moved in place, NaN where the
// reference stores NaN.
inline void UndistortReconstruction(const UndistortCameraOptions& options, std::vector<Camera>* cameras,
                                    const std::vector<int>& camera_of_image, std::vector<std::vector<double>>* xy) {
  if (camera_of_image.size() != xy->size()) throw std::runtime_error("one camera index per image");
  const std::vector<Camera> distorted = *cameras;
  std::vector<bool> keep(distorted.size());
  for (size_t i = 0; i < distorted.size(); ++i) {
    keep[i] = distorted[i].IsUndistorted() && options.max_image_size < 0;
    if (keep[i]) continue;
    if (distorted[i].IsSpherical()) {  // RescaleToMaxImageSize (:43-54), Camera::Rescale (scene/camera.cc:113-121)
      Camera& c = (*cameras)[i];
      const double scale = std::min(options.max_image_size / static_cast<double>(c.width),
                                    options.max_image_size / static_cast<double>(c.height));
      if (scale < 1.0) {
        const int w = static_cast<int>(std::round(scale * c.width)), h = static_cast<int>(std::round(scale * c.height));
        c.params[0] *= static_cast<double>(w) / c.width;
        c.params[1] *= static_cast<double>(h) / c.height;
        c.width = w;
        c.height = h;
      }
    } else {
      (*cameras)[i] = UndistortCamera(options, distorted[i]);
    }
  }
  for (size_t k = 0; k < xy->size(); ++k) {
    const size_t ci = static_cast<size_t>(camera_of_image[k]);
    if (ci >= distorted.size()) throw std::runtime_error("camera index out of range");
    std::vector<double>& pts = (*xy)[k];
    if (keep[ci] || pts.empty()) continue;
    const undistort_cam d = undistort_detail::ToC(distorted[ci]), u = undistort_detail::ToC((*cameras)[ci]);
    undistort_detail::Check(undistort_points(&d, &u, pts.data(), static_cast<int64_t>(pts.size() / 2), options.gpu_index));
  }
}

}  // namespace colmap_amd
