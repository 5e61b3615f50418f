// colors.hpp -- C++ host side of colour extraction (reference scene/reconstruction.cc:1122-1184,
// Reconstruction::ExtractColorsForAllImages) over the C ABI of colmap_amd_color.h. Header-only, standard library only.
//
//   std::vector<colmap_amd::ColorImage> images = ...;            // decoded pixels, 8-bit grey or RGB
//   std::vector<colmap_amd::ColorObservation> observations = ...; // image index, point index, point2D index, x, y
//   std::vector<std::array<uint8_t, 3>> colors = colmap_amd::ExtractColors(images, observations, num_points);
//
// Errors are std::runtime_error carrying color_last_error().
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../colmap_amd_color.h"

namespace colmap_amd {

struct ColorImage {  // 8-bit grey (channels 1) or RGB (channels 3), rows tight; an empty image could not be read
  int width = 0, height = 0, channels = 3;
  const uint8_t* data = nullptr;
};

struct ColorObservation {
  int64_t image = 0;    // index into images; the observations of a point are added in ascending image, then point2D
  int64_t point = 0;    // in [0, num_points)
  int64_t point2D = 0;  // the index of the observation inside its image
  double x = 0.0, y = 0.0;  // COLMAP pixel coordinates: the upper left pixel centre is (0.5, 0.5)
};

// ExtractColorsForAllImages over caller arrays on device gpu_index: colors[p] is the rounded mean of the bilinear
// samples of point p over the images that have pixels (data != nullptr), (0, 0, 0) for a point without a sample;
// counts (optional) takes the number of samples per point.
inline std::vector<std::array<uint8_t, 3>> ExtractColors(const std::vector<ColorImage>& images,
                                                        const std::vector<ColorObservation>& observations,
                                                        int64_t num_points, int gpu_index = 0,
                                                        std::vector<int32_t>* counts = nullptr) {
  auto fail = [] { throw std::runtime_error(color_last_error()); };
  const int64_t n = static_cast<int64_t>(observations.size());
  std::vector<int64_t> obs_point(n), obs_image(n), obs_point2D(n), slot(n), ptr(static_cast<size_t>(num_points) + 1);
  for (int64_t o = 0; o < n; ++o) {
    const ColorObservation& ob = observations[static_cast<size_t>(o)];
    if (ob.image < 0 || ob.image >= static_cast<int64_t>(images.size()))
      throw std::runtime_error("observation " + std::to_string(o) + ": image index out of range");
    obs_point[o] = ob.point;
    obs_image[o] = ob.image;
    obs_point2D[o] = ob.point2D;
  }
  if (color_slot_layout(n, num_points, obs_point.data(), obs_image.data(), obs_point2D.data(), ptr.data(), slot.data()) != 0)
    fail();
  // the observations of every image, in the order given
  std::vector<std::vector<double>> xy(images.size());
  std::vector<std::vector<int64_t>> slots(images.size());
  for (int64_t o = 0; o < n; ++o) {
    const ColorObservation& ob = observations[static_cast<size_t>(o)];
    xy[static_cast<size_t>(ob.image)].push_back(ob.x);
    xy[static_cast<size_t>(ob.image)].push_back(ob.y);
    slots[static_cast<size_t>(ob.image)].push_back(slot[o]);
  }
  color_extractor* extractor = color_create(n, gpu_index);
  if (!extractor) fail();
  struct Closer {
    color_extractor* e;
    ~Closer() { color_destroy(e); }
  } closer{extractor};
  for (size_t i = 0; i < images.size(); ++i) {
    const ColorImage& im = images[i];
    if (!im.data || slots[i].empty()) continue;  // an unreadable image is skipped
    if (color_add_image(extractor, im.data, im.width, im.height, im.channels, static_cast<int64_t>(slots[i].size()),
                        xy[i].data(), slots[i].data()) != 0)
      fail();
  }
  std::vector<std::array<uint8_t, 3>> colors(static_cast<size_t>(num_points));
  if (counts) counts->assign(static_cast<size_t>(num_points), 0);
  static_assert(sizeof(std::array<uint8_t, 3>) == 3, "colours are handed over as rgb[num_points][3]");
  if (color_finish(extractor, num_points, ptr.data(), num_points ? colors[0].data() : nullptr,
                   counts && num_points ? counts->data() : nullptr) != 0)
    fail();
  return colors;
}

}  // namespace colmap_amd
