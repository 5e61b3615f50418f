// color_plan.h -- everything colour extraction decides on the host: the slot layout of a model's observations, the
// checks on what a caller hands to color_add_image and color_finish, and which points take the wave-wide reduction.
// Plain C++17: no HIP runtime -- color_extract.hip checks with it and launches with its lists; tests/cpp/test_color_plan.cc
// checks it without a GPU.
//
// Slot layout: one slot per observation (an image point that has a 3D point), CSR by point -- point p owns the slots
// [ptr[p], ptr[p + 1]) -- and inside a point the observations stand in ascending image id, then ascending point2D index.
// The per-point sum runs in slot order, so this order is what makes a colour a function of the model alone.
#ifndef COLMAP_AMD_COLOR_PLAN_H_
#define COLMAP_AMD_COLOR_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <limits>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

namespace color_plan {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define COLOR_CHECK(cond, msg)                                                    \
  do {                                                                            \
    if (!(cond)) throw ::color_plan::Fail(std::string("Check failed: ") + (msg)); \
  } while (0)

// A point with up to kSerialMax slots is one lane's work; a longer range takes a whole wave: lane g adds the slots
// begin + g, begin + g + 64, ... in ascending order, then the 64 partial sums are combined by the butterfly
// 32, 16, 8, 4, 2, 1 -- an order that depends on the length of the range alone.
constexpr int64_t kSerialMax = 64;
constexpr int kWave = 64;

// obs_point [n] in [0, num_points), obs_image [n], obs_point2D [n] -> ptr [num_points + 1], slot [n]
inline void slot_layout(int64_t num_observations, int64_t num_points, const int64_t* obs_point, const int64_t* obs_image,
                        const int64_t* obs_point2D, int64_t* ptr, int64_t* slot) {
  COLOR_CHECK(num_observations >= 0 && num_points >= 0, "counts must not be negative");
  COLOR_CHECK(ptr != nullptr, "ptr is null (it has num_points + 1 entries)");
  COLOR_CHECK(num_observations == 0 || (obs_point && obs_image && obs_point2D && slot), "observation arrays are null");
  for (int64_t o = 0; o < num_observations; ++o)
    COLOR_CHECK(obs_point[o] >= 0 && obs_point[o] < num_points,
                "observation " + std::to_string(o) + ": point index " + std::to_string(obs_point[o]) + " out of range");
  std::vector<int64_t> order((size_t)num_observations);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    if (obs_point[a] != obs_point[b]) return obs_point[a] < obs_point[b];
    if (obs_image[a] != obs_image[b]) return obs_image[a] < obs_image[b];
    if (obs_point2D[a] != obs_point2D[b]) return obs_point2D[a] < obs_point2D[b];
    return a < b;
  });
  for (int64_t p = 0; p <= num_points; ++p) ptr[p] = 0;
  for (int64_t o = 0; o < num_observations; ++o) ++ptr[obs_point[o] + 1];
  for (int64_t p = 0; p < num_points; ++p) ptr[p + 1] += ptr[p];
  for (int64_t k = 0; k < num_observations; ++k) slot[order[(size_t)k]] = k;
}

// The slots of one color_add_image call against the slots taken so far (taken[s] != 0); marks them taken. Nothing is
// marked when a check fails.
inline void check_and_take_slots(std::vector<uint8_t>* taken, int64_t n, const int64_t* slot) {
  COLOR_CHECK(n >= 0, "the number of observations must not be negative");
  COLOR_CHECK(n == 0 || slot != nullptr, "slot is null");
  const int64_t num_slots = (int64_t)taken->size();
  for (int64_t i = 0; i < n; ++i)
    COLOR_CHECK(slot[i] >= 0 && slot[i] < num_slots, "observation " + std::to_string(i) + ": slot " + std::to_string(slot[i]) +
                                                         " out of range [0, " + std::to_string(num_slots) + ")");
  for (int64_t i = 0; i < n; ++i) {
    if ((*taken)[(size_t)slot[i]]) {
      for (int64_t j = 0; j < i; ++j) (*taken)[(size_t)slot[j]] = 0;  // undo this call's marks (all distinct so far)
      COLOR_CHECK(false, "observation " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + " given twice");
    }
    (*taken)[(size_t)slot[i]] = 1;
  }
}

inline void check_image(int32_t width, int32_t height, int32_t channels, const void* data) {
  COLOR_CHECK(data != nullptr, "null pixel buffer");
  COLOR_CHECK(width > 0 && height > 0, "image width and height must be positive");
  COLOR_CHECK(channels == 1 || channels == 3, "channels must be 1 (grey) or 3 (RGB)");
  COLOR_CHECK((int64_t)width * height * 3 <= (int64_t)std::numeric_limits<int32_t>::max(),
              "the image must have fewer than 2^31 bytes as RGB");
}

// ptr [num_points + 1] of color_finish: starts at or after 0, never decreases, ends inside the slots
inline void check_ptr(int64_t num_slots, int64_t num_points, const int64_t* ptr) {
  COLOR_CHECK(num_points >= 0, "num_points must not be negative");
  COLOR_CHECK(ptr != nullptr, "ptr is null (it has num_points + 1 entries)");
  COLOR_CHECK(ptr[0] >= 0, "ptr must not start below 0");
  for (int64_t p = 0; p < num_points; ++p)
    COLOR_CHECK(ptr[p + 1] >= ptr[p], "ptr decreases at point " + std::to_string(p));
  COLOR_CHECK(ptr[num_points] <= num_slots, "ptr ends at " + std::to_string(ptr[num_points]) + ", beyond the " +
                                                std::to_string(num_slots) + " slots");
}

// the points whose range takes the wave-wide reduction, ascending (of a checked ptr)
inline std::vector<int64_t> long_points(int64_t num_points, const int64_t* ptr) {
  std::vector<int64_t> out;
  for (int64_t p = 0; p < num_points; ++p)
    if (ptr[p + 1] - ptr[p] > kSerialMax) out.push_back(p);
  return out;
}

}  // namespace color_plan
#endif  // COLMAP_AMD_COLOR_PLAN_H_
