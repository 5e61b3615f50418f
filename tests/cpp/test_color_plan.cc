// The host-only plan of colour extraction (colmap_amd/csrc/color_plan.h) without a GPU: the slot layout of a 5-point
// model against the layout written out by hand, and every refused argument with its message. The arrays are exactly
// sized heap arrays, so that under the sanitizers a read or write past a bad slot before its check would be reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "color_plan.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

template <typename F>
static std::string message_of(F&& f) {
  try {
    f();
  } catch (const color_plan::Fail& e) {
    return e.what();
  }
  return "";
}

static bool contains(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
  // 5 points, 3 images; observations in image order as a reader meets them (image id, point2D index, point):
  //   image 7: (0 -> p3) (1 -> p0) (3 -> p3)      image 2: (0 -> p0) (2 -> p4) (5 -> p1)      image 9: (1 -> p0) (0 -> p1)
  // point 2 has no observation. Inside a point: ascending image id, then point2D index.
  const std::vector<int64_t> obs_image = {7, 7, 7, 2, 2, 2, 9, 9};
  const std::vector<int64_t> obs_p2d = {0, 1, 3, 0, 2, 5, 1, 0};
  const std::vector<int64_t> obs_point = {3, 0, 3, 0, 4, 1, 0, 1};
  std::vector<int64_t> ptr(6, -1), slot(8, -1);
  color_plan::slot_layout(8, 5, obs_point.data(), obs_image.data(), obs_p2d.data(), ptr.data(), slot.data());
  const std::vector<int64_t> want_ptr = {0, 3, 5, 5, 7, 8};
  // p0: (2,0) (7,1) (9,1) -> slots 0 1 2; p1: (2,5) (9,0) -> 3 4; p3: (7,0) (7,3) -> 5 6; p4: (2,2) -> 7
  const std::vector<int64_t> want_slot = {5, 1, 6, 0, 7, 3, 2, 4};
  EXPECT(ptr == want_ptr);
  EXPECT(slot == want_slot);
  EXPECT(contains(message_of([&] {
                    std::vector<int64_t> bad = obs_point;
                    bad[4] = 5;
                    color_plan::slot_layout(8, 5, bad.data(), obs_image.data(), obs_p2d.data(), ptr.data(), slot.data());
                  }),
                  "point index 5 out of range"));
  color_plan::slot_layout(0, 0, nullptr, nullptr, nullptr, ptr.data(), nullptr);  // an empty model has a layout
  EXPECT(ptr[0] == 0);

  // the slots of color_add_image
  std::vector<uint8_t> taken(8, 0);
  const std::vector<int64_t> first = {5, 1, 6};
  color_plan::check_and_take_slots(&taken, 3, first.data());
  EXPECT(taken[5] && taken[1] && taken[6] && !taken[0]);
  const std::vector<int64_t> again = {0, 7, 1};  // 1 was given by the earlier call
  EXPECT(contains(message_of([&] { color_plan::check_and_take_slots(&taken, 3, again.data()); }), "slot 1 given twice"));
  EXPECT(!taken[0] && !taken[7] && taken[1]);  // the refused call took nothing
  const std::vector<int64_t> twice = {0, 7, 0};
  EXPECT(contains(message_of([&] { color_plan::check_and_take_slots(&taken, 3, twice.data()); }), "slot 0 given twice"));
  EXPECT(!taken[0] && !taken[7]);
  const std::vector<int64_t> beyond = {0, 8};
  EXPECT(contains(message_of([&] { color_plan::check_and_take_slots(&taken, 2, beyond.data()); }), "slot 8 out of range"));
  const std::vector<int64_t> negative = {-1};
  EXPECT(contains(message_of([&] { color_plan::check_and_take_slots(&taken, 1, negative.data()); }), "slot -1 out of range"));
  EXPECT(!taken[0]);
  EXPECT(contains(message_of([&] { color_plan::check_and_take_slots(&taken, 1, nullptr); }), "slot is null"));
  const std::vector<int64_t> rest = {0, 7, 2, 3, 4};
  color_plan::check_and_take_slots(&taken, 5, rest.data());
  for (uint8_t t : taken) EXPECT(t == 1);

  // ptr of color_finish
  color_plan::check_ptr(8, 5, want_ptr.data());
  const std::vector<int64_t> decreasing = {0, 3, 2, 5, 7, 8};
  EXPECT(contains(message_of([&] { color_plan::check_ptr(8, 5, decreasing.data()); }), "ptr decreases at point 1"));
  EXPECT(contains(message_of([&] { color_plan::check_ptr(7, 5, want_ptr.data()); }), "beyond the 7 slots"));
  const std::vector<int64_t> below = {-1, 3, 5, 5, 7, 8};
  EXPECT(contains(message_of([&] { color_plan::check_ptr(8, 5, below.data()); }), "must not start below 0"));
  EXPECT(contains(message_of([&] { color_plan::check_ptr(8, 5, nullptr); }), "ptr is null"));

  // images
  const uint8_t pixel[3] = {0, 0, 0};
  color_plan::check_image(1, 1, 3, pixel);
  EXPECT(contains(message_of([&] { color_plan::check_image(1, 1, 2, pixel); }), "channels must be 1 (grey) or 3 (RGB)"));
  EXPECT(contains(message_of([&] { color_plan::check_image(0, 1, 3, pixel); }), "must be positive"));
  EXPECT(contains(message_of([&] { color_plan::check_image(1, 1, 3, nullptr); }), "null pixel buffer"));
  EXPECT(contains(message_of([&] { color_plan::check_image(40000, 40000, 1, pixel); }), "fewer than 2^31 bytes"));

  // which points take the wave-wide reduction: more than kSerialMax slots
  const std::vector<int64_t> long_ptr = {0, 64, 129, 129, 200};
  const std::vector<int64_t> longs = color_plan::long_points(4, long_ptr.data());
  EXPECT(longs.size() == 2 && longs[0] == 1 && longs[1] == 3);

  std::printf("color plan checks OK\n");
  return 0;
}
