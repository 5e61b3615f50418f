// The C++ surface of SIFT extraction (include/colmap_amd/feature_extraction.hpp) from g++, linked against the library:
//   host      FeatureKeypoint and SiftExtractionOptions without a device
//   nodevice  creating an extractor without a GPU fails loudly (exit 2)
//   blob      on the GPU: one bright blob gives a keypoint at its centre with a descriptor of norm ~512
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "colmap_amd/feature_extraction.hpp"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

using namespace colmap_amd;

static void host() {
  FeatureKeypoint k(3.0f, 4.0f, 2.0f, 0.5f);
  EXPECT(k.a11 == 2.0f * std::cos(0.5f) && k.a21 == 2.0f * std::sin(0.5f) && k.a12 == -k.a21 && k.a22 == k.a11);
  EXPECT(std::fabs(k.ComputeScale() - 2.0f) < 1e-6f && std::fabs(k.ComputeOrientation() - 0.5f) < 1e-6f);
  k.Rescale(2.0f, 3.0f);
  EXPECT(k.x == 6.0f && k.y == 12.0f && k.a11 == 2.0f * (2.0f * std::cos(0.5f)) && k.a12 == 3.0f * -(2.0f * std::sin(0.5f)));
  try {
    k.Rescale(0.0f);
    EXPECT(false);
  } catch (const std::runtime_error&) {
  }
  SiftExtractionOptions o;
  std::string why;
  EXPECT(o.Check(&why) && why.empty());
  o.first_octave = -2;
  EXPECT(!o.Check(&why) && why.find("first_octave") != std::string::npos);
  o = SiftExtractionOptions();
  o.max_num_orientations = 0;
  EXPECT(!o.Check());
  std::printf("host OK\n");
}

static void blob() {
  const int w = 64, h = 48;
  std::vector<uint8_t> im((size_t)w * h);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const double d = ((x - 30.0) * (x - 30.0) + (y - 20.0) * (y - 20.0) * 1.6) / (2 * 3.0 * 3.0);
      im[(size_t)y * w + x] = (uint8_t)(100.0 + 120.0 * std::exp(-d) + 0.5);
    }
  auto extractor = CreateSiftFeatureExtractor();
  FeatureKeypoints kp;
  FeatureDescriptors desc;
  EXPECT(extractor->Extract(GreyBitmap{w, h, im.data()}, &kp, &desc));
  EXPECT(!kp.empty() && desc.rows == (int)kp.size() && desc.data.size() == kp.size() * 128);
  bool at_centre = false;
  for (size_t i = 0; i < kp.size(); ++i) {
    if (std::fabs(kp[i].x - 30.5f) < 1.0f && std::fabs(kp[i].y - 20.5f) < 1.0f && kp[i].ComputeScale() > 2.0f) at_centre = true;
    double n2 = 0;
    for (int k = 0; k < 128; ++k) n2 += (double)desc.row((int)i)[k] * desc.row((int)i)[k];
    EXPECT(std::sqrt(n2) > 440.0 && std::sqrt(n2) < 560.0);  // L1_ROOT descriptors have length 512 up to rounding
  }
  EXPECT(at_centre);
  FeatureKeypoints again;
  EXPECT(extractor->Extract(GreyBitmap{w, h, im.data()}, &again, nullptr) && again.size() == kp.size());
  try {
    extractor->Extract(GreyBitmap{0, 0, nullptr}, &kp, &desc);
    EXPECT(false);
  } catch (const std::runtime_error& e) {
    EXPECT(std::string(e.what()).find("1 x 1") != std::string::npos);
  }
  std::printf("blob OK\n");
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "nodevice";
  if (mode == "host") host();
  if (mode == "blob") blob();
  if (mode == "nodevice") {
    try {
      auto extractor = CreateSiftFeatureExtractor();
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 2;
    }
  }
  return 0;
}
