// The task classes of the 11 x 11 wave kernels (colmap_amd/csrc/pm_patch_class.h) without a GPU: for every centred
// homography that patch_outside accepts, the per-tap arithmetic of ncc_front<false> (pm_kernels.hip), restated here
// with fmaf in the same order, must give finite coordinates for all 128 tap slots of the 16 lanes and clamp every one of
// the 121 taps to an all-zero entry of the packed image's ring. Random and adversarial homographies: divisors at both
// bounds, huge and cancelling terms, corners on the margin, infinities, NaNs and raw bit patterns.
//   g++ -std=c++17 -ffp-contract=off -I include -I colmap_amd/csrc tests/cpp/test_pm_patch_class.cc
#include "pm_patch_class.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

using colmap_amd::PmParams;
using colmap_amd::kFpRingX;
using colmap_amd::kFpRingY;

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (++g_fail < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

PmParams Shape(int w, int h, int radius, int step) {
  PmParams p{};
  p.src_w = w;
  p.src_h = h;
  p.radius = radius;
  p.step = step;
  p.fp_xmax = (float)(w + kFpRingX);
  p.fp_ymax = (float)(h + kFpRingY);
  return p;
}

float Med3(float v, float lo, float hi) { return std::fmin(std::fmax(v, lo), hi); }  // v is finite where this is used

// ncc_front<false>, all 16 lanes of a task's group: true when every coordinate is finite and every tap reads zeros.
// `transpose`: the tap order of the odd sweep directions (tap_tables_init).
bool TapsAllZeroRing(const PmParams& p, const float H[9], bool transpose, const char** why) {
  for (int j = 0; j < 16; ++j) {
    float csrc[8], rsrc[8], zz[8], pre[8], suf[8];
    bool valid[8];
    float run = 1.0f;
    for (int k = 0; k < 8; ++k) {
      const int t = j + 16 * k;
      valid[k] = t < 121;
      const int tt = valid[k] ? t : 0;
      int wrow = tt / 11, wcol = tt - wrow * 11;
      if (transpose) std::swap(wrow, wcol);
      const float dx = (float)(wcol * p.step), dy = (float)(wrow * p.step);
      csrc[k] = fmaf(H[0], dx, fmaf(H[1], dy, H[2]));
      rsrc[k] = fmaf(H[3], dx, fmaf(H[4], dy, H[5]));
      const float z = fmaf(H[6], dx, fmaf(H[7], dy, H[8]));
      zz[k] = valid[k] ? z : 1.0f;
      pre[k] = run;
      run = run * zz[k];
    }
    const float rinv = 1.0f / run;
    float sfx = 1.0f;
    for (int k = 7; k >= 0; --k) {
      suf[k] = sfx;
      sfx = sfx * zz[k];
    }
    if (!std::isfinite(run) || !std::isfinite(rinv) || run == 0.0f) {
      *why = "shared division";
      return false;
    }
    for (int k = 0; k < 8; ++k) {
      const float inv_z = (pre[k] * suf[k]) * rinv;
      const float px = inv_z * csrc[k], py = inv_z * rsrc[k];
      const float fx = floorf(px), fy = floorf(py);
      const float wx = px - fx, wy = py - fy;
      if (!std::isfinite(inv_z) || !std::isfinite(px) || !std::isfinite(py) || !std::isfinite(wx) || !std::isfinite(wy)) {
        *why = "coordinate not finite";
        return false;
      }
      if (!valid[k]) continue;  // (the kernel zeroes the texel of a slot beyond the window; its fraction must be finite)
      const int ix = (int)Med3(fx + (float)kFpRingX, (float)(kFpRingX - 2), p.fp_xmax);
      const int iy = (int)Med3(fy + (float)kFpRingY, (float)(kFpRingY - 2), p.fp_ymax);
      const bool zero = ix == kFpRingX - 2 || ix == p.src_w + kFpRingX || iy == kFpRingY - 2 || iy == p.src_h + kFpRingY;
      if (!zero) {
        *why = "tap reads an entry with texels";
        return false;
      }
    }
  }
  return true;
}

float FromBits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

float Nudge(float v, int ulps) {
  for (int i = 0; i < std::abs(ulps); ++i) v = std::nextafterf(v, ulps > 0 ? INFINITY : -INFINITY);
  return v;
}

struct Tally {
  long long drawn = 0, accepted = 0;
};

std::mt19937_64 rng(20260711);
double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
int I(int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); }

void Check(const PmParams& p, const float H[9], Tally& t) {
  ++t.drawn;
  if (!colmap_amd::patch_outside(p, H)) return;
  ++t.accepted;
  EXPECT(!colmap_amd::patch_inside(p, H));  // the classes are disjoint
  EXPECT(colmap_amd::patch_answered(p, H, 0.5f, 0.5f));
  for (int tr = 0; tr < 2; ++tr) {
    const char* why = "";
    if (!TapsAllZeroRing(p, H, tr != 0, &why)) {
      if (++g_fail < 20)
        std::printf("FAILED: accepted, but %s: w %d h %d r %d step %d H = %a %a %a  %a %a %a  %a %a %a\n", why, p.src_w,
                    p.src_h, p.radius, p.step, H[0], H[1], H[2], H[3], H[4], H[5], H[6], H[7], H[8]);
    }
  }
}

PmParams RandomShape() {
  static const int sizes[] = {8, 31, 64, 640, 1920, 2560, 8191, 8192};
  const int r = I(0, 3) == 0 ? 10 : 5;  // 11 taps a side either way: radius 5 step 1, or radius 10 step 2
  return Shape(sizes[I(0, 7)], sizes[I(0, 7)], r, r == 10 ? 2 : 1);
}

// a homography whose window lies beside edge `edge` (0 left, 1 right, 2 above, 3 below) by `gap` texels at divisor z0
void Beside(const PmParams& p, int edge, double gap, double z0, double skew, float H[9]) {
  const double e = 2.0 * p.radius;
  const double zx = U(-skew, skew) / e, zy = U(-skew, skew) / e;  // divisor slopes
  const double sx = U(0.2, 3.0), sy = U(0.2, 3.0), sh = U(-0.5, 0.5);
  // affine placement in texels, then multiplied by the divisor at the origin (projective part small)
  double ox = U(-2.0 * p.src_w, 3.0 * p.src_w), oy = U(-2.0 * p.src_h, 3.0 * p.src_h);
  const double ext = e * (sx + std::fabs(sh)) + 1.0, eyt = e * (sy + std::fabs(sh)) + 1.0;
  if (edge == 0) ox = -1.0 - gap - ext;
  if (edge == 1) ox = p.src_w + gap;
  if (edge == 2) oy = -1.0 - gap - eyt;
  if (edge == 3) oy = p.src_h + gap;
  H[0] = (float)(sx * z0); H[1] = (float)(sh * z0); H[2] = (float)(ox * z0);
  H[3] = (float)(sh * z0); H[4] = (float)(sy * z0); H[5] = (float)(oy * z0);
  H[6] = (float)zx; H[7] = (float)zy; H[8] = (float)z0;
}

}  // namespace

int main() {
  Tally plain, zbound, margin, huge, special, bits;
  const float kInf = std::numeric_limits<float>::infinity(), kNaN = std::numeric_limits<float>::quiet_NaN();
  float H[9];

  // 1. patches beside an edge at ordinary divisors, gaps from 0 to far
  for (int n = 0; n < 300000; ++n) {
    const PmParams p = RandomShape();
    Beside(p, I(0, 3), I(0, 2) ? U(0.0, 40.0) : U(0.0, 5000.0), U(0.3, 3.0), 0.2, H);
    Check(p, H, plain);
  }
  // 2. divisors at both bounds: origin divisor within a few ulps of 1/16 or 16, slopes of either sign
  for (int n = 0; n < 200000; ++n) {
    const PmParams p = RandomShape();
    const bool low = I(0, 1) != 0;
    Beside(p, I(0, 3), U(8.0, 200.0), low ? 0.0625 : 16.0, 0.0, H);
    const float slope = (float)(U(0.0, 1.0) < 0.5 ? 0.0 : U(-1e-3, 1e-3));
    H[6] = low ? std::fabs(slope) : -std::fabs(slope);
    H[7] = I(0, 1) ? H[6] : 0.0f;
    if (I(0, 3) == 0) { H[6] = -H[6]; H[7] = -H[7]; }  // corners across the bound: must be refused
    H[8] = Nudge(H[8], I(-3, 3));
    Check(p, H, zbound);
  }
  // 3. corners on the margin: the nearest corner within a few ulps of (1 + m) z, (w + m) z
  for (int n = 0; n < 200000; ++n) {
    const PmParams p = RandomShape();
    const int edge = I(0, 3);
    const double z0 = I(0, 1) ? U(0.0625, 0.07) : U(0.07, 16.0);
    Beside(p, edge, colmap_amd::kAnsMargin, z0, 0.0, H);
    H[1] = H[3] = 0.0f;  // axis-aligned: corner 0 or 3 is the nearest, placed on the margin below
    const float e = (float)(2 * p.radius);
    if (edge == 0) H[2] = Nudge(-(1.0f + colmap_amd::kAnsMargin) * H[8] - H[0] * e, I(-4, 4));
    if (edge == 1) H[2] = Nudge(((float)p.src_w + colmap_amd::kAnsMargin) * H[8], I(-4, 4));
    if (edge == 2) H[5] = Nudge(-(1.0f + colmap_amd::kAnsMargin) * H[8] - H[4] * e, I(-4, 4));
    if (edge == 3) H[5] = Nudge(((float)p.src_h + colmap_amd::kAnsMargin) * H[8], I(-4, 4));
    Check(p, H, margin);
  }
  // 4. huge and cancelling terms: edge vectors and origin around the term bound and far beyond it, opposite signs
  for (int n = 0; n < 200000; ++n) {
    const PmParams p = RandomShape();
    Beside(p, I(0, 3), U(8.0, 100.0), U(0.1, 10.0), 0.1, H);
    const float e = (float)(2 * p.radius);
    const float big = I(0, 2) ? Nudge(colmap_amd::kAnsTerm, I(-2, 2)) : std::ldexp(1.0f, I(10, 120));
    const int row = 3 * I(0, 2);
    const float sgn = I(0, 1) ? 1.0f : -1.0f;
    switch (I(0, 3)) {
      case 0: H[row + 0] = sgn * big / e; H[row + 2] = -sgn * big; break;          // a cancels the origin
      case 1: H[row + 0] = sgn * big / e; H[row + 1] = -sgn * big / e; break;      // a cancels b
      case 2: H[row + 2] = sgn * big; break;
      default: H[row + 1] = sgn * big / e; H[row + 2] = -sgn * big * 0.5f; break;
    }
    Check(p, H, huge);
  }
  // 5. infinities, NaNs, zeros, denormals in one or two entries of an otherwise accepted homography
  for (int n = 0; n < 100000; ++n) {
    const PmParams p = RandomShape();
    Beside(p, I(0, 3), U(8.0, 100.0), U(0.3, 3.0), 0.1, H);
    const float sp[] = {kInf, -kInf, kNaN, 0.0f, -0.0f, 1e-42f, -1e-42f, 3.4e38f, -3.4e38f};
    for (int m = I(1, 2); m > 0; --m) H[I(0, 8)] = sp[I(0, 8)];
    Check(p, H, special);
  }
  // 6. raw bit patterns
  for (int n = 0; n < 100000; ++n) {
    const PmParams p = RandomShape();
    for (int k = 0; k < 9; ++k) H[k] = FromBits((uint32_t)rng());
    Check(p, H, bits);
  }
  // images beyond the size the bound was derived for are refused
  {
    PmParams p = Shape(8193, 100, 5, 1);
    Beside(p, 1, 100.0, 1.0, 0.0, H);
    EXPECT(!colmap_amd::patch_outside(p, H));
    p = Shape(100, 100, 5, 1);
    Beside(p, 1, 100.0, 1.0, 0.0, H);
    EXPECT(colmap_amd::patch_outside(p, H));
  }
  // the flat-reference rule is ncc_finish's own expression
  for (int n = 0; n < 100000; ++n) {
    const float s = (float)U(0.0, 1.0), q = I(0, 1) ? s * s + (float)U(-2e-5, 2e-5) : (float)U(0.0, 1.0);
    const float ref_var = q - s * s;
    EXPECT(colmap_amd::ref_flat(s, q) == (ref_var < 1e-5f));
    for (int k = 0; k < 9; ++k) H[k] = kNaN;
    EXPECT(colmap_amd::patch_answered(Shape(64, 64, 5, 1), H, s, q) == (ref_var < 1e-5f));
  }
  EXPECT(!colmap_amd::ref_flat(kNaN, 0.5f));

  const Tally* all[] = {&plain, &zbound, &margin, &huge, &special, &bits};
  const char* names[] = {"beside", "divisor bounds", "margin", "huge terms", "special values", "bit patterns"};
  long long drawn = 0, accepted = 0;
  for (int i = 0; i < 6; ++i) {
    std::printf("%-16s drawn %8lld accepted %8lld\n", names[i], all[i]->drawn, all[i]->accepted);
    drawn += all[i]->drawn;
    accepted += all[i]->accepted;
  }
  EXPECT(drawn >= 1000000);
  // both sets are non-empty, in every adversarial family that is built around an accepted homography
  for (int i = 0; i < 5; ++i) EXPECT(all[i]->accepted > 0 && all[i]->accepted < all[i]->drawn);
  EXPECT(bits.accepted < bits.drawn);
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("pm patch class checks OK (%lld homographies, %lld accepted)\n", drawn, accepted);
  return 0;
}
