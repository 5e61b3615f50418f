// sift_solvers.h -- what one lane of the SIFT kernels (sift.hip) evaluates, as __host__ __device__ code: VLFeat's
// approximations restated from thirdparty/VLFeat/mathop.h and sift.c, the refinement of one extremum, and one sample of
// the orientation and descriptor windows. Every float and double stands where the C code has it; nothing here calls a
// transcendental function.
#ifndef COLMAP_AMD_SIFT_SOLVERS_H_
#define COLMAP_AMD_SIFT_SOLVERS_H_

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SIFT_HD __host__ __device__ inline
#else
#define SIFT_HD inline
#endif

namespace sifts {

constexpr double kPi = 3.141592653589793;         // VL_PI
constexpr float kEpsF = 1.19209290E-07F;          // VL_EPSILON_F
constexpr double kEpsD = 2.220446049250313e-16;   // VL_EPSILON_D
constexpr int kExpnSize = 256;
constexpr double kExpnMax = 25.0;
constexpr int kOriBins = 36;
constexpr int kNBO = 8, kNBP = 4, kDescDim = kNBO * kNBP * kNBP;

SIFT_HD float mod_2pi_f(float x) {  // vl_mod_2pi_f
  while (x > (float)(2 * kPi)) x -= (float)(2 * kPi);
  while (x < 0.0F) x += (float)(2 * kPi);
  return x;
}

SIFT_HD long floor_f(float x) {  // vl_floor_f
  const long xi = (long)x;
  if (x >= 0 || (float)xi == x) return xi;
  return xi - 1;
}

SIFT_HD long floor_d(double x) {  // vl_floor_d
  const long xi = (long)x;
  if (x >= 0 || (double)xi == x) return xi;
  return xi - 1;
}

SIFT_HD float fast_atan2_f(float y, float x) {  // vl_fast_atan2_f
  float angle, r;
  const float c3 = 0.1821F;
  const float c1 = 0.9675F;
  const float abs_y = fabsf(y) + kEpsF;
  if (x >= 0) {
    r = (x - abs_y) / (x + abs_y);
    angle = (float)(kPi / 4);
  } else {
    r = (x + abs_y) / (abs_y - x);
    angle = (float)(3 * kPi / 4);
  }
  angle += (c3 * r * r - c1) * r;
  return (y < 0) ? -angle : angle;
}

SIFT_HD float fast_resqrt_f(float x) {  // vl_fast_resqrt_f
  const float xhalf = (float)0.5 * x;
  int32_t i;
  memcpy(&i, &x, 4);
  i = 0x5f3759df - (i >> 1);
  float u;
  memcpy(&u, &i, 4);
  u = u * ((float)1.5 - xhalf * u * u);
  u = u * ((float)1.5 - xhalf * u * u);
  return u;
}

SIFT_HD float fast_sqrt_f(float x) {  // vl_fast_sqrt_f
  return ((double)x < 1e-8) ? 0 : x * fast_resqrt_f(x);
}

SIFT_HD double fast_expn(const double* tab, double x) {  // fast_expn (sift.c:691-706)
  if (x > kExpnMax) return 0.0;
  x *= kExpnSize / kExpnMax;
  const int i = (int)floor_d(x);
  const double r = x - i;
  const double a = tab[i];
  const double b = tab[i + 1];
  return a + r * (b - a);
}

// SAVE_BACK of update_gradient (sift.c:1465-1468)
SIFT_HD void gradient_polar(float gx, float gy, float* mod, float* ang) {
  *mod = fast_sqrt_f(gx * gx + gy * gy);
  *ang = mod_2pi_f((float)((double)fast_atan2_f(gy, gx) + 2 * kPi));
}

// The refinement of one extremum (vl_sift_detect, sift.c:1267-1427). `dog` is the octave's DoG stack, [S + 2][h][w];
// (x, y, s_index) the candidate with s_index = is - s_min. The 3 x 3 system is held in named scalars and the pivot row
// is exchanged by selects: a private array under a run-time row index would live in scratch.
struct Refined {
  int32_t ix, iy, is, good;
  float x, y, s, pad;
  double sn;  // the refined scale index in double: the host computes sigma from it
};

SIFT_HD double sel3(int i, double a0, double a1, double a2) { return i == 0 ? a0 : i == 1 ? a1 : a2; }

SIFT_HD Refined refine(const float* dog, int w, int h, int s_min, int s_max, int x, int y, int s, double tp, double te,
                       double xper) {
  const long xo = 1, yo = w, so = (long)w * h;
  double Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dss = 0, Dxy = 0, Dxs = 0, Dys = 0;
  double b0 = 0, b1 = 0, b2 = 0;
  int dx = 0, dy = 0;
  const float* pt = dog;
  for (int iter = 0; iter < 5; ++iter) {
    x += dx;
    y += dy;
    pt = dog + xo * x + yo * y + so * (s - s_min);
#define SIFT_AT(dx_, dy_, ds_) (pt[(dx_) * xo + (dy_) * yo + (ds_) * so])
    Dx = 0.5 * (SIFT_AT(+1, 0, 0) - SIFT_AT(-1, 0, 0));
    Dy = 0.5 * (SIFT_AT(0, +1, 0) - SIFT_AT(0, -1, 0));
    Ds = 0.5 * (SIFT_AT(0, 0, +1) - SIFT_AT(0, 0, -1));
    Dxx = (SIFT_AT(+1, 0, 0) + SIFT_AT(-1, 0, 0) - 2.0 * SIFT_AT(0, 0, 0));
    Dyy = (SIFT_AT(0, +1, 0) + SIFT_AT(0, -1, 0) - 2.0 * SIFT_AT(0, 0, 0));
    Dss = (SIFT_AT(0, 0, +1) + SIFT_AT(0, 0, -1) - 2.0 * SIFT_AT(0, 0, 0));
    Dxy = 0.25 * (SIFT_AT(+1, +1, 0) + SIFT_AT(-1, -1, 0) - SIFT_AT(-1, +1, 0) - SIFT_AT(+1, -1, 0));
    Dxs = 0.25 * (SIFT_AT(+1, 0, +1) + SIFT_AT(-1, 0, -1) - SIFT_AT(-1, 0, +1) - SIFT_AT(+1, 0, -1));
    Dys = 0.25 * (SIFT_AT(0, +1, +1) + SIFT_AT(0, -1, -1) - SIFT_AT(0, -1, +1) - SIFT_AT(0, +1, -1));

    // A(i, j) = a<i><j>, row i, column j
    double a00 = Dxx, a11 = Dyy, a22 = Dss, a01 = Dxy, a10 = Dxy, a02 = Dxs, a20 = Dxs, a12 = Dys, a21 = Dys;
    b0 = -Dx;
    b1 = -Dy;
    b2 = -Ds;
    bool singular = false;
    // ---- j = 0
    {
      double maxa = 0, maxabsa = 0;
      int maxi = -1;
      if (fabs(a00) > maxabsa) { maxa = a00; maxabsa = fabs(a00); maxi = 0; }
      if (fabs(a10) > maxabsa) { maxa = a10; maxabsa = fabs(a10); maxi = 1; }
      if (fabs(a20) > maxabsa) { maxa = a20; maxabsa = fabs(a20); maxi = 2; }
      if (maxabsa < 1e-10f) {
        singular = true;
      } else {
        // swap row 0 with row maxi, normalise row 0
        const double r0 = sel3(maxi, a00, a10, a20), r1 = sel3(maxi, a01, a11, a21), r2 = sel3(maxi, a02, a12, a22);
        const double rb = sel3(maxi, b0, b1, b2);
        if (maxi == 1) { a10 = a00; a11 = a01; a12 = a02; b1 = b0; }
        if (maxi == 2) { a20 = a00; a21 = a01; a22 = a02; b2 = b0; }
        a00 = r0 / maxa; a01 = r1 / maxa; a02 = r2 / maxa; b0 = rb / maxa;
        double f = a10;
        a10 -= f * a00; a11 -= f * a01; a12 -= f * a02; b1 -= f * b0;
        f = a20;
        a20 -= f * a00; a21 -= f * a01; a22 -= f * a02; b2 -= f * b0;
      }
    }
    // ---- j = 1
    if (!singular) {
      double maxa = 0, maxabsa = 0;
      int maxi = -1;
      if (fabs(a11) > maxabsa) { maxa = a11; maxabsa = fabs(a11); maxi = 1; }
      if (fabs(a21) > maxabsa) { maxa = a21; maxabsa = fabs(a21); maxi = 2; }
      if (maxabsa < 1e-10f) {
        singular = true;
      } else {
        const double r1 = maxi == 1 ? a11 : a21, r2 = maxi == 1 ? a12 : a22, rb = maxi == 1 ? b1 : b2;
        if (maxi == 2) { a21 = a11; a22 = a12; b2 = b1; }
        a11 = r1 / maxa; a12 = r2 / maxa; b1 = rb / maxa;
        const double f = a21;
        a21 -= f * a11; a22 -= f * a12; b2 -= f * b1;
      }
    }
    // ---- j = 2
    if (!singular) {
      const double maxa = a22, maxabsa = fabs(a22);
      if (!(maxabsa > 0) || maxabsa < 1e-10f) {
        singular = true;
      } else {
        a22 = a22 / maxa;
        b2 = b2 / maxa;
      }
    }
    if (singular) {
      b0 = 0; b1 = 0; b2 = 0;
    }
    // backward substitution (runs after a singular break as well: on zeros)
    {
      double t = b2;
      b1 -= t * a12;
      b0 -= t * a02;
      t = b1;
      b0 -= t * a01;
    }
    dx = ((b0 > 0.6 && x < w - 2) ? 1 : 0) + ((b0 < -0.6 && x > 1) ? -1 : 0);
    dy = ((b1 > 0.6 && y < h - 2) ? 1 : 0) + ((b1 < -0.6 && y > 1) ? -1 : 0);
    if (dx == 0 && dy == 0) break;
  }
  Refined r;
  const double val = SIFT_AT(0, 0, 0) + 0.5 * (Dx * b0 + Dy * b1 + Ds * b2);
#undef SIFT_AT
  const double score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
  const double xn = x + b0;
  const double yn = y + b1;
  const double sn = s + b2;
  const bool good = fabs(val) > tp && score < (te + 1) * (te + 1) / te && score >= 0 && fabs(b0) < 1.5 && fabs(b1) < 1.5 &&
                    fabs(b2) < 1.5 && xn >= 0 && xn <= w - 1 && yn >= 0 && yn <= h - 1 && sn >= s_min && sn <= s_max;
  r.ix = x;
  r.iy = y;
  r.is = s;
  r.good = good ? 1 : 0;
  r.s = (float)sn;
  r.x = (float)(xn * xper);
  r.y = (float)(yn * xper);
  r.pad = 0.0f;
  r.sn = sn;
  return r;
}

// One sample of the orientation window (vl_sift_calc_keypoint_orientations, sift.c:1616-1651, bilinear form): the two
// bins it feeds and what it adds to each. false: outside the circular window.
SIFT_HD bool orientation_sample(const double* expn, double x, double y, double sigmaw, int W, int px, int py, float mod_f,
                                float ang_f, int* bin0, int* bin1, double* v0, double* v1) {
  const double dx = (double)px - x;
  const double dy = (double)py - y;
  const double r2 = dx * dx + dy * dy;
  if (r2 >= W * W + 0.6) return false;
  const double wgt = fast_expn(expn, r2 / (2 * sigmaw * sigmaw));
  const double mod = mod_f;
  const double ang = ang_f;
  const double fbin = kOriBins * ang / (2 * kPi);
  const int bin = (int)floor_d(fbin - 0.5);
  const double rbin = fbin - bin - 0.5;
  *bin0 = (bin + kOriBins) % kOriBins;
  *bin1 = (bin + 1) % kOriBins;
  *v0 = (1 - rbin) * mod * wgt;
  *v1 = (rbin)*mod * wgt;
  return true;
}

// One sample of the descriptor window (vl_sift_calc_keypoint_descriptor, sift.c:2012-2066): the lower-left bin and the
// eight weights in the order (dbinx, dbiny, dbint); a weight whose spatial bin is outside the 4 x 4 grid is not added
// (`inside` bit dbinx * 2 + dbiny).
struct DescSample {
  int binx, biny, bint;
  float wgt[8];
};

SIFT_HD DescSample descriptor_sample(const double* expn, double x, double y, double angle0, double st0, double ct0,
                                     double SBP, int px, int py, float mod, float angle) {
  DescSample d;
  const float theta = mod_2pi_f((float)((double)angle - angle0));
  const float dx = (float)((double)px - x);
  const float dy = (float)((double)py - y);
  const float nx = (float)((ct0 * dx + st0 * dy) / SBP);
  const float ny = (float)((-st0 * dx + ct0 * dy) / SBP);
  const float nt = (float)((double)(kNBO * theta) / (2 * kPi));
  const float wsigma = (float)(kNBP / 2);
  const float win = (float)fast_expn(expn, (double)(nx * nx + ny * ny) / (2.0 * wsigma * wsigma));
  d.binx = (int)floor_f((float)((double)nx - 0.5));
  d.biny = (int)floor_f((float)((double)ny - 0.5));
  d.bint = (int)floor_f(nt);
  const float rbinx = (float)((double)nx - (d.binx + 0.5));
  const float rbiny = (float)((double)ny - (d.biny + 0.5));
  const float rbint = nt - (float)d.bint;
  for (int dbinx = 0; dbinx < 2; ++dbinx)
    for (int dbiny = 0; dbiny < 2; ++dbiny)
      for (int dbint = 0; dbint < 2; ++dbint)
        d.wgt[dbinx * 4 + dbiny * 2 + dbint] = win * mod * fabsf((float)(1 - dbinx) - rbinx) * fabsf((float)(1 - dbiny) - rbiny) *
                                              fabsf((float)(1 - dbint) - rbint);
  return d;
}

}  // namespace sifts

#endif  // COLMAP_AMD_SIFT_SOLVERS_H_
