"""numpy checker of SIFT extraction: the reference's VLFeat route (SiftCPUFeatureExtractor::Extract, feature/sift.cc:138-341,
over thirdparty/VLFeat/sift.c, imopv.c, mathop.h) restated to be obviously right, with float32 and float64 exactly where
the C code has float and double. exp, pow, powf, sin and cos are the C library's, called through ctypes; everything else
is + - * / floor and VLFeat's own approximations.

Summation order: every histogram bin is ONE accumulator that takes its contributions in the raster order of the window
(np.add.at adds unbuffered, in index order), which is the reference's order and the device's.

extract(image, options) -> dict(octaves=[dict(o, w, h, levels, dog, num_candidates, det_i, det_f, sn, counts, angles,
float_desc, stats)], level_num_features, level_num_rows, keypoints, float_desc, descriptors, skip, num_out): the final
result is rows skip .. skip + num_out of keypoints / descriptors.
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

f32, f64 = np.float32, np.float64

_m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("exp", "sin", "cos", "sqrt"):
    getattr(_m, _n).restype = C.c_double
    getattr(_m, _n).argtypes = [C.c_double]
_m.pow.restype = C.c_double
_m.pow.argtypes = [C.c_double, C.c_double]
_m.powf.restype = C.c_float
_m.powf.argtypes = [C.c_float, C.c_float]

VL_PI = 3.141592653589793
EPS_F = f32(1.19209290E-07)
EPS_D = 2.220446049250313e-16
EXPN_SZ, EXPN_MAX = 256, 25.0
NBO, NBP = 8, 4


def c_exp(x):
    return _m.exp(float(x))


def c_pow(x, y):
    return _m.pow(float(x), float(y))


# ---------------------------------------------------------------------------------------------------------------------
# plan: geometry, sigmas, taps, table (vl_sift_new, _vl_sift_smooth, fast_expn_init)
# ---------------------------------------------------------------------------------------------------------------------
def shift_left(x, n):
    return x << n if n >= 0 else x >> -n


def geometry(width, height, o):
    S = o["octave_resolution"]
    O = o["num_octaves"]
    if O < 0:
        O = int(max(math.floor(math.log(min(width, height)) / 0.693147180559945) - o["first_octave"] - 3, 1))
    sigmak = c_pow(2.0, 1.0 / S)
    sigma0 = 1.6 * sigmak
    return dict(width=width, height=height, O=O, S=S, o_min=o["first_octave"], s_min=-1, s_max=S + 1, sigman=0.5,
                sigmak=sigmak, sigma0=sigma0, dsigma0=sigma0 * _m.sqrt(1.0 - 1.0 / (sigmak * sigmak)))


def num_octaves_run(g):
    n = 0
    while n < g["O"] and shift_left(g["width"], -(g["o_min"] + n)) >= 2 and shift_left(g["height"], -(g["o_min"] + n)) >= 2:
        n += 1
    return n


def base_smoothing(g, first):
    """sigma of the smoothing of level s_min, or None (the `sa > sb` tests of vl_sift_process_first/next_octave)."""
    if first:
        sa = g["sigma0"] * c_pow(g["sigmak"], g["s_min"])
        sb = g["sigman"] * c_pow(2.0, -g["o_min"])
    else:
        s_best = min(g["s_min"] + g["S"], g["s_max"])
        sa = g["sigma0"] * float(_m.powf(g["sigmak"], g["s_min"]))
        sb = g["sigma0"] * float(_m.powf(g["sigmak"], s_best - g["S"]))
    return _m.sqrt(sa * sa - sb * sb) if sa > sb else None


def level_sigma(g, s):
    return g["dsigma0"] * c_pow(g["sigmak"], s)


def gaussian_half_width(sigma):
    return int(max(math.ceil(4.0 * sigma), 1))


def gaussian_taps(sigma):
    W = gaussian_half_width(sigma)
    f = np.zeros(2 * W + 1, f32)
    acc = f32(0)
    for j in range(2 * W + 1):
        d = f32(j - W) / f32(sigma)
        f[j] = f32(c_exp(-0.5 * float(d * d)))
        acc = f32(acc + f[j])
    return f / acc


def expn_table():
    # 257 entries and one more, 0: x == 25 exactly reads entry 257 with weight 0 (past the end of VLFeat's own table)
    return np.array([c_exp(-float(k) * (EXPN_MAX / EXPN_SZ)) for k in range(EXPN_SZ + 1)] + [0.0], f64)


_EXPN = None


def fast_expn(x):
    """fast_expn on a float64 array."""
    global _EXPN
    if _EXPN is None:
        _EXPN = expn_table()
    x = np.asarray(x, f64)
    big = x > EXPN_MAX
    xs = np.where(big, 0.0, x) * (EXPN_SZ / EXPN_MAX)
    i = floor_to_int(xs)
    r = xs - i
    a, b = _EXPN[i], _EXPN[i + 1]
    return np.where(big, 0.0, a + r * (b - a))


# ---------------------------------------------------------------------------------------------------------------------
# mathop.h
# ---------------------------------------------------------------------------------------------------------------------
def floor_to_int(x):
    """vl_floor_f / vl_floor_d on an array."""
    xi = np.trunc(x).astype(np.int64)
    return np.where((x >= 0) | (xi.astype(x.dtype) == x), xi, xi - 1)


def mod_2pi_f(x):
    x = np.array(x, f32, copy=True)
    two_pi = f32(2 * VL_PI)
    while True:
        m = x > two_pi
        if not m.any():
            break
        x[m] = x[m] - two_pi
    while True:
        m = x < f32(0)
        if not m.any():
            break
        x[m] = x[m] + two_pi
    return x


def fast_atan2_f(y, x):
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    c3, c1 = f32(0.1821), f32(0.9675)
    abs_y = np.abs(y) + EPS_F
    pos = x >= 0
    with np.errstate(all="ignore"):
        r = np.where(pos, (x - abs_y) / (x + abs_y), (x + abs_y) / (abs_y - x)).astype(f32)
    angle = np.where(pos, f32(VL_PI / 4), f32(3 * VL_PI / 4)).astype(f32)
    angle = angle + (c3 * r * r - c1) * r
    return np.where(y < 0, -angle, angle).astype(f32)


def fast_resqrt_f(x):
    x = np.asarray(x, f32)
    xhalf = f32(0.5) * x
    i = np.int32(0x5f3759df) - (x.view(np.int32) >> 1)
    u = i.astype(np.int32).view(f32)
    u = u * (f32(1.5) - xhalf * u * u)
    u = u * (f32(1.5) - xhalf * u * u)
    return u


def fast_sqrt_f(x):
    x = np.atleast_1d(np.asarray(x, f32))
    with np.errstate(all="ignore"):
        return np.where(x.astype(f64) < 1e-8, f32(0), x * fast_resqrt_f(x)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# pyramid
# ---------------------------------------------------------------------------------------------------------------------
def upsample_rows(a):
    """copy_and_upsample_rows without its transpose: [h][w] -> [h][2w]."""
    h, w = a.shape
    out = np.zeros((h, 2 * w), f32)
    out[:, 0:2 * w - 1:2] = a
    out[:, 1:2 * w - 2:2] = (0.5 * (a[:, :-1] + a[:, 1:]).astype(f64)).astype(f32)  # a + b in float, 0.5 * in double
    out[:, 2 * w - 1] = a[:, w - 1]
    return out


def upsample2(im):
    return upsample_rows(upsample_rows(im).T.copy()).T.copy()


def decimate(a, step=2):
    """copy_and_downsample into an image floor(w / step) x floor(h / step)."""
    h, w = a.shape
    return a[0:(h // step) * step:step, 0:(w // step) * step:step].copy()


def conv_axis0(a, taps):
    """vl_imconvcol_vf with padding by continuity: one float accumulator per output, taps in ascending source index."""
    W = (len(taps) - 1) // 2
    h = a.shape[0]
    acc = np.zeros_like(a, dtype=f32)
    rows = np.arange(h)
    for t in range(2 * W + 1):
        src = np.clip(rows - W + t, 0, h - 1)
        acc = acc + a[src] * taps[t]
    return acc


def smooth(a, sigma):
    taps = gaussian_taps(sigma)
    return conv_axis0(conv_axis0(a, taps).T.copy(), taps).T.copy()  # columns first, then rows


# ---------------------------------------------------------------------------------------------------------------------
# detection and refinement (vl_sift_detect)
# ---------------------------------------------------------------------------------------------------------------------
def extrema(dog, tp):
    """(s_index, y, x) of the 26-neighbour extrema of the interior, in vl_sift_detect's order."""
    L, h, w = dog.shape
    if h < 3 or w < 3:
        return np.zeros((0, 3), np.int64)
    v = dog[1:L - 1, 1:h - 1, 1:w - 1]
    is_max = v.astype(f64) >= 0.8 * tp
    is_min = v.astype(f64) <= -0.8 * tp
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if ds == dy == dx == 0:
                    continue
                n = dog[1 + ds:L - 1 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                is_max &= v > n
                is_min &= v < n
    return np.argwhere(is_max | is_min) + 1  # C order: s, then y, then x


def refine(dog, x, y, s, g, tp, te, o_cur, stats):
    """One candidate; s is the level index (is). Returns None or (ix, iy, is, x, y, s as float32, sn as float)."""
    L, h, w = dog.shape
    s_min, s_max = g["s_min"], g["s_max"]
    xper = c_pow(2.0, o_cur)
    dx = dy = 0
    moved = False
    for it in range(5):
        x += dx
        y += dy
        moved = moved or dx != 0 or dy != 0

        def at(ax, ay, a_s):
            return dog[s - s_min + a_s, y + ay, x + ax]  # np.float32

        Dx = 0.5 * float(at(1, 0, 0) - at(-1, 0, 0))
        Dy = 0.5 * float(at(0, 1, 0) - at(0, -1, 0))
        Ds = 0.5 * float(at(0, 0, 1) - at(0, 0, -1))
        Dxx = float(at(1, 0, 0) + at(-1, 0, 0)) - 2.0 * float(at(0, 0, 0))
        Dyy = float(at(0, 1, 0) + at(0, -1, 0)) - 2.0 * float(at(0, 0, 0))
        Dss = float(at(0, 0, 1) + at(0, 0, -1)) - 2.0 * float(at(0, 0, 0))
        Dxy = 0.25 * float(at(1, 1, 0) + at(-1, -1, 0) - at(-1, 1, 0) - at(1, -1, 0))
        Dxs = 0.25 * float(at(1, 0, 1) + at(-1, 0, -1) - at(-1, 0, 1) - at(1, 0, -1))
        Dys = 0.25 * float(at(0, 1, 1) + at(0, -1, -1) - at(0, -1, 1) - at(0, 1, -1))
        A = [[Dxx, Dxy, Dxs], [Dxy, Dyy, Dys], [Dxs, Dys, Dss]]  # A[row][column]
        b = [-Dx, -Dy, -Ds]
        with np.errstate(all="ignore"):
            for j in range(3):
                maxa, maxabsa, maxi = 0.0, 0.0, -1
                for i in range(j, 3):
                    if abs(A[i][j]) > maxabsa:
                        maxa, maxabsa, maxi = A[i][j], abs(A[i][j]), i
                if maxabsa < float(f32(1e-10)):
                    b = [0.0, 0.0, 0.0]
                    stats["singular"] += 1
                    break
                i = maxi
                for jj in range(j, 3):
                    A[i][jj], A[j][jj] = A[j][jj], A[i][jj]
                    A[j][jj] = float(f64(A[j][jj]) / f64(maxa))
                b[j], b[i] = b[i], b[j]
                b[j] = float(f64(b[j]) / f64(maxa))
                for ii in range(j + 1, 3):
                    xx = A[ii][j]
                    for jj in range(j, 3):
                        A[ii][jj] -= xx * A[j][jj]
                    b[ii] -= xx * b[j]
            for i in (2, 1):
                xx = b[i]
                for ii in range(i - 1, -1, -1):
                    b[ii] -= xx * A[ii][i]
        dx = (1 if (b[0] > 0.6 and x < w - 2) else 0) + (-1 if (b[0] < -0.6 and x > 1) else 0)
        dy = (1 if (b[1] > 0.6 and y < h - 2) else 0) + (-1 if (b[1] < -0.6 and y > 1) else 0)
        if dx == 0 and dy == 0:
            break
    if moved:
        stats["moved"] += 1
    val = float(dog[s - s_min, y, x]) + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2])
    with np.errstate(all="ignore"):
        score = float(f64((Dxx + Dyy) * (Dxx + Dyy)) / f64(Dxx * Dyy - Dxy * Dxy))
    xn, yn, sn = x + b[0], y + b[1], s + b[2]
    tests = (("peak", abs(val) > tp), ("edge", score < (te + 1) * (te + 1) / te and score >= 0),
             ("offset", abs(b[0]) < 1.5 and abs(b[1]) < 1.5 and abs(b[2]) < 1.5),
             ("xy_range", 0 <= xn <= w - 1 and 0 <= yn <= h - 1), ("s_range", s_min <= sn <= s_max))
    good = True
    for name, ok in tests:
        if not ok:
            stats["rejected_" + name] += 1
            good = False
    if not good:
        return None
    return x, y, s, f32(xn * xper), f32(yn * xper), f32(sn), sn


# ---------------------------------------------------------------------------------------------------------------------
# gradient, orientations, descriptors
# ---------------------------------------------------------------------------------------------------------------------
def gradient(level):
    """update_gradient for one level: (modulus, angle) float32 planes."""
    a = level
    gx = np.zeros_like(a)
    gy = np.zeros_like(a)
    gx[:, 1:-1] = (0.5 * (a[:, 2:] - a[:, :-2]).astype(f64)).astype(f32)
    gx[:, 0] = a[:, 1] - a[:, 0]
    gx[:, -1] = a[:, -1] - a[:, -2]
    gy[1:-1, :] = (0.5 * (a[2:, :] - a[:-2, :]).astype(f64)).astype(f32)
    gy[0, :] = a[1, :] - a[0, :]
    gy[-1, :] = a[-1, :] - a[-2, :]
    mod = fast_sqrt_f((gx * gx + gy * gy).ravel()).reshape(a.shape)
    ang = mod_2pi_f((fast_atan2_f(gy, gx).astype(f64) + 2 * VL_PI).astype(f32))
    return mod, ang


def orientations(grad, g, det, o_cur):
    """vl_sift_calc_keypoint_orientations (bilinear form): (count, [4] angles)."""
    ix, iy, si, kx, ky, ks, ksigma = det
    mod_p, ang_p = grad[si - g["s_min"] - 1]
    h, w = mod_p.shape
    xper = c_pow(2.0, o_cur)
    x, y, sigma = float(kx) / xper, float(ky) / xper, float(ksigma) / xper
    xi, yi = int(x + 0.5), int(y + 0.5)
    sigmaw = 1.5 * sigma
    W = int(max(math.floor(3.0 * sigmaw), 1))
    nbins = 36
    if xi < 0 or xi > w - 1 or yi < 0 or yi > h - 1 or si < g["s_min"] + 1 or si > g["s_max"] - 2:
        return 0, [0.0] * 4
    ys = np.arange(max(-W, -yi), min(W, h - 1 - yi) + 1)
    xs = np.arange(max(-W, -xi), min(W, w - 1 - xi) + 1)
    YS, XS = np.meshgrid(ys, xs, indexing="ij")  # raster order: ys outer, xs inner
    YS, XS = YS.ravel(), XS.ravel()
    dx = (xi + XS).astype(f64) - x
    dy = (yi + YS).astype(f64) - y
    r2 = dx * dx + dy * dy
    keep = ~(r2 >= W * W + 0.6)
    YS, XS, r2 = YS[keep], XS[keep], r2[keep]
    wgt = fast_expn(r2 / (2 * sigmaw * sigmaw))
    mod = mod_p[yi + YS, xi + XS].astype(f64)
    ang = ang_p[yi + YS, xi + XS].astype(f64)
    fbin = nbins * ang / (2 * VL_PI)
    b = floor_to_int(fbin - 0.5)
    rbin = fbin - b - 0.5
    hist = np.zeros(nbins, f64)
    idx = np.stack([(b + nbins) % nbins, (b + 1) % nbins], 1).ravel()
    val = np.stack([(1 - rbin) * mod * wgt, rbin * mod * wgt], 1).ravel()
    np.add.at(hist, idx, val)
    hist = [float(v) for v in hist]
    for it in range(6):
        prev, first = hist[nbins - 1], hist[0]
        for i in range(nbins - 1):
            newh = (prev + hist[i] + hist[(i + 1) % nbins]) / 3.0
            prev = hist[i]
            hist[i] = newh
        hist[nbins - 1] = (prev + hist[nbins - 1] + first) / 3.0
    maxh = 0.0
    for v in hist:
        maxh = max(maxh, v)
    angles = []
    for i in range(nbins):
        h0, hm, hp = hist[i], hist[(i - 1 + nbins) % nbins], hist[(i + 1 + nbins) % nbins]
        if h0 > 0.8 * maxh and h0 > hm and h0 > hp:
            di = -0.5 * (hp - hm) / (hp + hm - 2 * h0)
            angles.append(2 * VL_PI * (i + di + 0.5) / nbins)
            if len(angles) == 4:
                break
    return len(angles), angles + [0.0] * (4 - len(angles))


def sequential_sum_f32(v):
    return np.cumsum(v, dtype=f32)[-1]  # cumsum adds left to right in float32


def normalize_histogram(d):
    norm = sequential_sum_f32(d * d)
    norm = f32(fast_sqrt_f(norm)[0] + EPS_F)
    return (d / norm).astype(f32)


def descriptor(grad, g, det, angle0, o_cur):
    """vl_sift_calc_keypoint_descriptor: [128] float32 in VLFeat's bin order, or None where the reference returns early."""
    ix, iy, si, kx, ky, ks, ksigma = det
    mod_p, ang_p = grad[si - g["s_min"] - 1]
    h, w = mod_p.shape
    xper = c_pow(2.0, o_cur)
    x, y, sigma = float(kx) / xper, float(ky) / xper, float(ksigma) / xper
    xi, yi = int(x + 0.5), int(y + 0.5)
    st0, ct0 = _m.sin(float(angle0)), _m.cos(float(angle0))
    SBP = 3.0 * sigma + EPS_D
    W = int(math.floor(_m.sqrt(2.0) * SBP * (NBP + 1) / 2.0 + 0.5))
    if xi < 0 or xi >= w or yi < 0 or yi >= h - 1 or si < g["s_min"] + 1 or si > g["s_max"] - 2:
        return None
    descr = np.zeros(NBO * NBP * NBP, f32)
    dys = np.arange(max(-W, 1 - yi), min(W, h - yi - 2) + 1)
    dxs = np.arange(max(-W, 1 - xi), min(W, w - xi - 2) + 1)
    if len(dys) and len(dxs):
        DY, DX = np.meshgrid(dys, dxs, indexing="ij")
        DY, DX = DY.ravel(), DX.ravel()
        mod = mod_p[yi + DY, xi + DX]
        angle = ang_p[yi + DY, xi + DX]
        theta = mod_2pi_f((angle.astype(f64) - angle0).astype(f32))
        dx = ((xi + DX).astype(f64) - x).astype(f32)
        dy = ((yi + DY).astype(f64) - y).astype(f32)
        nx = ((ct0 * dx.astype(f64) + st0 * dy.astype(f64)) / SBP).astype(f32)
        ny = ((-st0 * dx.astype(f64) + ct0 * dy.astype(f64)) / SBP).astype(f32)
        nt = ((f32(NBO) * theta).astype(f64) / (2 * VL_PI)).astype(f32)
        wsigma = f32(NBP / 2)
        win = fast_expn((nx * nx + ny * ny).astype(f64) / (2.0 * float(wsigma) * float(wsigma))).astype(f32)
        binx = floor_to_int((nx.astype(f64) - 0.5).astype(f32))
        biny = floor_to_int((ny.astype(f64) - 0.5).astype(f32))
        bint = floor_to_int(nt)
        rbinx = (nx.astype(f64) - (binx + 0.5)).astype(f32)
        rbiny = (ny.astype(f64) - (biny + 0.5)).astype(f32)
        rbint = nt - bint.astype(f32)
        idx, val = [], []
        for dbinx in (0, 1):
            for dbiny in (0, 1):
                for dbint in (0, 1):
                    ok = (binx + dbinx >= -(NBP // 2)) & (binx + dbinx < NBP // 2) & (biny + dbiny >= -(NBP // 2)) & (biny + dbiny < NBP // 2)
                    weight = win * mod * np.abs(f32(1 - dbinx) - rbinx) * np.abs(f32(1 - dbiny) - rbiny) * np.abs(f32(1 - dbint) - rbint)
                    where = ((bint + dbint) % NBO) + (biny + dbiny + NBP // 2) * (NBO * NBP) + (binx + dbinx + NBP // 2) * NBO
                    idx.append(np.where(ok, where, -1))
                    val.append(weight.astype(f32))
        idx = np.stack(idx, 1).ravel()  # sample-major, then (dbinx, dbiny, dbint): the order of the C loops
        val = np.stack(val, 1).ravel()
        m = idx >= 0
        np.add.at(descr, idx[m], val[m])
    descr = normalize_histogram(descr)
    descr = np.where(descr.astype(f64) > 0.2, f32(0.2), descr).astype(f32)
    return normalize_histogram(descr)


def to_bytes(d, normalization):
    """L1_ROOT / L2 with sequential sums, then FeatureDescriptorsToUnsignedByte (feature/utils.cc:45-69)."""
    d = d.astype(f32)
    if normalization == 1:
        z = sequential_sum_f32(d * d)
        if z > 0:
            d = (d / np.sqrt(z, dtype=f32)).astype(f32)
    else:
        l1 = sequential_sum_f32(np.abs(d))
        with np.errstate(all="ignore"):
            inv = f32(1) / l1
            d = np.sqrt(d * inv, dtype=f32)
    scaled = (f32(512.0) * d).astype(f32)
    r = np.where(scaled >= 0,  # std::round: halves away from zero
                 np.floor(scaled.astype(f64) + 0.5), -np.floor(-scaled.astype(f64) + 0.5))
    return np.clip(r, 0, 255).astype(np.uint8)


UBC = np.array([(k & ~7) | ((8 - (k & 7)) & 7) for k in range(128)])


def cut_levels(level_num_features, level_num_rows, max_num_features):
    first, nf, nout = 0, 0, 0
    for i in range(len(level_num_rows) - 1, -1, -1):
        nf += level_num_features[i]
        nout += level_num_rows[i]
        if nf > max_num_features:
            first = i
            break
    return first, nout


# ---------------------------------------------------------------------------------------------------------------------
def extract(image, o, want_descriptors=True):
    image = np.asarray(image)
    h0, w0 = image.shape
    g = geometry(w0, h0, o)
    im = image.astype(f32) / f32(255.0)
    tp, te = float(o["peak_threshold"]), float(o["edge_threshold"])
    S = g["S"]
    out = dict(octaves=[], geometry=g)
    level_num_features, level_num_rows = [], []
    all_kp, all_fd, all_desc = [], [], []
    prev_levels = None
    for k in range(num_octaves_run(g)):
        o_cur = g["o_min"] + k
        if k == 0:
            base = upsample2(im) if g["o_min"] < 0 else decimate(im, 1 << g["o_min"])
        else:
            base = decimate(prev_levels[min(g["s_min"] + S, g["s_max"]) - g["s_min"]])
        sd = base_smoothing(g, k == 0)
        if sd is not None:
            base = smooth(base, sd)
        levels = [base]
        for s in range(g["s_min"] + 1, g["s_max"] + 1):
            levels.append(smooth(levels[-1], level_sigma(g, s)))
        levels = np.stack(levels)
        prev_levels = levels
        dog = levels[1:] - levels[:-1]
        cand = extrema(dog, tp)
        stats = dict(moved=0, singular=0, rejected_peak=0, rejected_edge=0, rejected_offset=0, rejected_xy_range=0, rejected_s_range=0)
        dets = []
        for si, y, x in cand:
            r = refine(dog, int(x), int(y), int(si) + g["s_min"], g, tp, te, o_cur, stats)
            if r is not None:
                ix, iy, is_, fx, fy, fs, sn = r
                sigma = f32(g["sigma0"] * c_pow(2.0, sn / S) * c_pow(2.0, o_cur))
                dets.append((ix, iy, is_, fx, fy, fs, sigma, sn))
        hh, ww = base.shape
        oc = dict(o=o_cur, w=ww, h=hh, levels=levels, dog=dog, num_candidates=len(cand), stats=stats,
                  det_i=np.array([[o_cur, d[0], d[1], d[2]] for d in dets], np.int32).reshape(-1, 4),
                  det_f=np.array([[d[3], d[4], d[5], d[6]] for d in dets], f32).reshape(-1, 4),
                  sn=np.array([d[7] for d in dets], f64))
        counts, angles, fdesc = [], [], []
        grad = None
        if dets:
            grad = [gradient(levels[s - g["s_min"]]) for s in range(g["s_min"] + 1, g["s_max"] - 1)]
            oc["gradient"] = grad
        prev_level = -1
        for d in dets:
            det = d[:7]
            if o["upright"]:
                n, a = 1, [0.0, 0.0, 0.0, 0.0]
            else:
                n, a = orientations(grad, g, det, o_cur)
            counts.append(n)
            angles.append(a)
            if d[2] != prev_level:
                level_num_features.append(0)
                level_num_rows.append(0)
            level_num_features[-1] += 1
            prev_level = d[2]
            for j in range(min(n, o["max_num_orientations"])):
                all_kp.append([f32(d[3] + f32(0.5)), f32(d[4] + f32(0.5)), d[6], f32(a[j])])
                level_num_rows[-1] += 1
                if want_descriptors:
                    fd = descriptor(grad, g, det, a[j], o_cur)
                    if fd is None:  # the reference keeps the bytes of the row before; the device writes zeros
                        fd = np.zeros(128, f32)
                        all_desc.append(np.zeros(128, np.uint8))
                    else:
                        ubc = np.zeros(128, np.uint8)
                        ubc[UBC] = to_bytes(fd, o["normalization"])  # TransformVLFeatToUBCFeatureDescriptors
                        all_desc.append(ubc)
                    fdesc.append(fd)
                    all_fd.append(fd)
        oc["counts"] = np.array(counts, np.int32)
        oc["angles"] = np.array(angles, f64).reshape(-1, 4)
        oc["float_desc"] = np.array(fdesc, f32).reshape(-1, 128)
        out["octaves"].append(oc)
    first, nout = cut_levels(level_num_features, level_num_rows, o["max_num_features"])
    out["level_num_features"] = np.array(level_num_features, np.int32)
    out["level_num_rows"] = np.array(level_num_rows, np.int32)
    out["skip"] = int(sum(level_num_rows[:first]))
    out["num_out"] = int(nout)
    out["keypoints"] = np.array(all_kp, f32).reshape(-1, 4)
    out["float_desc"] = np.array(all_fd, f32).reshape(-1, 128)
    out["descriptors"] = np.array(all_desc, np.uint8).reshape(-1, 128)
    return out
