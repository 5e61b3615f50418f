"""CPU checker of image undistortion (tests only): numpy in double precision, written from the reference's sources
(sensor/models.h, image/undistortion.cc, image/warp.cc, sensor/bitmap.cc) and not from colmap_amd/csrc/undistort*.

What is independent of the library under test:
  * the forward models are vectorised numpy in the reference's order of operations (exact agreement is expected for the
    models without a transcendental function);
  * the Newton iteration of IterativeUndistortion takes its Jacobian from COMPLEX-STEP differentiation of the forward
    distortion (exact to rounding, like the reference's Jets), where the library uses hand-derived Jacobians;
  * the warp is a gather over whole arrays, the resize a pair of dense weight matrices.
It also reports, per output pixel, how close the interpolant is to a rounding boundary and how close the source
coordinate is to a pixel boundary: the two situations in which device libm vs host libm may legitimately flip a pixel by
one."""
from __future__ import annotations

import numpy as np

SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, FULL_OPENCV, FOV = range(8)
SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE, THIN_PRISM_FISHEYE, RAD_TAN_THIN_PRISM_FISHEYE = 8, 9, 10, 11
SIMPLE_DIVISION, DIVISION, SIMPLE_FISHEYE, FISHEYE, EUCM, EQUIRECTANGULAR = 12, 13, 14, 15, 16, 17
ONE_FOCAL = (SIMPLE_PINHOLE, SIMPLE_RADIAL, RADIAL, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE, SIMPLE_DIVISION, SIMPLE_FISHEYE)
FISHEYES = (OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE, THIN_PRISM_FISHEYE, RAD_TAN_THIN_PRISM_FISHEYE,
            SIMPLE_FISHEYE, FISHEYE)
ITERATIVE = (SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, FULL_OPENCV, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE,
             THIN_PRISM_FISHEYE, RAD_TAN_THIN_PRISM_FISHEYE)
# models whose forward projection uses no transcendental function (sqrt and division are correctly rounded everywhere)
NO_TRANSCENDENTAL = (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV, SIMPLE_DIVISION, DIVISION, EUCM)
EPS = np.finfo(np.float64).eps


class Camera:
    def __init__(self, model_id, width, height, params, camera_id=0):
        self.model_id, self.width, self.height = int(model_id), int(width), int(height)
        self.params = np.asarray(params, np.float64).copy()
        self.camera_id = camera_id

    def __repr__(self):
        return f"Camera({self.model_id}, {self.width}x{self.height}, {self.params.tolist()})"


def split(model, p):
    """(f1, f2, c1, c2, extra)"""
    if model in ONE_FOCAL:
        return p[0], p[0], p[1], p[2], p[3:]
    return p[0], p[1], p[2], p[3], p[4:]


def distortion(model, e, u, v):
    """CameraModel::Distortion (sensor/models.h), real or complex arrays."""
    u2, uv, v2 = u * u, u * v, v * v
    r2 = u2 + v2
    if model in (SIMPLE_RADIAL, SIMPLE_RADIAL_FISHEYE):
        radial = e[0] * r2
        return u * radial, v * radial
    if model == RADIAL:
        radial = e[0] * r2 + e[1] * r2 * r2
        return u * radial, v * radial
    if model == RADIAL_FISHEYE:
        radial = e[0] * r2 + e[1] * (r2 * r2)
        return u * radial, v * radial
    if model == OPENCV:
        k1, k2, p1, p2 = e
        radial = k1 * r2 + k2 * r2 * r2
        return (u * radial + 2.0 * p1 * uv + p2 * (r2 + 2.0 * u2),
                v * radial + 2.0 * p2 * uv + p1 * (r2 + 2.0 * v2))
    if model == OPENCV_FISHEYE:
        t4 = r2 * r2
        t6, t8 = t4 * r2, t4 * t4
        radial = e[0] * r2 + e[1] * t4 + e[2] * t6 + e[3] * t8
        return u * radial, v * radial
    if model == FULL_OPENCV:
        k1, k2, p1, p2, k3, k4, k5, k6 = e
        r4 = r2 * r2
        r6 = r4 * r2
        radial = (1.0 + k1 * r2 + k2 * r4 + k3 * r6) / (1.0 + k4 * r2 + k5 * r4 + k6 * r6)
        return (u * radial + 2.0 * p1 * uv + p2 * (r2 + 2.0 * u2) - u,
                v * radial + 2.0 * p2 * uv + p1 * (r2 + 2.0 * v2) - v)
    if model == THIN_PRISM_FISHEYE:
        k1, k2, p1, p2, k3, k4, sx1, sy1 = e
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        radial = k1 * r2 + k2 * r4 + k3 * r6 + k4 * r8
        return (u * radial + 2.0 * p1 * uv + p2 * (r2 + 2.0 * u2) + sx1 * r2,
                v * radial + 2.0 * p2 * uv + p1 * (r2 + 2.0 * v2) + sy1 * r2)
    if model == RAD_TAN_THIN_PRISM_FISHEYE:
        th, pw = 1.0, 1.0
        for i in range(6):
            pw = pw * r2
            th = th + e[i] * pw
        p0, p1, s0, s1, s2, s3 = e[6:12]
        x, y = th * u, th * v
        x2, y2, xy = x * x, y * y, x * y
        q2 = x2 + y2
        q4 = q2 * q2
        return (x + (2.0 * p1 * xy + p0 * (q2 + 2.0 * x2)) + (s0 * q2 + s1 * q4) - u,
                y + (2.0 * p0 * xy + p1 * (q2 + 2.0 * y2)) + (s2 * q2 + s3 * q4) - v)
    return 0.0 * u, 0.0 * v


def _fisheye_from_normal(u, v):
    r = np.sqrt(u * u + v * v)
    big = r > EPS
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(big, np.arctan(r) / r, 1.0)
    return np.where(big, u * s, u), np.where(big, v * s, v)


def _normal_from_fisheye(uu, vv):
    theta = np.sqrt(uu * uu + vv * vv)
    tc = theta * np.cos(theta)
    big = tc > EPS
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(big, np.sin(theta) / tc, 1.0)
    return np.where(big, uu * s, uu), np.where(big, vv * s, vv)


def _fov_factor(omega, radius2, inverse):
    omega2 = omega * omega
    if omega2 < 1e-4:
        return (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0
    t = np.tan(omega / 2.0)
    radius = np.sqrt(radius2)
    with np.errstate(invalid="ignore", divide="ignore"):
        if inverse:
            small = (omega * (omega * omega * radius2 + 3.0)) / (6.0 * t)
            general = np.tan(radius * omega) / (radius * 2.0 * t)
        else:
            small = (-2.0 * t * (4.0 * radius2 * t * t - 3.0)) / (3.0 * omega)
            general = np.arctan(radius * 2.0 * t) / (radius * omega)
    return np.where(radius2 < 1e-4, small, general)


def img_from_normalized(cam, u, v):
    """ImgFromCam(u, v, 1) -> (x, y, valid) (sensor/models.h, check_cheirality = true)."""
    m, p = cam.model_id, cam.params
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    ok = np.ones(u.shape, bool)
    if m == EQUIRECTANGULAR:
        x = (np.arctan2(u, 1.0) / (2.0 * np.pi) + 0.5) * p[0]
        y = (0.5 - np.arctan2(-v, np.sqrt(u * u + 1.0)) / np.pi) * p[1]
        return x, y, ok
    f1, f2, c1, c2, e = split(m, p)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if m in (SIMPLE_PINHOLE, PINHOLE):
            return f1 * u + c1, f2 * v + c2, ok
        if m in (SIMPLE_DIVISION, DIVISION):
            rho = np.sqrt(u * u + v * v)
            disc_sq = 1.0 - 4.0 * rho * rho * e[0]
            ok = ~(disc_sq < 0.0)
            r = 2.0 / (1.0 + np.sqrt(np.where(ok, disc_sq, 0.0)))
            return f1 * r * u + c1, f2 * r * v + c2, ok
        if m == EUCM:
            alpha, beta = e
            rho2 = beta * (u * u + v * v) + 1.0
            ok = ~(rho2 < 0.0)
            den = alpha * np.sqrt(np.where(ok, rho2, 0.0)) + (1.0 - alpha)
            ok &= den >= EPS
            return f1 * (u / den) + c1, f2 * (v / den) + c2, ok
        if m == FOV:
            factor = _fov_factor(e[0], u * u + v * v, inverse=False)
            return f1 * (u * factor) + c1, f2 * (v * factor) + c2, ok
        if m in FISHEYES:
            u, v = _fisheye_from_normal(u, v)
        du, dv = distortion(m, e, u, v)
        return f1 * (u + du) + c1, f2 * (v + dv) + c2, ok


class NewtonTrace:
    """Per point of one iterative_undistortion call: the iterations taken, the steps the trust region shortened, the
    steps at which elimination with partial pivoting would swap its rows (|J10| > |J00|), and those of them at which
    elimination WITHOUT the swap would divide by (nearly) nothing (|J00| <= 1e-12 |J10|)."""

    def __init__(self, n):
        self.iterations, self.clamped, self.row_swaps, self.tiny_pivots = (np.zeros(n, np.int64) for _ in range(4))
        self.converged = np.zeros(n, bool)


def iterative_undistortion(model, e, u, v, trace=None):
    """IterativeUndistortion (sensor/models.h:1141-1197), all points at once; Jacobian by complex step. `trace`, a
    NewtonTrace of the same length, is filled in when given; the values do not depend on it."""
    x0, y0 = u.copy(), v.copy()
    x, y = u.copy(), v.copy()
    done = np.zeros(u.shape, bool)
    h = 1e-30
    with np.errstate(all="ignore"):
        for _ in range(100):
            act = ~done
            if not act.any():
                break
            xa, ya = x[act], y[act]
            du, dv = distortion(model, e, xa, ya)
            dux, dvx = distortion(model, e, xa + 1j * h, ya + 0j)
            duy, dvy = distortion(model, e, xa + 0j, ya + 1j * h)
            J = np.empty(xa.shape + (2, 2))
            J[..., 0, 0] = np.imag(dux) / h + 1.0
            J[..., 0, 1] = np.imag(duy) / h
            J[..., 1, 0] = np.imag(dvx) / h
            J[..., 1, 1] = np.imag(dvy) / h + 1.0
            rhs = np.stack([xa + du - x0[act], ya + dv - y0[act]], -1)
            det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
            sx = (J[..., 1, 1] * rhs[..., 0] - J[..., 0, 1] * rhs[..., 1]) / det
            sy = (J[..., 0, 0] * rhs[..., 1] - J[..., 1, 0] * rhs[..., 0]) / det
            radius_sqr = np.maximum((xa * xa + ya * ya) * 0.1 * 0.1, 0.1 * 0.1)
            n2 = sx * sx + sy * sy
            s = np.where(n2 > radius_sqr, np.sqrt(radius_sqr / n2), 1.0)
            if trace is not None:
                trace.iterations[act] += 1
                trace.clamped[act] += n2 > radius_sqr
                trace.row_swaps[act] += np.abs(J[..., 1, 0]) > np.abs(J[..., 0, 0])
                trace.tiny_pivots[act] += np.abs(J[..., 0, 0]) <= 1e-12 * np.abs(J[..., 1, 0])
            sx, sy = sx * s, sy * s
            x[act] = xa - sx
            y[act] = ya - sy
            fin = np.zeros(u.shape, bool)
            fin[act] = sx * sx + sy * sy < 1e-10
            done |= fin
    if trace is not None:
        trace.converged[:] = done
    return x, y, done


def cam_from_img(cam, xy):
    """CamFromImg for (N,2) pixels -> (N,2), NaN rows where the reference returns no value."""
    m, p = cam.model_id, cam.params
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    ok = np.ones(len(xy), bool)
    with np.errstate(all="ignore"):
        if m == EQUIRECTANGULAR:
            theta = 2.0 * np.pi * (x / p[0] - 0.5)
            phi = np.pi * (0.5 - y / p[1])
            rz = np.cos(phi) * np.cos(theta)
            ok = ~(rz <= EPS)
            u, v = np.cos(phi) * np.sin(theta) / rz, -np.sin(phi) / rz
        else:
            f1, f2, c1, c2, e = split(m, p)
            u, v = (x - c1) / f1, (y - c2) / f2
            if m in (SIMPLE_DIVISION, DIVISION):
                denom = 1.0 + e[0] * (u * u + v * v)
                u, v = u / denom, v / denom
            elif m == FOV:
                factor = _fov_factor(e[0], u * u + v * v, inverse=True)
                u, v = u * factor, v * factor
            elif m in (SIMPLE_FISHEYE, FISHEYE):
                u, v = _normal_from_fisheye(u, v)
            elif m == EUCM:
                alpha, beta = e
                r2 = u * u + v * v
                gamma = 1.0 - alpha
                radicand = 1.0 - (alpha - gamma) * beta * r2
                ok = ~(radicand < 0)
                helper_den = alpha * np.sqrt(np.where(ok, radicand, 0.0)) + gamma
                ok &= ~(helper_den < EPS)
                helper = (1.0 - alpha * alpha * beta * r2) / helper_den
                ok &= ~(helper < EPS)
                u, v = u / helper, v / helper
            elif m in ITERATIVE:
                u, v, ok = iterative_undistortion(m, e, u, v)
                if m in FISHEYES:
                    u, v = _normal_from_fisheye(u, v)
    out = np.stack([u, v], 1)
    out[~ok] = np.nan
    return out


def undistort_points(distorted, undistorted, xy):
    """The observation loop of UndistortReconstruction (image/undistortion.cc:334-381)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    if distorted.model_id == EQUIRECTANGULAR:
        return xy * np.array([undistorted.width / distorted.width, undistorted.height / distorted.height])
    uv = cam_from_img(distorted, xy)
    x, y, ok = img_from_normalized(undistorted, uv[:, 0], uv[:, 1])
    out = np.stack([x, y], 1)
    out[~ok | np.isnan(uv[:, 0])] = np.nan
    return out


def rescaled(cam, width, height):
    """Camera::Rescale(new_width, new_height) (scene/camera.cc:123-131)."""
    sx, sy = width / cam.width, height / cam.height
    p = cam.params.copy()
    if cam.model_id == EQUIRECTANGULAR:
        p[0] *= sx
        p[1] *= sy
    elif cam.model_id in ONE_FOCAL:
        p[0] *= 0.5 * (sx + sy)
        p[1] *= sx
        p[2] *= sy
    else:
        p[0] *= sx
        p[1] *= sy
        p[2] *= sx
        p[3] *= sy
    return Camera(cam.model_id, width, height, p, cam.camera_id)


def _cround(x):
    """std::round: half away from zero."""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def cast_u8(value):
    """BitmapColor<float>::Cast<uint8_t> (sensor/bitmap.h:216-223) of a double the reference narrows to float first."""
    r = _cround(np.asarray(value, np.float64).astype(np.float32))
    return np.clip(r, 0, 255).astype(np.uint8)


class WarpResult:
    """image: the expected pixels; near_half: the double interpolant of some channel lies within `half_tol` of a
    half-integer; near_edge: a source coordinate lies within `edge_tol` px of an integer."""

    def __init__(self, image, near_half, near_edge):
        self.image, self.near_half, self.near_edge = image, near_half, near_edge

    @property
    def may_differ(self):
        return self.near_half | self.near_edge


def warp(source_cam, target_cam, image, interpolation="bilinear", half_tol=1e-4, edge_tol=1e-9):
    """WarpImageBetweenCamerasImpl's pixel loop (image/warp.cc:113-139) for a PINHOLE target, whole image at once."""
    assert target_cam.model_id == PINHOLE
    img = np.asarray(image, np.uint8)
    grey = img.ndim == 2
    src = (img[..., None] if grey else img).astype(np.float64)
    H, W = source_cam.height, source_cam.width
    assert src.shape[:2] == (H, W)
    fx, fy, cx, cy = target_cam.params
    xs = (np.arange(target_cam.width, dtype=np.float64) + 0.5 - cx) / fx
    ys = (np.arange(target_cam.height, dtype=np.float64) + 0.5 - cy) / fy
    u, v = np.meshgrid(xs, ys)
    sx, sy, ok = img_from_normalized(source_cam, u, v)
    x, y = sx - 0.5, sy - 0.5
    C = src.shape[2]
    out = np.zeros(u.shape + (C,), np.uint8)
    near_half = np.zeros(u.shape, bool)
    with np.errstate(invalid="ignore"):
        if interpolation == "nearest":
            xr, yr = _cround(x), _cround(y)
            ok = ok & (xr >= 0) & (xr <= W - 1) & (yr >= 0) & (yr <= H - 1)
            xi, yi = np.where(ok, xr, 0).astype(np.int64), np.where(ok, yr, 0).astype(np.int64)
            out[ok] = src[yi[ok], xi[ok]].astype(np.uint8)
            # the rounding boundary of nearest-neighbour sampling is the half-integer coordinate
            fx_, fy_ = np.abs(x - np.floor(x) - 0.5), np.abs(y - np.floor(y) - 0.5)
            near_edge = (fx_ < edge_tol) | (fy_ < edge_tol)
        else:
            xf, yf = np.floor(x), np.floor(y)
            ok = ok & (xf >= 0) & (xf + 1 <= W - 1) & (yf >= 0) & (yf + 1 <= H - 1)
            x0, y0 = np.where(ok, xf, 0).astype(np.int64), np.where(ok, yf, 0).astype(np.int64)
            dx, dy = (x - xf)[..., None], (y - yf)[..., None]
            dx_1, dy_1 = 1.0 - dx, 1.0 - dy
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            v0 = dx_1 * src[y0, x0] + dx * src[y0, x1]
            v1 = dx_1 * src[y1, x0] + dx * src[y1, x1]
            val = dy_1 * v0 + dy * v1
            out[ok] = cast_u8(val)[ok]
            frac = np.abs(val - np.floor(val) - 0.5)
            near_half = ok & np.any(frac < half_tol, -1)
            near_edge = (np.abs(x - _cround(x)) < edge_tol) | (np.abs(y - _cround(y)) < edge_tol)
        near_edge &= np.isfinite(x) & np.isfinite(y)
    return WarpResult(out[..., 0] if grey else out, near_half, near_edge)


def _resize_weights(src_size, dst_size):
    """The triangle filter of colmap_amd/csrc/undistort.hip as a (dst, src) matrix of unnormalised weights."""
    s = src_size / dst_size
    r = max(s, 1.0)
    c = (np.arange(dst_size, dtype=np.float64) + 0.5) * s
    j = np.arange(src_size, dtype=np.float64)
    w = np.maximum(0.0, 1.0 - np.abs(j[None, :] + 0.5 - c[:, None]) / r)
    j0, j1 = np.floor(c - r), np.ceil(c + r)
    w[(j[None, :] < j0[:, None]) | (j[None, :] > j1[:, None])] = 0.0
    return w


def resize(image, width, height, half_tol=1e-4):
    """-> WarpResult of the resized image (near_edge all false)."""
    img = np.asarray(image, np.uint8)
    grey = img.ndim == 2
    src = (img[..., None] if grey else img).astype(np.float64)
    wy, wx = _resize_weights(src.shape[0], height), _resize_weights(src.shape[1], width)
    val = np.einsum("yj,jic->yic", wy, np.einsum("xi,jic->jxc", wx, src))
    val = val / (wx.sum(1)[None, :, None] * wy.sum(1)[:, None, None])
    out = cast_u8(val)
    near_half = np.any(np.abs(val - np.floor(val) - 0.5) < half_tol, -1)
    return WarpResult(out[..., 0] if grey else out, near_half, np.zeros(near_half.shape, bool))


def should_warp_directly(source_cam, target_cam, direct_warp_min_scale=0.5):
    """ShouldWarpDirectly (image/warp.cc:72-89)."""
    if (target_cam.width, target_cam.height) == (source_cam.width, source_cam.height):
        return True
    return min(target_cam.width / source_cam.width, target_cam.height / source_cam.height) >= direct_warp_min_scale


def distort_image(pinhole_cam, distorted_cam, image):
    """The inverse of undistortion, for building test inputs: the image a `distorted_cam` lens would have taken of what
    `pinhole_cam` saw (bilinear gather at CamFromImg of every distorted pixel)."""
    img = np.asarray(image, np.uint8)
    xs, ys = np.meshgrid(np.arange(distorted_cam.width) + 0.5, np.arange(distorted_cam.height) + 0.5)
    uv = cam_from_img(distorted_cam, np.stack([xs.ravel(), ys.ravel()], 1))
    fx, fy, cx, cy = pinhole_cam.params
    x = np.nan_to_num(fx * uv[:, 0] + cx - 0.5, nan=-10.0)
    y = np.nan_to_num(fy * uv[:, 1] + cy - 0.5, nan=-10.0)
    H, W = img.shape[:2]
    x, y = np.clip(x, 0, W - 1.001), np.clip(y, 0, H - 1.001)  # clamp to edge: no blank border in the test input
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    dx, dy = x - x0, y - y0
    f = img.astype(np.float64)
    if f.ndim == 3:
        dx, dy = dx[:, None], dy[:, None]
    val = (1 - dy) * ((1 - dx) * f[y0, x0] + dx * f[y0, x0 + 1]) + dy * ((1 - dx) * f[y0 + 1, x0] + dx * f[y0 + 1, x0 + 1])
    return cast_u8(val).reshape((distorted_cam.height, distorted_cam.width) + img.shape[2:])


def gradient_image(width=100, height=100):
    """The RGB test image of the reference's warp-options test (image/undistortion_test.cc:269-279)."""
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    return np.stack([x, y, (x + y) // 2], -1).astype(np.uint8)


def noise_image(width, height, channels=1, seed=0, n_comp=24):
    """Seeded band-limited noise: the procedural texture of colmap_amd/synthetic.py (sums of sinusoids with wavelengths
    of 5..40 px) evaluated on the image plane."""
    import math
    from colmap_amd import synthetic
    out = []
    for c in range(channels):
        wave, phase, amp = synthetic._texture_params(seed + 101 * c, n_comp, 2 * math.pi / 40, 2 * math.pi / 5, "cpu")
        wave, phase, amp = wave.numpy(), phase.numpy(), amp.numpy()
        x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
        arg = x[..., None] * wave[:, 0] + y[..., None] * wave[:, 1] + phase
        tex = (np.sin(arg) * amp).sum(-1) / np.linalg.norm(amp)
        out.append(np.clip(np.floor(128.0 + 70.0 * tex + 0.5), 0, 255).astype(np.uint8))
    return out[0] if channels == 1 else np.stack(out, -1)
