"""ImgFromCam(u, v, 1) of all 18 camera models at 50 significant digits (mpmath), restated branch by branch from the
formulas as tests/undistort_reference.py states them: the noise floor a double evaluation is measured against.

The reference's FORMULAS are the specification, not the functions they approximate: FOV's two series branches are the
truncated series (the exact function differs from them by up to 0.7 px at omega = 0.005), the fisheye scale is applied
only for r > epsilon, and pi is the double M_PI. Inputs are doubles and enter exactly; the thresholds are compared on the
50-digit quantities, which the cases keep away from their thresholds (tests/camera_edge_cases.py), so the branch taken is
the one the checker takes -- the tests assert that.

    img_from_normalized(model, params, u, v) -> (x, y) as mpf, or None where the model has no value
"""
import mpmath as mp

import undistort_reference as R

DIGITS = 50
EPS = mp.mpf(2) ** -52
FOV_EPS = mp.mpf("1e-4")


def _f(x):
    return mp.mpf(float(x))


def _distortion(model, e, u, v):
    u2, uv, v2 = u * u, u * v, v * v
    r2 = u2 + v2
    if model in (R.SIMPLE_RADIAL, R.SIMPLE_RADIAL_FISHEYE):
        radial = e[0] * r2
        return u * radial, v * radial
    if model in (R.RADIAL, R.RADIAL_FISHEYE):
        radial = e[0] * r2 + e[1] * r2 ** 2
        return u * radial, v * radial
    if model == R.OPENCV:
        k1, k2, p1, p2 = e
        radial = k1 * r2 + k2 * r2 ** 2
        return (u * radial + 2 * p1 * uv + p2 * (r2 + 2 * u2), v * radial + 2 * p2 * uv + p1 * (r2 + 2 * v2))
    if model == R.OPENCV_FISHEYE:
        radial = e[0] * r2 + e[1] * r2 ** 2 + e[2] * r2 ** 3 + e[3] * r2 ** 4
        return u * radial, v * radial
    if model == R.FULL_OPENCV:
        k1, k2, p1, p2, k3, k4, k5, k6 = e
        radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        return (u * radial + 2 * p1 * uv + p2 * (r2 + 2 * u2) - u, v * radial + 2 * p2 * uv + p1 * (r2 + 2 * v2) - v)
    if model == R.THIN_PRISM_FISHEYE:
        k1, k2, p1, p2, k3, k4, sx1, sy1 = e
        radial = k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3 + k4 * r2 ** 4
        return (u * radial + 2 * p1 * uv + p2 * (r2 + 2 * u2) + sx1 * r2,
                v * radial + 2 * p2 * uv + p1 * (r2 + 2 * v2) + sy1 * r2)
    if model == R.RAD_TAN_THIN_PRISM_FISHEYE:
        th = 1 + sum(e[i] * r2 ** (i + 1) for i in range(6))
        p0, p1, s0, s1, s2, s3 = e[6:12]
        x, y = th * u, th * v
        q2 = x * x + y * y
        return (x + 2 * p1 * x * y + p0 * (q2 + 2 * x * x) + s0 * q2 + s1 * q2 ** 2 - u,
                y + 2 * p0 * x * y + p1 * (q2 + 2 * y * y) + s2 * q2 + s3 * q2 ** 2 - v)
    return mp.mpf(0), mp.mpf(0)


def _fov_distortion_factor(omega, radius2):
    omega2 = omega * omega
    if omega2 < FOV_EPS:
        return omega2 * radius2 / 3 - omega2 / 12 + 1
    t = mp.tan(omega / 2)
    if radius2 < FOV_EPS:
        return -2 * t * (4 * radius2 * t * t - 3) / (3 * omega)
    radius = mp.sqrt(radius2)
    return mp.atan(radius * 2 * t) / (radius * omega)


def img_from_normalized(model, params, u, v):
    with mp.workdps(DIGITS):
        p = [_f(x) for x in params]
        u, v = _f(u), _f(v)
        if model == R.EQUIRECTANGULAR:
            pi = _f(R.np.pi)
            return ((mp.atan2(u, 1) / (2 * pi) + mp.mpf("0.5")) * p[0],
                    (mp.mpf("0.5") - mp.atan2(-v, mp.sqrt(u * u + 1)) / pi) * p[1])
        f1, f2, c1, c2, e = R.split(model, p)
        if model in (R.SIMPLE_PINHOLE, R.PINHOLE):
            return f1 * u + c1, f2 * v + c2
        if model in (R.SIMPLE_DIVISION, R.DIVISION):
            disc_sq = 1 - 4 * (u * u + v * v) * e[0]
            if disc_sq < 0:
                return None
            r = 2 / (1 + mp.sqrt(disc_sq))
            return f1 * r * u + c1, f2 * r * v + c2
        if model == R.EUCM:
            alpha, beta = e
            rho2 = beta * (u * u + v * v) + 1
            if rho2 < 0:
                return None
            den = alpha * mp.sqrt(rho2) + (1 - alpha)
            if not den >= EPS:
                return None
            return f1 * (u / den) + c1, f2 * (v / den) + c2
        if model == R.FOV:
            factor = _fov_distortion_factor(e[0], u * u + v * v)
            return f1 * (u * factor) + c1, f2 * (v * factor) + c2
        if model in R.FISHEYES:
            r = mp.sqrt(u * u + v * v)
            if r > EPS:
                u, v = u * (mp.atan(r) / r), v * (mp.atan(r) / r)
        du, dv = _distortion(model, e, u, v)
        return f1 * (u + du) + c1, f2 * (v + dv) + c2
