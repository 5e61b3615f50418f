"""Camera-model inputs at strong distortion and at the edges of each model's domain: what the Newton iteration's trust
region, pivot and iteration limit, the validity rules and the series branches of colmap_amd/csrc/camera_projection.h
exist for, and what the bundle-adjustment intrinsics on an in-image grid (tests/test_undistort_gpu.py) never reach.

A case is (kind, camera, points): kind "inverse" takes pixels through CamFromImg, kind "forward" takes normalized
coordinates through ImgFromCam(u, v, 1). Every case names the branches it exists for; census(case) counts, FROM THE
CHECKER ALONE (tests/undistort_reference.py), how many of its points take each branch, and tests/test_camera_edge_cases.py
asserts a non-zero count for every name. No validity predicate is evaluated near its threshold: place() moves a point
whose quantity lies within MARGIN (1e-9) of its own scale from the threshold (it does not drop it), assert_margins() restates
that for the tests.

    case(name) -> Case;  INVERSE, FORWARD: the case names;  WARP_CAMERAS, warp_camera(name): the warps into the invalid region
"""
import functools
from typing import NamedTuple

import numpy as np

import test_undistort_gpu as G
import undistort_reference as R
from colmap_amd import workspace as W

MARGIN = 1e-9
FOV_EPS = 1e-4


class Case(NamedTuple):
    name: str
    kind: str            # "inverse" | "forward"
    cam: R.Camera
    points: np.ndarray   # (N, 2) pixels (inverse) or normalized coordinates (forward)
    branches: tuple      # the census counters this case exists for


def _name(model):
    return W.CAMERA_MODELS[model][0]


def _camera(model, extra):
    """The bundle-adjustment camera of `model` with its extra parameters replaced."""
    cam = G.ba_camera(model)
    n = 3 if model in R.ONE_FOCAL else 4
    return R.Camera(model, cam.width, cam.height, list(cam.params[:n]) + list(extra))


def _pixels(cam, uv):
    f1, f2, c1, c2, _ = R.split(cam.model_id, cam.params)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    return np.stack([f1 * uv[:, 0] + c1, f2 * uv[:, 1] + c2], 1)


def _grid(x0, x1, nx, y0, y1, ny):
    xs, ys = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
    return np.stack([xs.ravel(), ys.ravel()], 1)


def _ring(radius, n=12, phase=0.3):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a)], 1)


# ---- the predicates, restated from the checker's formulas ------------------------------------------------------------

def _normalized(cam, xy):
    f1, f2, c1, c2, e = R.split(cam.model_id, cam.params)
    return (xy[:, 0] - c1) / f1, (xy[:, 1] - c2) / f2, e


def _newton(cam, xy):
    xn, yn, e = _normalized(cam, xy)
    tr = R.NewtonTrace(len(xy))
    x, y, ok = R.iterative_undistortion(cam.model_id, e, xn, yn, tr)
    return x, y, ok, tr


def predicates(kind, cam, pts):
    """name -> (quantity, threshold, gap): every quantity a validity rule or a branch compares with a threshold, NaN
    where the rule is not reached, and how far from the threshold it has to stay: MARGIN times the size of the terms the
    quantity is made of."""
    m = cam.model_id
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    nan = np.full(len(pts), np.nan)
    out = {}
    with np.errstate(all="ignore"):
        if kind == "inverse":
            xn, yn, e = _normalized(cam, pts)
            r2 = xn * xn + yn * yn
            if m in (R.SIMPLE_DIVISION, R.DIVISION):   # not a rule, a pole: 1 + k r^2 = 0 has no finite value
                out["denom"] = (1.0 + e[0] * r2, 0.0, np.maximum(1.0, np.abs(e[0]) * r2))
            elif m == R.FOV:
                out["omega2"] = (np.full(len(pts), e[0] * e[0]), FOV_EPS, np.full(len(pts), FOV_EPS))
                out["radius2"] = (r2 if e[0] * e[0] >= FOV_EPS else nan, FOV_EPS, np.maximum(r2, FOV_EPS))
            elif m in (R.SIMPLE_FISHEYE, R.FISHEYE):
                theta = np.sqrt(r2)
                out["theta_cos_theta"] = (theta * np.cos(theta), R.EPS, np.ones(len(pts)))
            elif m == R.EUCM:
                alpha, beta = e
                gamma = 1.0 - alpha
                radicand = 1.0 - (alpha - gamma) * beta * r2
                out["radicand"] = (radicand, 0.0, np.maximum(1.0, np.abs((alpha - gamma) * beta) * r2))
                helper_den = np.where(radicand < 0, np.nan, alpha * np.sqrt(np.abs(radicand)) + gamma)
                out["helper_den"] = (helper_den, R.EPS, np.ones(len(pts)))
                helper = np.where(helper_den < R.EPS, np.nan, (1.0 - alpha * alpha * beta * r2) / helper_den)
                out["helper"] = (helper, R.EPS, np.maximum(1.0, np.abs(alpha * alpha * beta) * r2) / np.abs(helper_den))
            elif m in R.ITERATIVE and m in R.FISHEYES:
                x, y, ok, _ = _newton(cam, pts)
                theta = np.sqrt(x * x + y * y)
                out["theta_cos_theta"] = (np.where(ok, theta * np.cos(theta), np.nan), R.EPS, np.ones(len(pts)))
        else:
            u, v = pts[:, 0], pts[:, 1]
            r2 = u * u + v * v
            e = R.split(m, cam.params)[4]
            if m in (R.SIMPLE_DIVISION, R.DIVISION):
                rho = np.sqrt(r2)
                out["disc_sq"] = (1.0 - 4.0 * rho * rho * e[0], 0.0, np.maximum(1.0, 4.0 * r2 * abs(e[0])))
            elif m == R.EUCM:
                alpha, beta = e
                rho2 = beta * r2 + 1.0
                out["rho2"] = (rho2, 0.0, np.maximum(1.0, abs(beta) * r2))
                den = np.where(rho2 < 0, np.nan, alpha * np.sqrt(np.abs(rho2)) + (1.0 - alpha))
                out["den"] = (den, R.EPS, np.ones(len(pts)))
            elif m == R.FOV:
                out["omega2"] = (np.full(len(pts), e[0] * e[0]), FOV_EPS, np.full(len(pts), FOV_EPS))
                out["radius2"] = (r2 if e[0] * e[0] >= FOV_EPS else nan, FOV_EPS, np.maximum(r2, FOV_EPS))
            elif m in R.FISHEYES:
                r = np.sqrt(r2)
                out["r"] = (r, R.EPS, np.maximum(r, R.EPS))
    out = {key: (q, thr, MARGIN * scale) for key, (q, thr, scale) in out.items()}
    if "den" in out:
        # u / den with den = alpha sqrt(rho2) - (alpha - 1) a difference of terms of size 1: a value just above the
        # threshold carries a relative error of eps / den, and 1e-12 (the noise-floor bar at f = 1000) needs den > 2e-4
        out["den"] = out["den"][:2] + (np.full(len(pts), 1e-2),)
    return out


def too_close(kind, cam, pts):
    """The points at which some predicate's quantity is closer to its threshold than the gap it has to keep."""
    bad = np.zeros(len(pts), bool)
    for q, thr, gap in predicates(kind, cam, pts).values():
        with np.errstate(invalid="ignore"):
            bad |= np.abs(q - thr) < gap
    return bad


def place(kind, cam, pts):
    """Moves (never drops) the points that sit on a threshold, by a fraction of the grid spacing."""
    pts = np.array(pts, np.float64).reshape(-1, 2)
    step = np.array([0.37, -0.23]) * (1.0 if kind == "inverse" else 1e-3)
    for _ in range(40):
        bad = too_close(kind, cam, pts)
        if not bad.any():
            return pts
        pts[bad] += step
    raise AssertionError("a point could not be moved off a threshold")


def assert_margins(c):
    n = len(c.points)
    for key, (q, thr, gap) in predicates(c.kind, c.cam, c.points).items():
        with np.errstate(invalid="ignore"):
            bad = np.abs(q - thr) < gap
        assert not bad.any(), f"{c.name}: {key} too close to {thr} at {np.nonzero(bad)[0][:5]} of {n}"


# ---- the census ------------------------------------------------------------------------------------------------------

def census(c):
    """branch name -> number of points of the case that take it, from the checker alone."""
    m, cam, pts = c.cam.model_id, c.cam, c.points
    p = predicates(c.kind, cam, pts)
    n = {}

    def count(name, mask):
        n[name] = int(np.count_nonzero(mask))

    with np.errstate(invalid="ignore"):
        if c.kind == "inverse" and m in R.ITERATIVE:
            _, _, ok, tr = _newton(cam, pts)
            count("newton_over_3_iterations", tr.iterations > 3)
            count("newton_100_iterations", tr.iterations == 100)
            count("newton_clamped_step", tr.clamped > 0)
            count("newton_row_swap", tr.row_swaps > 0)
            count("newton_pivot_near_zero", (tr.tiny_pivots > 0) & ok)
            count("newton_not_converged", ~ok)
            count("newton_converged", ok)
        if "theta_cos_theta" in p:
            tc = p["theta_cos_theta"][0]
            count("fisheye_inverse_pass_through", tc <= R.EPS)
            count("fisheye_inverse_scaled", tc > R.EPS)
        if "denom" in p:
            count("division_denominator_positive", p["denom"][0] > 0)
            count("division_denominator_negative", p["denom"][0] < 0)
        if "radicand" in p:
            count("eucm_radicand_negative", p["radicand"][0] < 0)
            count("eucm_helper_den_small", p["helper_den"][0] < R.EPS)
            count("eucm_helper_small", p["helper"][0] < R.EPS)
            count("eucm_inverse_value", p["helper"][0] >= R.EPS)
        if "disc_sq" in p:
            count("disc_sq_negative", p["disc_sq"][0] < 0)
            count("disc_sq_nonnegative", p["disc_sq"][0] >= 0)
        if "rho2" in p:
            count("eucm_rho2_negative", p["rho2"][0] < 0)
            count("eucm_den_small", p["den"][0] < R.EPS)
            count("eucm_forward_value", p["den"][0] >= R.EPS)
        if "omega2" in p:
            small_omega = p["omega2"][0] < FOV_EPS
            count("fov_omega_small", small_omega)
            count("fov_radius_small", p["radius2"][0] < FOV_EPS)
            count("fov_general", p["radius2"][0] >= FOV_EPS)
            count("fov_principal_point", np.hypot(*_fov_centre_offset(c)) == 0.0)
        if "r" in p:
            count("fisheye_r_small", p["r"][0] <= R.EPS)
            count("fisheye_r_large", p["r"][0] > R.EPS)
    return n


def _fov_centre_offset(c):
    if c.kind == "forward":
        return c.points[:, 0], c.points[:, 1]
    xn, yn, _ = _normalized(c.cam, c.points)
    return xn, yn


# ---- the cases -------------------------------------------------------------------------------------------------------

STRENGTHS = (8, 40)
ITERATIVE_GRID = _grid(-1500.5, 2524.5, 48, -1200.5, 1968.5, 36)   # 1728 pixels over 4x the 1024 x 768 image
assert len(ITERATIVE_GRID) == 1728

# what each iterative case reaches beside the trust region and the long iterations, which all of them reach; written
# down from the census of the checker (tests/test_camera_edge_cases.py asserts every entry)
_SWAP = ("newton_row_swap",)                                       # none for the two SIMPLE_RADIAL models: J10 = J01 there
_LIMIT = ("newton_not_converged", "newton_100_iterations")
_PASS = ("fisheye_inverse_pass_through",)                         # the solution has theta >= pi / 2
_ITERATIVE_EXTRA = {
    (R.SIMPLE_RADIAL, 8): (), (R.SIMPLE_RADIAL, 40): (),
    (R.RADIAL, 8): _SWAP, (R.RADIAL, 40): _SWAP,
    (R.OPENCV, 8): _SWAP, (R.OPENCV, 40): _SWAP,
    (R.OPENCV_FISHEYE, 8): _SWAP + _PASS, (R.OPENCV_FISHEYE, 40): _SWAP + _PASS,
    (R.FULL_OPENCV, 8): _SWAP + _LIMIT, (R.FULL_OPENCV, 40): _SWAP + _LIMIT,
    (R.SIMPLE_RADIAL_FISHEYE, 8): _PASS, (R.SIMPLE_RADIAL_FISHEYE, 40): (),
    (R.RADIAL_FISHEYE, 8): _SWAP + _PASS, (R.RADIAL_FISHEYE, 40): _SWAP + _PASS,
    (R.THIN_PRISM_FISHEYE, 8): _SWAP, (R.THIN_PRISM_FISHEYE, 40): _SWAP + _LIMIT,
    (R.RAD_TAN_THIN_PRISM_FISHEYE, 8): _SWAP + _LIMIT + _PASS, (R.RAD_TAN_THIN_PRISM_FISHEYE, 40): _SWAP + _LIMIT + _PASS,
}
_NEWTON_COMMON = ("newton_over_3_iterations", "newton_clamped_step", "newton_converged")

FORWARD_GRID = np.concatenate([_grid(-3.01, 2.97, 40, -2.53, 2.49, 30),
                               [[0.0, 0.0], [1e-9, -2e-9], [3e-3, 4e-3], [7e-3, -7e-3], [1e-17, 0.0]]], 0)
assert len(FORWARD_GRID) == 1205

FOV_OMEGAS = (0.6, 1.4, 0.005)
_FOV_BRANCHES = {0.6: ("fov_radius_small", "fov_general", "fov_principal_point"),
                 1.4: ("fov_radius_small", "fov_general", "fov_principal_point"),
                 0.005: ("fov_omega_small", "fov_principal_point")}


def _inverse_cases():
    cases = {}
    for m in R.ITERATIVE:
        for s in STRENGTHS:
            cam = G.strong(G.ba_camera(m), float(s))
            cases[f"inverse-{_name(m)}-x{s}"] = (cam, ITERATIVE_GRID, _NEWTON_COMMON + _ITERATIVE_EXTRA[m, s])
    # J00 + 1 == 0 at the start of the iteration, exactly: with u = 0, v = 1 it is 1 + (k1 + k2) + 2 p1, all dyadic, and
    # f = 1024 makes the pixel (512, 1408) the normalized point (0, 1) exactly. Elimination without the row swap divides
    # by that zero (inf - inf, no value); with it the iteration converges. The neighbours, 2^-36 px away, have
    # |J00 + 1| of 1e-13.
    for i, extra in enumerate(((-2.0, -2.0, 1.5, -1.0), (-2.0, -1.0, 1.0, -0.5), (-0.5, -2.0, 0.75, -0.5),
                               (0.125, -2.0, 0.4375, -0.125))):
        cam = R.Camera(R.OPENCV, 1024, 768, (1024.0, 1024.0, 512.0, 384.0) + extra)
        near = np.array([[512.0 + i * 2.0 ** -36, 1408.0 + j * 2.0 ** -36] for j in (-1, 0, 1) for i in (-1, 0, 1)])
        pts = np.concatenate([near[[4, 0, 1, 2, 3, 5, 6, 7, 8]], _grid(0.5, 1023.5, 5, 0.5, 767.5, 5)], 0)
        cases[f"inverse-OPENCV-zero-pivot-{i}"] = (cam, pts, ("newton_pivot_near_zero", "newton_row_swap", "newton_converged"))
    # theta = r / f on either side of pi / 2: rings at 0.2 .. 3.0 rad and an in-image grid
    for m in (R.SIMPLE_FISHEYE, R.FISHEYE):
        cam = G.ba_camera(m)
        uv = np.concatenate([_ring(t, 12, 0.1 * k) for k, t in enumerate((0.2, 0.9, 1.4, 1.55, 1.5707, 1.5709, 1.6, 2.2, 3.0))]
                            + [[[0.0, 0.0]]], 0)
        pts = np.concatenate([_pixels(cam, uv), _grid(0.5, 1023.5, 9, 0.5, 767.5, 7)], 0)
        cases[f"inverse-{_name(m)}"] = (cam, pts, ("fisheye_inverse_pass_through", "fisheye_inverse_scaled"))
    # EUCM: r^2 beyond 1 / (alpha^2 beta) has helper < eps, beyond 1 / ((2 alpha - 1) beta) a negative radicand; the
    # denominator alpha sqrt(radicand) + (1 - alpha) can fall below eps only for alpha > 1, hence the third camera, whose
    # ring at r^2 = 0.352 lies between helper_den = 0 (r^2 = 0.3472) and radicand = 0 (r^2 = 0.3571)
    eucm_grid = _grid(-3100.5, 4124.5, 41, -2900.5, 3668.5, 31)
    for (alpha, beta), names in (((0.56, 0.87), ("eucm_radicand_negative", "eucm_helper_small", "eucm_inverse_value")),
                                 ((0.9, -0.3), ("eucm_inverse_value",)),
                                 ((1.2, 2.0), ("eucm_radicand_negative", "eucm_helper_den_small", "eucm_inverse_value"))):
        cam = _camera(R.EUCM, (alpha, beta))
        pts = np.concatenate([eucm_grid, _pixels(cam, np.concatenate([_ring(np.sqrt(0.352)), _ring(0.3), _ring(0.58)], 0))], 0)
        cases[f"inverse-EUCM-{alpha}-{beta}"] = (cam, pts, names)
    # the division models: 1 + k r^2 changes sign at r^2 = -1 / k for k < 0
    for m, k in ((R.DIVISION, 0.2), (R.DIVISION, -0.4), (R.SIMPLE_DIVISION, 0.05), (R.SIMPLE_DIVISION, -0.4)):
        names = ("division_denominator_positive",) + (("division_denominator_negative",) if k < 0 else ())
        cases[f"inverse-{_name(m)}-k{k}"] = (_camera(m, (k,)), ITERATIVE_GRID, names)
    # FOV: radii on either side of radius^2 = 1e-4 (0.01: 9 px at f = 900), the principal point, and an in-image grid
    # (radius * omega stays below 1.1: tan() of the general branch has its pole at pi / 2)
    for omega in FOV_OMEGAS:
        cam = _camera(R.FOV, (omega,))
        uv = np.concatenate([_ring(t, 8, 0.2 * k) for k, t in enumerate((1e-6, 1e-3, 0.009, 0.0099, 0.0101, 0.011, 0.05, 0.3, 0.75))]
                            + [[[0.0, 0.0]]], 0)
        pts = np.concatenate([_pixels(cam, uv), _grid(0.5, 1023.5, 9, 0.5, 767.5, 7)], 0)
        cases[f"inverse-FOV-{omega}"] = (cam, pts, _FOV_BRANCHES[omega])
    return cases


def _forward_cases():
    cases = {}
    for m in G.PERSPECTIVE_MODELS:
        names = ()
        if m in R.FISHEYES:
            names = ("fisheye_r_small", "fisheye_r_large")
        elif m in (R.SIMPLE_DIVISION, R.DIVISION):
            names = ("disc_sq_nonnegative",)
        elif m == R.EUCM:
            names = ("eucm_forward_value",)
        elif m == R.FOV:
            names = _FOV_BRANCHES[0.6]
        cases[f"forward-{_name(m)}-x8"] = (G.strong(G.ba_camera(m), 8.0), FORWARD_GRID, names)
    for m, k in ((R.DIVISION, 0.2), (R.DIVISION, -0.4), (R.SIMPLE_DIVISION, 0.05)):
        names = ("disc_sq_nonnegative",) + (("disc_sq_negative",) if k > 0 else ())
        cases[f"forward-{_name(m)}-k{k}"] = (_camera(m, (k,)), FORWARD_GRID, names)
    # den = alpha sqrt(rho2) + (1 - alpha) falls below eps only for alpha > 1 and beta < 0 (r^2 in 3.24 .. 3.33 here)
    for (alpha, beta), names in (((0.9, -0.3), ("eucm_rho2_negative", "eucm_forward_value")),
                                 ((1.2, 2.0), ("eucm_forward_value",)),
                                 ((1.2, -0.3), ("eucm_rho2_negative", "eucm_den_small", "eucm_forward_value"))):
        cases[f"forward-EUCM-{alpha}-{beta}"] = (_camera(R.EUCM, (alpha, beta)), FORWARD_GRID, names)
    for omega in FOV_OMEGAS[1:]:
        cases[f"forward-FOV-{omega}"] = (_camera(R.FOV, (omega,)), FORWARD_GRID, _FOV_BRANCHES[omega])
    return cases


_INVERSE, _FORWARD = _inverse_cases(), _forward_cases()
INVERSE, FORWARD = list(_INVERSE), list(_FORWARD)
ALL = INVERSE + FORWARD


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once; the arrays are read-only."""
    kind = "inverse" if name in _INVERSE else "forward"
    cam, pts, names = (_INVERSE if kind == "inverse" else _FORWARD)[name]
    pts = place(kind, cam, pts)
    pts.setflags(write=False)
    return Case(name, kind, cam, pts, tuple(names))


# The branches of camera_projection.h that the suite's other inputs leave unreached; every one is named by some case.
REQUIRED = ("newton_clamped_step", "newton_row_swap", "newton_pivot_near_zero", "newton_not_converged", "newton_100_iterations",
            "fov_omega_small", "fov_radius_small", "fov_principal_point", "disc_sq_negative",
            "eucm_radicand_negative", "eucm_helper_den_small", "eucm_helper_small", "eucm_rho2_negative", "eucm_den_small",
            "fisheye_inverse_pass_through", "fisheye_r_small", "division_denominator_negative")

# ---- warps into the invalid region -----------------------------------------------------------------------------------

WARP_SOURCE = (64, 48)
WARP_TARGET = R.Camera(R.PINHOLE, 72, 52, [12.0, 12.0, 36.0, 26.0])   # corners at |u| = 3; 72 leaves a partial lane group
WARP_CAMERAS = {
    "DIVISION-k0.2": (R.DIVISION, (0.2,)),
    "SIMPLE_DIVISION-k0.05": (R.SIMPLE_DIVISION, (0.05,)),
    "EUCM-0.9--0.3": (R.EUCM, (0.9, -0.3)),
    "FOV-0.005": (R.FOV, (0.005,)),
    "FULL_OPENCV-x8": (R.FULL_OPENCV, None),
}


def warp_camera(name):
    """The source camera of a warp case: 64 x 48 with a focal length of 14 px, so that the image spans |u| < 2.3 and the
    target's corners at |u| = 3 look past it; the principal point is off the pixel grid (rule (b) of the parity rule)."""
    model, extra = WARP_CAMERAS[name]
    if extra is None:
        extra = G.strong(G.ba_camera(model), 8.0).params[4:]
    focal = (14.0,) if model in R.ONE_FOCAL else (14.0, 14.2)
    return R.Camera(model, *WARP_SOURCE, list(focal) + [32.37, 23.79] + list(extra))
