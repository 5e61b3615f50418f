"""colmap_amd/csrc/camera_projection.h as gfx950 runs it, at strong distortion and at the edges of the models' domains
(the cases of tests/camera_edge_cases.py), pointwise:

  UndistortPoints(cam, unit pinhole, xy)  is CamFromImg(cam, xy) unchanged       (1 * u + 0 is exact)
  UndistortPoints(unit pinhole, cam, uv)  is ImgFromCam(cam, (u, v, 1)) unchanged ((x - 0) / 1 is exact)

Inverse: the device against the host build of the same header (U.CamFromImg) -- the same rows without a value, equal
values for the models without a transcendental function (-ffp-contract=off: same expression, same rounding; equal as
numbers: the unit pinhole's "+ 0" turns -0.0 into 0.0), at most 16 eps of max(1, |value|) for the others (one sin, one
cos: 2 ulp on the device + 1 on the host, and three roundings, doubled) -- and against the numpy checker: the same rows
without a value, values within 1e-9 of max(1, |value|) (1e-6 px at f = 1000).
Forward: the same rows without a value as the checker; values within 4 B + 4 eps max(f, |value|) of the 50-digit
evaluation (tests/camera_projection_mp.py), B being the checker's own worst error against it over the case; equal to the
checker for the models without a transcendental function.
Warp: five cameras whose domain ends inside the target, under the parity rule of tests/test_undistort_gpu.py, with the
blank set equal to the checker's.

The case functions are shared with tests/test_camera_projection_emul.py (the CPU stand-in build of the same source)."""
import functools

import numpy as np
import pytest

import camera_edge_cases as E
import rectify_reference as RR
import test_undistort_gpu as G
import undistort_reference as R
from colmap_amd import undistortion as U

UNIT = R.Camera(R.PINHOLE, 1, 1, [1.0, 1.0, 0.0, 0.0])
EPS = R.EPS
DEVICE_HOST_EPS = 16.0
CHECKER_BAR = 1e-9
NOISE_FLOOR_BAR = 1e-9   # px per max(1, |value| / f): what a double evaluation of the forward models may lose


def _focal(cam):
    return float(max(R.split(cam.model_id, cam.params)[:2]))


@functools.lru_cache(maxsize=None)
def forward_truth(name):
    """(hi, lo, valid, B) of a forward case: the 50-digit values as hi + lo (two doubles), which points have a value, and
    B = max |checker - 50 digits| in px. Computed once per session and read-only."""
    mp = pytest.importorskip("mpmath")
    import camera_projection_mp as M
    c = E.case(name)
    x, y, ok = R.img_from_normalized(c.cam, c.points[:, 0], c.points[:, 1])
    want = np.stack([x, y], 1)
    hi, lo = np.full(want.shape, np.nan), np.zeros(want.shape)
    valid = np.zeros(len(want), bool)
    err = np.zeros(want.shape)
    with mp.workdps(M.DIGITS):
        for i, (u, v) in enumerate(c.points):
            val = M.img_from_normalized(c.cam.model_id, c.cam.params, u, v)
            if val is None:
                continue
            valid[i] = True
            for k in range(2):
                hi[i, k] = float(val[k])
                lo[i, k] = float(val[k] - mp.mpf(hi[i, k]))
                err[i, k] = abs(float(mp.mpf(float(want[i, k])) - val[k])) if ok[i] else np.inf
    assert np.array_equal(valid, ok), f"{name}: the 50-digit evaluation takes another validity branch than the checker"
    bar = NOISE_FLOOR_BAR * np.maximum(1.0, np.abs(hi) / _focal(c.cam))
    B = float(err[valid].max()) if valid.any() else 0.0
    print(f"{name}: B = max |checker - 50 digits| = {B:.3e} px, worst share of its bar {np.nanmax(err[valid] / bar[valid]):.3e}")
    assert (err[valid] <= bar[valid]).all(), f"{name}: the checker is {np.nanmax(err[valid] / bar[valid]):.3g} x its noise-floor bar"
    for a in (hi, lo, valid):
        a.setflags(write=False)
    return hi, lo, valid, B


def _same_rows_without_value(got, want, what):
    g, w = np.isnan(got), np.isnan(want)
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(w[:, 0], w[:, 1])
    assert np.array_equal(g, w), f"{what}: rows without a value differ at {np.nonzero(g[:, 0] != w[:, 0])[0][:8].tolist()}"
    return ~g[:, 0]


def case_inverse(name):
    c = E.case(name)
    E.assert_margins(c)
    m = c.cam.model_id
    got = U.UndistortPoints(c.cam, UNIT, c.points)
    host = U.CamFromImg(c.cam, c.points)
    want = R.cam_from_img(c.cam, c.points)
    has = _same_rows_without_value(got, host, f"{name} device / host")
    _same_rows_without_value(got, want, f"{name} device / checker")
    scale = np.maximum(1.0, np.abs(host[has]))
    d_host = float((np.abs(got[has] - host[has]) / scale).max() / EPS) if has.any() else 0.0
    d_want = float((np.abs(got[has] - want[has]) / np.maximum(1.0, np.abs(want[has]))).max()) if has.any() else 0.0
    print(f"{name}: {int(has.sum())} of {len(has)} points have a value; device - host {d_host:.2f} eps, "
          f"device - checker {d_want:.3e} (relative to max(1, |value|))")
    if m in R.NO_TRANSCENDENTAL:
        assert np.array_equal(got[has], host[has]), f"{name}: device and host differ by {d_host:.2f} eps"
    else:
        assert d_host <= DEVICE_HOST_EPS
    assert d_want <= CHECKER_BAR
    return d_host, d_want


def case_forward(name):
    c = E.case(name)
    E.assert_margins(c)
    m = c.cam.model_id
    hi, lo, valid, B = forward_truth(name)
    got = U.UndistortPoints(UNIT, c.cam, c.points)
    x, y, ok = R.img_from_normalized(c.cam, c.points[:, 0], c.points[:, 1])
    want = np.stack([x, y], 1)
    want[~ok] = np.nan
    has = _same_rows_without_value(got, want, f"{name} device / checker")
    assert np.array_equal(has, valid)
    err = np.abs((got[has] - hi[has]) - lo[has])
    bar = 4.0 * B + 4.0 * EPS * np.maximum(_focal(c.cam), np.abs(hi[has]))
    worst = float((err / bar).max()) if has.any() else 0.0
    print(f"{name}: {int(has.sum())} of {len(has)} points have a value; B {B:.3e} px, max |device - 50 digits| {err.max():.3e} px, "
          f"worst share of the bar {worst:.3f}")
    assert worst <= 1.0
    if m in R.NO_TRANSCENDENTAL:
        assert np.array_equal(got[has], want[has]), "a model without a transcendental function must equal the checker"
    return B, float(err.max())


WARP_CASES = [(n, ch, interp) for n in E.WARP_CAMERAS for ch in (1, 3) for interp in ("bilinear", "nearest")]
WARP_IDS = [f"{n}-{ch}ch-{interp}" for n, ch, interp in WARP_CASES]


def warp_inputs(name, channels):
    return E.warp_camera(name), R.noise_image(*E.WARP_SOURCE, channels, 7)


def _blank(image):
    return image == 0 if image.ndim == 2 else ~image.any(-1)


def case_warp(name, channels, interp):
    cam, img = warp_inputs(name, channels)
    got = U.WarpImageWithHomographyBetweenCameras(U.WarpImageOptions(interpolation=interp), np.eye(3), cam, E.WARP_TARGET, img)
    want = RR.warp_with_homography(np.eye(3), cam, E.WARP_TARGET, img, interp)
    blank = _blank(want.image)
    assert 0.1 <= blank.mean() <= 0.9, blank.mean()
    G.compare_under_parity_rule(got, want, None, f"warp into the invalid region {name} {channels}ch {interp}")
    assert np.array_equal(_blank(got), blank), "the blank set differs from the checker's"


# ---- the GPU runs ----------------------------------------------------------------------------------------------------

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", E.INVERSE)
def test_inverse_matches_host_build_and_checker(name):
    case_inverse(name)


@pytest.mark.parametrize("name", E.FORWARD)
def test_forward_matches_50_digits_and_checker(name):
    case_forward(name)


@pytest.mark.parametrize("case", WARP_CASES, ids=WARP_IDS)
def test_warp_into_the_invalid_region(case):
    case_warp(*case)
