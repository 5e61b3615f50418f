"""CPU checker of stereo rectification (tests only): numpy in double precision on top of tests/undistort_reference.py,
written from the reference's sources (image/undistortion.cc:384-445, image/warp.cc:196-250) and not from
colmap_amd/csrc/undistort.hip.

What is independent of the library under test:
  * rectify_stereo_cameras takes axis and angle from the skew part and the trace of the rotation (the library goes
    through the quaternion, like Eigen), builds rotations with Rodrigues' formula on matrices, and inverts the
    calibration matrices with numpy.linalg;
  * warp_with_homography is a gather over whole arrays with undistort_reference's camera models and interpolant."""
from __future__ import annotations

import numpy as np

import undistort_reference as R


def euler_to_rotation(rx, ry, rz):
    """EulerAnglesToRotationMatrix (geometry/pose.cc): Rz(rz) Ry(ry) Rx(rx)."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _rodrigues(angle, axis):
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], np.float64)
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


def _angle_axis(Rm):
    """angle in [0, pi] and unit axis of a rotation matrix; (0, x axis) for the identity."""
    w = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    s = np.linalg.norm(w) / 2.0
    c = (np.trace(Rm) - 1.0) / 2.0
    if s == 0.0 and c > 0:
        return 0.0, np.array([1.0, 0.0, 0.0])
    return float(np.arctan2(s, c)), w / np.linalg.norm(w)   # not for angles near pi (the tests have none)


def calibration_matrix(cam):
    f1, f2, c1, c2, _ = R.split(cam.model_id, cam.params)
    return np.array([[f1, 0, c1], [0, f2, c2], [0, 0, 1]], np.float64)


def rectify_stereo_cameras(camera1, camera2, Rm, t):
    """RectifyStereoCameras (image/undistortion.cc:384-445) -> (H1, H2, Q)."""
    assert camera1.model_id in (R.SIMPLE_PINHOLE, R.PINHOLE) and camera2.model_id in (R.SIMPLE_PINHOLE, R.PINHOLE)
    Rm, t = np.asarray(Rm, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    angle, axis = _angle_axis(Rm)
    R2 = _rodrigues(-0.5 * angle, axis)
    R1 = R2.T
    t = R2 @ t
    x = np.array([1.0, 0.0, 0.0])
    if t @ x < 0:
        x = -x
    rot_axis = np.cross(t, x)
    if np.linalg.norm(rot_axis) < np.finfo(np.float64).eps:
        Rx = np.eye(3)
    else:
        a = np.arccos(abs(t @ x) / (np.linalg.norm(t) * np.linalg.norm(x)))
        Rx = _rodrigues(a, rot_axis / np.linalg.norm(rot_axis))
    R1, R2, t = Rx @ R1, Rx @ R2, Rx @ t
    K1, K2 = calibration_matrix(camera1), calibration_matrix(camera2)
    K = np.eye(3)
    K[0, 0] = K[1, 1] = min((K1[0, 0] + K1[1, 1]) / 2.0, (K2[0, 0] + K2[1, 1]) / 2.0)
    K[0, 2] = K1[0, 2]
    K[1, 2] = (K1[1, 2] + K2[1, 2]) / 2.0
    H1 = K @ R1 @ np.linalg.inv(K1)
    H2 = K @ R2 @ np.linalg.inv(K2)
    Q = np.eye(4)
    Q[3, 0], Q[3, 1], Q[3, 2], Q[2, 3], Q[3, 3] = -K[1, 2], -K[0, 2], K[0, 0], -1.0 / t[0], 0.0
    return H1, H2, Q


def warp_with_homography(Hinv, source_cam, target_cam, image, interpolation="bilinear", half_tol=1e-4, edge_tol=1e-9):
    """WarpImageWithHomographyBetweenCamerasImpl's pixel loop (image/warp.cc:214-245), direct path, for a PINHOLE
    target, whole image at once -> undistort_reference.WarpResult."""
    assert target_cam.model_id == R.PINHOLE
    Hinv = np.asarray(Hinv, np.float64).reshape(3, 3)
    img = np.asarray(image, np.uint8)
    grey = img.ndim == 2
    src = (img[..., None] if grey else img).astype(np.float64)
    H, W = source_cam.height, source_cam.width
    assert src.shape[:2] == (H, W)
    fx, fy, cx, cy = target_cam.params
    px, py = np.meshgrid(np.arange(target_cam.width, dtype=np.float64) + 0.5,
                         np.arange(target_cam.height, dtype=np.float64) + 0.5)
    wx = Hinv[0, 0] * px + Hinv[0, 1] * py + Hinv[0, 2]
    wy = Hinv[1, 0] * px + Hinv[1, 1] * py + Hinv[1, 2]
    wz = Hinv[2, 0] * px + Hinv[2, 1] * py + Hinv[2, 2]
    nonzero = wz != 0
    with np.errstate(all="ignore"):
        wzs = np.where(nonzero, wz, 1.0)
        u, v = (wx / wzs - cx) / fx, (wy / wzs - cy) / fy
        sx, sy, ok = R.img_from_normalized(source_cam, u, v)
    ok = ok & nonzero
    x, y = sx - 0.5, sy - 0.5
    C = src.shape[2]
    out = np.zeros(u.shape + (C,), np.uint8)
    near_half = np.zeros(u.shape, bool)
    with np.errstate(invalid="ignore"):
        if interpolation == "nearest":
            xr, yr = R._cround(x), R._cround(y)
            ok = ok & (xr >= 0) & (xr <= W - 1) & (yr >= 0) & (yr <= H - 1)
            xi, yi = np.where(ok, xr, 0).astype(np.int64), np.where(ok, yr, 0).astype(np.int64)
            out[ok] = src[yi[ok], xi[ok]].astype(np.uint8)
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
            out[ok] = R.cast_u8(val)[ok]
            frac = np.abs(val - np.floor(val) - 0.5)
            near_half = ok & np.any(frac < half_tol, -1)
            near_edge = (np.abs(x - R._cround(x)) < edge_tol) | (np.abs(y - R._cround(y)) < edge_tol)
        near_edge &= np.isfinite(x) & np.isfinite(y) & nonzero
    return R.WarpResult(out[..., 0] if grey else out, near_half, near_edge)


def rectify_pair(undistorted_cam, cam1, cam2, image1, image2, Rm, t, interpolation="bilinear"):
    """RectifyAndUndistortStereoImages (image/undistortion.cc:447-490) given the undistorted camera, direct path:
    -> (WarpResult 1, WarpResult 2, Q)."""
    H1, H2, Q = rectify_stereo_cameras(undistorted_cam, undistorted_cam, Rm, t)
    return (warp_with_homography(np.linalg.inv(H1), cam1, undistorted_cam, image1, interpolation),
            warp_with_homography(np.linalg.inv(H2), cam2, undistorted_cam, image2, interpolation), Q)


def rectify_indirect(undistorted_cam, cam, image, H, interpolation="bilinear"):
    """The library's indirect path (include/colmap_amd_undistort.h): the target camera rescaled to the source's size, the
    homography conjugated with that pixel scaling, the warp at source size -> (WarpResult of the intermediate image,
    WarpResult of the resize of its pixels)."""
    mid_cam = R.rescaled(undistorted_cam, cam.width, cam.height)
    S = np.diag([mid_cam.width / undistorted_cam.width, mid_cam.height / undistorted_cam.height, 1.0])
    mid = warp_with_homography(S @ np.linalg.inv(H) @ np.linalg.inv(S), cam, mid_cam, image, interpolation)
    return mid, R.resize(mid.image, undistorted_cam.width, undistorted_cam.height)
