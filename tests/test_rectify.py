"""Stereo rectification without a GPU: undistort_rectify_cameras on the host side of the hipcc-built library against the
known answer of the reference's own test (image/undistortion_test.cc:482-513), against the numpy restatement of
tests/rectify_reference.py, and against properties that need neither; and how rare the exception of the GPU parity rule
is on the cases of tests/test_rectify_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import rectify_reference as RR
import test_rectify_gpu as TG
import test_undistort_gpu as G
import undistort_reference as R
from colmap_amd import undistortion as U
from colmap_amd import workspace as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from colmap_amd import build
    build.build()


def _pinhole(f, w, h, cx=None, cy=None, fy=None):
    return W.SparseCamera(1, R.PINHOLE, w, h, np.array([f, f if fy is None else fy, w / 2.0 if cx is None else cx,
                                                        h / 2.0 if cy is None else cy], np.float64))


def test_abi_exports_every_declared_undistort_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colmap_amd_undistort.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(undistort_[a-z0-9_]+)\s*\(", text)))
    assert {"undistort_rectify_cameras", "undistort_rectify_images", "undistort_warp_homography"} <= set(names)
    from colmap_amd import build
    lib = ctypes.CDLL(build.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_stereo_pair_struct_matches_the_header():
    """undistort_stereo_pair as ctypes lays it out is two undistort_image, 9 + 3 + 16 doubles."""
    assert ctypes.sizeof(U._StereoPair) == 2 * ctypes.sizeof(U._Image) + 28 * 8
    assert U._StereoPair.R.offset == 2 * ctypes.sizeof(U._Image)


def test_rectify_cameras_known_answer():
    """image/undistortion_test.cc:482-513; the matrices are printed transposed there."""
    cam = _pinhole(1.0, 1, 1)
    H1, H2, Q = U.RectifyStereoCameras(cam, cam, RR.euler_to_rotation(0.1, 0.2, 0.3), [0.1, 0.2, 0.3])
    H1_ref = np.array([[-0.202759, -0.815848, -0.897034], [0.416329, 0.733069, -0.199657], [0.910839, -0.175408, 0.942638]])
    H2_ref = np.array([[-0.082173, -1.01288, -0.698868], [0.301854, 0.472844, -0.465336], [0.963533, 0.292411, 1.12528]])
    Q_ref = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -2.67261], [-0.5, -0.5, 1, 0]], np.float64)
    assert np.abs(H1 - H1_ref.T).max() <= 1e-5
    assert np.abs(H2 - H2_ref.T).max() <= 1e-5
    assert np.abs(Q - Q_ref).max() <= 1e-5


def _random_pose(rng):
    """A pose whose rotated baseline makes at least 0.05 rad with the x axis (there |d acos| <= 20 |d arg|)."""
    while True:
        Rm = RR.euler_to_rotation(*rng.uniform(-0.4, 0.4, 3))
        t = rng.uniform(-1.0, 1.0, 3)
        angle, axis = RR._angle_axis(Rm)
        th = RR._rodrigues(-0.5 * angle, axis) @ t
        if np.arccos(abs(th[0]) / np.linalg.norm(th)) >= 0.05:
            return Rm, t


def test_rectify_cameras_matches_numpy_restatement():
    """20 seeded random poses, cameras 640x480 with f in [400, 900]: entries agree within 1e-10 max|H|. A few ulps of
    double stay below 1e-14 where the baseline is at least 0.05 rad off the x axis; 1e-10 leaves four orders of margin."""
    rng = np.random.default_rng(2024)
    worst = 0.0
    for k in range(20):
        Rm, t = _random_pose(rng)
        f1, f2 = rng.uniform(400, 900, 2)
        cam1 = _pinhole(f1, 640, 480, 320 + rng.uniform(-20, 20), 240 + rng.uniform(-20, 20), f1 * rng.uniform(0.98, 1.02))
        cam2 = W.SparseCamera(2, R.SIMPLE_PINHOLE, 640, 480, np.array([f2, 320 + rng.uniform(-20, 20), 240 + rng.uniform(-20, 20)]))
        got = U.RectifyStereoCameras(cam1, cam2, Rm, t)
        want = RR.rectify_stereo_cameras(cam1, cam2, Rm, t)
        for g, w, name in zip(got, want, ("H1", "H2", "Q")):
            err = np.abs(g - w).max() / np.abs(w).max()
            worst = max(worst, err)
            assert err <= 1e-10, (k, name, err)
    print(f"rectify_cameras vs numpy: worst relative entry error {worst:.3e}")


def test_rectified_rows_agree():
    """The defining property, independent of the checker: a point seen by both cameras lands on the same row."""
    rng = np.random.default_rng(7)
    Rm, t = RR.euler_to_rotation(0.05, -0.1, 0.08), np.array([0.4, 0.07, -0.05])
    cam1, cam2 = _pinhole(520.0, 640, 480, 318.0, 243.0), _pinhole(610.0, 640, 480, 325.0, 236.0, 605.0)
    H1, H2, Q = U.RectifyStereoCameras(cam1, cam2, Rm, t)
    X1 = np.stack([rng.uniform(-1, 1, 100), rng.uniform(-1, 1, 100), rng.uniform(3, 10, 100)], 1)
    X2 = X1 @ Rm.T + t
    assert (X2[:, 2] > 0).all()
    p1 = (H1 @ RR.calibration_matrix(cam1) @ X1.T).T
    p2 = (H2 @ RR.calibration_matrix(cam2) @ X2.T).T
    rows1, rows2 = p1[:, 1] / p1[:, 2], p2[:, 1] / p2[:, 2]
    print(f"rectified rows: max |dy| {np.abs(rows1 - rows2).max():.3e} px")
    assert np.abs(rows1 - rows2).max() <= 1e-8
    # and disparity is along x only: the columns differ
    assert np.abs(p1[:, 0] / p1[:, 2] - p2[:, 0] / p2[:, 2]).min() > 1.0


def _K(cam1, cam2):
    K1, K2 = RR.calibration_matrix(cam1), RR.calibration_matrix(cam2)
    K = np.eye(3)
    K[0, 0] = K[1, 1] = min((K1[0, 0] + K1[1, 1]) / 2, (K2[0, 0] + K2[1, 1]) / 2)
    K[0, 2], K[1, 2] = K1[0, 2], (K1[1, 2] + K2[1, 2]) / 2
    return K, K1, K2


def test_baseline_along_x_needs_no_rotation():
    cam1, cam2 = _pinhole(500.0, 640, 480, 310.0, 250.0), _pinhole(640.0, 640, 480, 330.0, 230.0)
    K, K1, K2 = _K(cam1, cam2)
    for tx in (0.25, -0.25):   # -x takes the flipped unit vector (image/undistortion.cc:405-408): still no rotation
        H1, H2, Q = U.RectifyStereoCameras(cam1, cam2, np.eye(3), [tx, 0.0, 0.0])
        np.testing.assert_allclose(H1, K @ np.linalg.inv(K1), rtol=0, atol=1e-12 * np.abs(H1).max())
        np.testing.assert_allclose(H2, K @ np.linalg.inv(K2), rtol=0, atol=1e-12 * np.abs(H2).max())
        assert Q[2, 3] == -1.0 / tx
        assert (Q[3, 0], Q[3, 1], Q[3, 2], Q[3, 3]) == (-K[1, 2], -K[0, 2], K[0, 0], 0.0)


def test_baseline_along_minus_x_takes_the_flipped_unit_vector():
    """t = (-1, 0.1, 0): with the flipped unit vector the correction is the small rotation by atan(0.1) onto -x; without
    the flip it would be the rotation by pi - atan(0.1) onto +x."""
    cam = _pinhole(500.0, 640, 480)
    H1, H2, Q = U.RectifyStereoCameras(cam, cam, np.eye(3), [-1.0, 0.1, 0.0])
    K = RR.calibration_matrix(cam)
    Rx = np.linalg.inv(K) @ H1 @ K
    np.testing.assert_allclose(Rx @ Rx.T, np.eye(3), atol=1e-12)
    angle = np.arccos((np.trace(Rx) - 1.0) / 2.0)
    assert abs(angle - np.arctan(0.1)) <= 1e-12
    np.testing.assert_allclose(Rx @ np.array([-1.0, 0.1, 0.0]), [-np.hypot(1.0, 0.1), 0.0, 0.0], atol=1e-12)
    assert abs(Q[2, 3] - 1.0 / np.hypot(1.0, 0.1)) <= 1e-12    # -1 / t.x with t.x < 0
    np.testing.assert_allclose(H1, H2, atol=0, rtol=0)


def test_non_pinhole_camera_is_an_error():
    pin = _pinhole(500.0, 640, 480)
    radial = W.SparseCamera(2, R.SIMPLE_RADIAL, 640, 480, np.array([500.0, 320.0, 240.0, 0.1]))
    for c1, c2, which in ((radial, pin, "camera1"), (pin, radial, "camera2")):
        with pytest.raises(U.UndistortError, match=which + r"\.model_id == SimplePinholeCameraModel::model_id"):
            U.RectifyStereoCameras(c1, c2, np.eye(3), [1.0, 0.0, 0.0])


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam1, cam2, img1, img2 = TG.parity_inputs((64, 48), 1, R.SIMPLE_RADIAL)
    Rm, t = TG.pose("a")
    with pytest.raises(U.UndistortError, match="no HIP device available"):
        U.RectifyAndUndistortStereoImages(U.UndistortCameraOptions(), img1, img2, cam1, cam2, Rm, t)
    with pytest.raises(U.UndistortError, match="no HIP device available"):
        U.WarpImageWithHomographyBetweenCameras(U.WarpImageOptions(), np.eye(3), cam1,
                                                U.UndistortCamera(U.UndistortCameraOptions(), cam1), img1)


def test_checker_eligibility_share_is_small_for_the_rectify_cases():
    """The exception of the parity rule is rare by construction: counted from the checker alone on every GPU case."""
    for (size, channels, interp, model, pose_name) in TG.PARITY_CASES:
        cam1, cam2, img1, img2 = TG.parity_inputs(size, channels, model)
        Rm, t = TG.pose(pose_name)
        und = G._ref_cam(U.UndistortCamera(G._options(interp), cam1))
        for res in RR.rectify_pair(und, cam1, cam2, img1, img2, Rm, t, interp)[:2]:
            assert res.may_differ.mean() <= 0.01, (size, channels, interp, model, pose_name, res.may_differ.mean())
    cam = TG.source_camera(R.OPENCV, 64, 48)
    target = R.Camera(R.PINHOLE, 61, 47, [80.0, 81.0, 30.2, 23.4])
    for interp, channels in (("bilinear", 3), ("nearest", 1)):
        res = RR.warp_with_homography(TG.ZERO_W_HINV, cam, target, R.noise_image(64, 48, channels, 9), interp)
        assert res.may_differ.mean() <= 0.01
    # the indirect case: the intermediate image at source size
    cam1, cam2, img1, img2 = TG.parity_inputs((61, 47), 3, R.OPENCV)
    und = G._ref_cam(U.UndistortCamera(G._options(max_image_size=20), cam1))
    H1, H2, _ = RR.rectify_stereo_cameras(und, und, *TG.pose("a"))
    for cam, img, H in ((cam1, img1, H1), (cam2, img2, H2)):
        mid, small = RR.rectify_indirect(und, cam, img, H)
        assert mid.may_differ.mean() <= 0.01 and small.may_differ.mean() <= 0.01
