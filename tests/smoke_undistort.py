"""smoke(): one small image undistortion (64x48, SIMPLE_RADIAL) on cuda:0 through undistort_images, checked against the
numpy checker tests/undistort_reference.py (test infrastructure; imported only from __graft_entry__.smoke())."""
import numpy as np


def run():
    import undistort_reference as R
    from colmap_amd import undistortion as U
    cam = R.Camera(R.SIMPLE_RADIAL, 64, 48, [60.0, 32.3, 23.6, 0.2])
    img = R.noise_image(64, 48, 1, seed=7)
    got, out_cam = U.UndistortImage(U.UndistortCameraOptions(blank_pixels=0.5), img, cam)
    want = R.warp(cam, R.Camera(out_cam.model_id, out_cam.width, out_cam.height, out_cam.params), img)
    assert out_cam.model_id == R.PINHOLE and got.shape == want.image.shape
    assert np.array_equal(got, want.image), "undistorted image differs from the checker"   # no transcendental: exact
    xy = np.array([[10.5, 7.25], [50.0, 40.0], [32.3, 23.6]])
    moved = U.UndistortPoints(cam, out_cam, xy)
    assert np.abs(moved - R.undistort_points(cam, want_cam(out_cam, R), xy)).max() <= 1e-6
    print(f"smoke: image undistortion HIP == checker on 64x48 SIMPLE_RADIAL -> {out_cam.width}x{out_cam.height} PINHOLE")


def want_cam(c, R):
    return R.Camera(c.model_id, c.width, c.height, c.params)
