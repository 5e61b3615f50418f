"""The C++ surface of image undistortion (include/colmap_amd/undistortion.hpp) from g++: tests/cpp/test_undistort_host.cc,
compiled like tests/test_cpp_host.py compiles its host programs. The known answers of the reference's UndistortCamera
tests run without a GPU (host-only undistort_camera); the image and the observations on the GPU are compared with
tests/undistort_reference.py."""
import subprocess

import numpy as np
import pytest

import test_cpp_host
import undistort_reference as R


@pytest.fixture(scope="session")
def undistort_host(tmp_path_factory):
    return test_cpp_host._compile("test_undistort_host", tmp_path_factory)


def test_cpp_known_answers(undistort_host):
    r = subprocess.run([undistort_host, "known"], capture_output=True, text=True)
    assert r.returncode == 0 and "known OK" in r.stdout, r.stderr


def test_cpp_image_without_a_gpu_fails_loudly(undistort_host, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([undistort_host, "image", str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device available" in r.stderr


@pytest.mark.gpu
def test_cpp_image_and_reconstruction_match_checker(undistort_host, tmp_path):
    out = tmp_path / "out.txt"
    r = subprocess.run([undistort_host, "image", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = out.read_text().splitlines()
    w, h, c = (int(v) for v in lines[0].split())
    got = np.array(lines[1].split(), np.uint8).reshape(h, w, c)
    cam = R.Camera(R.SIMPLE_RADIAL, 100, 100, [100.0, 50.0, 50.0, 0.5])
    und = R.Camera(R.PINHOLE, 84, 84, [100.0, 100.0, 42.0, 42.0])
    want = R.warp(cam, und, R.gradient_image(100, 100))
    assert np.array_equal(got, want.image)   # SIMPLE_RADIAL: no transcendental, exact
    xy = np.array(lines[2].split(), float).reshape(-1, 2)
    ref = R.undistort_points(cam, und, np.array([[10.0, 20.0], [50.0, 50.0], [90.5, 12.25]]))
    assert np.abs(xy - ref).max() <= 1e-6
