"""The C++ surface of stereo rectification (include/colmap_amd/undistortion.hpp) and colour extraction
(include/colmap_amd/colors.hpp) from g++: tests/cpp/test_image_commands_host.cc, compiled like tests/test_cpp_host.py
compiles its host programs. RectifyStereoCameras' known answer runs without a GPU; the rectified images and the colours
on the GPU are compared with the Python surface and with the values the solid inputs imply."""
import subprocess

import numpy as np
import pytest

import rectify_reference as RR
import test_cpp_host
import undistort_reference as R


@pytest.fixture(scope="session")
def image_commands_host(tmp_path_factory):
    return test_cpp_host._compile("test_image_commands_host", tmp_path_factory)


def test_cpp_rectify_known_answer(image_commands_host):
    r = subprocess.run([image_commands_host, "known"], capture_output=True, text=True)
    assert r.returncode == 0 and "known OK" in r.stdout, r.stderr


def test_cpp_without_a_gpu_fails_loudly(image_commands_host, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([image_commands_host, "device", str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device available" in r.stderr


@pytest.mark.gpu
def test_cpp_rectify_and_colors(image_commands_host, tmp_path):
    from colmap_amd import undistortion as U
    out = tmp_path / "out.txt"
    r = subprocess.run([image_commands_host, "device", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = out.read_text().splitlines()
    w, h = (int(v) for v in lines[0].split())
    got1 = np.array(lines[1].split(), np.uint8).reshape(h, w, 3)
    got2 = np.array(lines[2].split(), np.uint8).reshape(h, w, 3)
    cam = R.Camera(R.SIMPLE_RADIAL, 100, 100, [100.0, 50.0, 50.0, 0.1])
    red = np.zeros((100, 100, 3), np.uint8)
    red[..., 0] = 255
    green = np.zeros((100, 100, 3), np.uint8)
    green[..., 1] = 255
    o1, o2, _, _ = U.RectifyAndUndistortStereoImages(U.UndistortCameraOptions(), red, green, cam, cam,
                                                     RR.euler_to_rotation(0.0, 0.05, 0.0), [0.1, 0.0, 0.0])
    assert np.array_equal(got1, o1) and np.array_equal(got2, o2)   # the same library call from both surfaces
    colours = np.array(lines[3].split(), int).reshape(4, 4)
    assert colours.tolist() == [[21, 41, 221, 2]] * 3 + [[0, 0, 0, 0]]
