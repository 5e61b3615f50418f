"""The host-only plan of image undistortion (colmap_amd/csrc/undistort_plan.h): tests/cpp/test_undistort_plan.cc checks
UndistortCamera and RectifyStereoCameras against the known answers of the reference's tests, the route of an image
(clone, resize, direct, indirect) at the edges of direct_warp_min_scale, the mid camera and the conjugated homography of
the indirect route, padded pitches, buffer sizes and grids, and every refusal with its message and with the image or pair
it names. Compiled with g++ alone: the header needs neither the HIP runtime nor the library. The second build runs the
same stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan(tmp_path, sanitize):
    exe = str(tmp_path / "test_undistort_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_undistort_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "undistort plan checks OK" in r.stdout
