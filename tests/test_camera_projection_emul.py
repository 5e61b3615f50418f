"""The cases of tests/test_camera_projection_gpu.py through the CPU stand-in build of colmap_amd/csrc/undistort.hip
(tests/hip_emul/build_undistort.sh): the points and warp kernels and the host function read the same
camera_projection.h, so device-against-host is trivially equal here; what this run checks without a GPU is the header
against the numpy checker and the 50-digit evaluation at every edge case, and the case functions themselves."""
import pytest

import camera_edge_cases as E
import test_camera_projection_gpu as P
import test_undistort_emul as UE
from colmap_amd import undistortion as U

emulated_library = UE.emulated_library


def test_emulated_library_is_the_one_under_test():
    assert U.lib() is UE._emul_lib()


@pytest.mark.parametrize("name", E.INVERSE)
def test_inverse_matches_host_build_and_checker(name):
    P.case_inverse(name)


@pytest.mark.parametrize("name", E.FORWARD)
def test_forward_matches_50_digits_and_checker(name):
    P.case_forward(name)


@pytest.mark.parametrize("case", P.WARP_CASES, ids=P.WARP_IDS)
def test_warp_into_the_invalid_region(case):
    P.case_warp(*case)
