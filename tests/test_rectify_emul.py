"""The rectification kernel and its host code in colmap_amd/csrc/undistort.hip, run on the CPU through the stand-in build
of the unmodified source (tests/hip_emul/build_undistort.sh), against tests/rectify_reference.py. The GPU tests run the
same case functions through the hipcc build (tests/test_rectify_gpu.py)."""
import pytest

import test_rectify_gpu as G
import test_undistort_emul as E
from colmap_amd import undistortion as U


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library U.lib() returns -- what the GPU cases call -- is the CPU build."""
    import os
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(U, "lib", E._emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert U.lib() is E._emul_lib()
    assert hasattr(U.lib(), "undistort_rectify_images") and hasattr(U.lib(), "undistort_warp_homography")


@pytest.mark.parametrize("case", G.PARITY_CASES, ids=G.PARITY_IDS)
def test_rectify_parity(case):
    G.case_parity(*case)


@pytest.mark.parametrize("interp,channels", [("bilinear", 3), ("nearest", 1)])
def test_zero_third_coordinate_is_blank(interp, channels):
    G.case_zero_w(interp, channels)


def test_indirect_path():
    G.case_indirect()


def test_reference_property_solid_colours():
    G.case_reference_property()


def test_batch_is_bit_identical_to_single_calls():
    G.case_batch()


def test_errors():
    G.case_errors()


def test_stereo_image_rectifier_end_to_end(tmp_path):
    G.case_rectifier_end_to_end(tmp_path)


def test_standalone_image_undistorter_end_to_end(tmp_path):
    G.case_standalone_end_to_end(tmp_path)
