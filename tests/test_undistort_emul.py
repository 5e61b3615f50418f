"""colmap_amd/csrc/undistort.hip -- warp, points and resize kernels plus their host code -- run on the CPU through the
stand-in build of the unmodified source (tests/hip_emul/build_undistort.sh), against tests/undistort_reference.py. The
GPU tests run the same case functions through the hipcc build (tests/test_undistort_gpu.py)."""
import ctypes as C
import os
import subprocess

import pytest

import test_undistort_gpu as G
from colmap_amd import undistortion as U

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_lib = None


def _emul_lib():
    global _lib
    if _lib is None:
        so, src = os.path.join(EMUL, "libundistort_emul.so"), os.path.join(EMUL, "..", "..", "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("undistort.hip", "undistort_plan.h", "camera_projection.h")] + [os.path.join(EMUL, "hip", "hip_runtime.h"),
                                                                                                 os.path.join(EMUL, "..", "..", "include", "colmap_amd", "camera_models.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_undistort.sh")])
        _lib = C.CDLL(so)
        _lib.undistort_last_error.restype = C.c_char_p
    return _lib


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library U.lib() returns -- what the GPU cases call -- is the CPU build."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(U, "lib", _emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert U.lib() is _emul_lib()
    assert hasattr(U.lib(), "undistort_images")


@pytest.mark.parametrize("case", G.WARP_CASES, ids=G.WARP_IDS)
def test_warp_parity(case):
    G.case_warp(*case)


@pytest.mark.parametrize("model", G.PERSPECTIVE_MODELS, ids=[U.W.CAMERA_MODELS[m][0] for m in G.PERSPECTIVE_MODELS])
def test_points_match_checker(model):
    G.case_points(model)


def test_points_spherical():
    G.case_points_spherical()


def test_resize_kernel_matches_restated_filter():
    G.case_resize()


def test_indirect_path_property():
    G.case_indirect_property()


def test_indirect_path_small_target():
    G.case_indirect_small_target()


def test_blank_pixels_known_answers():
    G.case_blank_pixels()


def test_spherical_image():
    G.case_spherical_image()


def test_batch_and_errors():
    G.case_batch_and_errors()


def test_mixed_route_batch():
    G.case_mixed_route_batch()
