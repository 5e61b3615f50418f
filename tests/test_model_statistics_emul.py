"""colmap_amd/csrc/model_stats.hip -- every pass and its host code -- run on the CPU through the stand-in build of the
unmodified source (tests/hip_emul/build_model.sh), against colmap_amd.workspace.Model. The GPU tests run the same case
functions through the hipcc build (tests/test_model_statistics_gpu.py, where the comparison rule is stated)."""
import ctypes as C
import os
import subprocess

import pytest

import test_model_statistics_gpu as G
from colmap_amd import model_statistics as MS

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_lib = None


def _emul_lib():
    global _lib
    if _lib is None:
        so, src = os.path.join(EMUL, "libmodel_emul.so"), os.path.join(EMUL, "..", "..", "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("model_stats.hip", "model_plan.h")]
        deps += [os.path.join(EMUL, "hip", "hip_runtime.h"), os.path.join(EMUL, "..", "..", "include", "colmap_amd_model.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_model.sh")])
        _lib = C.CDLL(so)
    return _lib


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library MS.lib() returns -- what the GPU cases call -- is the CPU build."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(MS, "lib", _emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert MS.lib() is _emul_lib()
    assert hasattr(MS.lib(), "model_compute_pair_statistics")


def test_generated_model_has_the_shapes():
    G.case_model_shape()


def test_depth_ranges_match_checker():
    G.case_depth_ranges()


@pytest.mark.parametrize("percentile", G.PERCENTILES)
def test_pair_statistics_match_checker(percentile):
    G.case_pair_statistics(percentile)


@pytest.mark.parametrize("num_images,min_deg", G.OVERLAP_CASES)
def test_overlap_lists_match_checker(num_images, min_deg):
    G.case_overlap(num_images, min_deg)


def test_expectations_of_the_reference():
    G.case_reference_expectations()


def test_empty_models():
    G.case_empty_models()


def test_input_validation():
    G.case_input_validation()


def test_patch_match_config_auto_lines():
    G.case_patch_match_config()


def test_from_workspace_device_route(tmp_path):
    G.case_from_workspace(tmp_path)
