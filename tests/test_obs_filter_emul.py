"""colmap_amd/csrc/obs_filter.hip -- both passes and their host code -- run on the CPU through the stand-in build of the
unmodified source (tests/hip_emul/build_obs.sh), against tests/obs_reference.py. The GPU tests run the same case
functions through the hipcc build (tests/test_obs_filter_gpu.py)."""
import ctypes as C
import os
import subprocess

import pytest

import obs_reference as Q
import test_obs_filter as T
import test_obs_filter_gpu as G
from colmap_amd import observation_manager as OM

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_lib = None


def _emul_lib():
    global _lib
    if _lib is None:
        so, src = os.path.join(EMUL, "libobs_emul.so"), os.path.join(EMUL, "..", "..", "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("obs_filter.hip", "obs_plan.h", "camera_projection.h")]
        deps += [os.path.join(EMUL, "hip", "hip_runtime.h"), os.path.join(EMUL, "..", "..", "include", "colmap_amd_obs.h"),
                 os.path.join(EMUL, "..", "..", "include", "colmap_amd", "camera_models.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_obs.sh")])
        _lib = C.CDLL(so)
        _lib.obs_last_error.restype = C.c_char_p
    return _lib


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library OM.lib() returns -- what the GPU cases call -- is the CPU build."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(OM, "lib", _emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert OM.lib() is _emul_lib()
    assert hasattr(OM.lib(), "obs_filter_all_points3D")


def test_generated_model_has_the_shapes():
    G.case_model_shape()


def test_edges_model_has_the_observations_it_is_named_for():
    G.case_edges_shape()


@pytest.mark.parametrize("error_type", [Q.PIXEL, Q.NORMALIZED, Q.ANGULAR], ids=["pixel", "normalized", "angular"])
@pytest.mark.parametrize("name", ["mixed", "single", "seam", "edges"])
def test_filter_all_points3D_matches_checker(name, error_type):
    G.case_filter_all(name, error_type)


def test_errors_then_angles():
    G.case_order_errors_then_angles()


@pytest.mark.parametrize("name", ["mixed", "single", "edges"])
def test_negative_depth_matches_checker(name):
    G.case_negative_depth(name)


@pytest.mark.parametrize("name", ["mixed", "seam"])
def test_short_tracks_match_checker(name):
    G.case_short_tracks(name)


@pytest.mark.parametrize("name", ["mixed", "single", "seam", "edges"])
def test_point_errors_match_checker(name):
    G.case_point_errors(name)


def test_empty_model():
    G.case_empty_model()


def test_input_validation():
    G.case_input_validation()


def test_manager_applies_deletions():
    G.case_manager_applies_deletions()


def test_known_answers_of_the_reference():
    T.known_answers(OM.ObservationManager)


def test_subsets_and_single_rules():
    G.case_subsets_and_single_rules()


def test_point_filtering_command_round_trip(tmp_path):
    T.command_round_trip(tmp_path, manager=None)
