"""colmap_amd/csrc/model_align.hip -- the scoring kernels, the transform and their host code with the search loop of
align_plan.h -- run on the CPU through the stand-in build of the unmodified source (tests/hip_emul/build_align.sh),
against tests/align_reference.py. The GPU tests run the same case functions through the hipcc build
(tests/test_alignment_gpu.py)."""
import ctypes as C
import os
import subprocess

import pytest

import test_alignment_gpu as G
from colmap_amd import alignment as AL

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_lib = None


def emul_lib():
    global _lib
    if _lib is None:
        root = os.path.join(EMUL, "..", "..")
        so, src = os.path.join(EMUL, "libalign_emul.so"), os.path.join(root, "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("model_align.hip", "align_plan.h", "camera_projection.h")]
        deps += [os.path.join(EMUL, "hip", "hip_runtime.h"), os.path.join(root, "include", "colmap_amd_align.h"),
                 os.path.join(root, "include", "colmap_amd", "camera_models.hpp"),
                 os.path.join(root, "include", "colmap_amd", "bundle_adjustment.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_align.sh")])
        _lib = C.CDLL(so)
        _lib.align_last_error.restype = C.c_char_p
        _lib.align_destroy.restype = None
        _lib.align_destroy.argtypes = [C.c_void_p]
    return _lib


def have_host_compiler():
    return os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or "HIP_EMUL_CXX" in os.environ


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library AL.lib() returns -- what the GPU cases call -- is the CPU build."""
    if not have_host_compiler():
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(AL, "lib", emul_lib)


@pytest.fixture
def edge_scorer():
    with AL.ReprojScorer(AL.flatten_pair(*G.edge_pair())) as scorer:
        yield scorer


def test_emulated_library_is_the_one_under_test():
    assert AL.lib() is emul_lib()
    assert hasattr(AL.lib(), "align_reproj_score")
    G.case_tile_size()


def test_pair_has_the_shapes():
    G.case_pair_shape()


@pytest.mark.parametrize("B", G.batch_sizes())
def test_reproj_score_matches_checker(edge_scorer, B):
    G.case_reproj_score(edge_scorer, B)


def test_reproj_batch_invariance(edge_scorer):
    G.case_reproj_batch_invariance(edge_scorer)


@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("N", [3, 64, 65, 1000])
def test_position_score_matches_checker(N, B):
    G.case_position_score(N, B)


def test_position_batch_invariance():
    G.case_position_batch_invariance()


@pytest.mark.parametrize("B", [1, 7, 64])
def test_search_matches_checker(B):
    G.case_search_matches_checker(B)


@pytest.mark.parametrize("name", ["min_num_trials", "max_num_trials", "dynamic_stop"])
def test_search_edges(name):
    G.case_search_edges(name)


def test_search_too_few_images():
    G.case_search_too_few_images()


def test_public_functions():
    G.case_public_functions()


@pytest.mark.parametrize("N", [1, 257, 1000])
def test_transform_matches_host(N):
    G.case_transform(N)


def test_validation():
    G.case_validation()


def test_empty_inputs():
    G.case_empty_inputs()
