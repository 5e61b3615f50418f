"""colmap_amd/csrc/feature_match.hip -- the matching kernel with the int8 matrix instruction, the cache and the host
plan of match_plan.h -- run on the CPU through the stand-in build of the unmodified source
(tests/hip_emul/build_match.sh, which force-includes the stand-in of the matrix instruction, tests/hip_emul/mfma_i8.h),
against tests/match_reference.py. The GPU tests run the same case functions through the hipcc build
(tests/test_feature_matching_gpu.py)."""
import ctypes as C
import os
import subprocess

import pytest

import test_feature_matching_gpu as G
from colmap_amd import feature_matching as FM

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_lib = None


def emul_lib():
    global _lib
    if _lib is None:
        root = os.path.join(EMUL, "..", "..")
        so, src = os.path.join(EMUL, "libmatch_emul.so"), os.path.join(root, "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("feature_match.hip", "match_plan.h")]
        deps += [os.path.join(EMUL, "hip", "hip_runtime.h"), os.path.join(EMUL, "mfma_i8.h"),
                 os.path.join(EMUL, "build_match.sh"), os.path.join(root, "include", "colmap_amd_match.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_match.sh")])
        _lib = FM.declare(C.CDLL(so))
    return _lib


def have_host_compiler():
    return os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or "HIP_EMUL_CXX" in os.environ


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library FM.lib() returns -- what the GPU cases call -- is the CPU build."""
    if not have_host_compiler():
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(FM, "lib", emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert FM.lib() is emul_lib()
    assert hasattr(FM.lib(), "match_pairs")
    G.case_shapes()


@pytest.mark.parametrize("n1,n2", G.SMALL_SIZES + G.LARGE_SIZES)
def test_selection_matches_checker(n1, n2):
    G.case_selection(n1, n2)


def test_asymmetric_exact_integers():
    G.case_asymmetric()


def test_extreme_rows():
    G.case_extremes()


def test_ties_take_the_first_column():
    G.case_ties()


@pytest.mark.parametrize("name", ["defaults", "no_cross_check", "ratio", "distance"])
def test_final_matches(name):
    G.case_options(name)


def test_batch_invariance():
    G.case_batch_invariance()


def test_cache_replace_and_evict():
    G.case_cache()


def test_max_num_matches(capfd):
    G.case_max_num_matches(capfd)


def test_validation():
    G.case_validation()


def test_exhaustive_matcher_command(tmp_path, capsys):
    G.case_exhaustive_matcher_command(tmp_path, capsys)
