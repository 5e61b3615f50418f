"""colmap_amd/csrc/two_view.hip -- the solver and scoring kernels and their host code with the search and the decisions
of two_view_plan.h -- run on the CPU through the stand-in build of the unmodified source
(tests/hip_emul/build_two_view.sh), against tests/two_view_reference.py. The GPU tests run the same case functions
through the hipcc build (tests/test_two_view_geometry_gpu.py)."""
import contextlib
import ctypes as C
import io
import os
import subprocess

import pytest

import test_two_view_geometry_gpu as G
from colmap_amd import two_view_geometry as TV

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_lib = None


def emul_lib():
    global _lib
    if _lib is None:
        root = os.path.join(EMUL, "..", "..")
        so, src = os.path.join(EMUL, "libtwo_view_emul.so"), os.path.join(root, "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("two_view.hip", "two_view_plan.h", "two_view_solvers.h")]
        deps += [os.path.join(EMUL, "hip", "hip_runtime.h"), os.path.join(root, "include", "colmap_amd_tvg.h"),
                 os.path.join(root, "include", "colmap_amd", "camera_models.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_two_view.sh")])
        _lib = C.CDLL(so)
        _lib.tvg_last_error.restype = C.c_char_p
        _lib.tvg_route_name.restype = C.c_char_p
        _lib.tvg_destroy.restype = None
        _lib.tvg_destroy.argtypes = [C.c_void_p]
        _lib.tvg_draw_sample.argtypes = [C.c_int32, C.c_uint64, C.c_int32, C.c_uint64, C.c_uint32, C.c_void_p]
        _lib.tvg_score.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 5
    return _lib


def have_host_compiler():
    return os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or "HIP_EMUL_CXX" in os.environ


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library TV.lib() returns -- what the GPU cases call -- is the CPU build."""
    if not have_host_compiler():
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(TV, "lib", emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert TV.lib() is emul_lib()
    assert TV.model_tile() == 64 and TV.match_tile() == 256 and TV.trial_round() == 64


@pytest.mark.parametrize("kind", G.KINDS, ids=G.KIND_IDS)
def test_scores_are_exact(kind):
    G.case_scores_exact(kind)


@pytest.mark.parametrize("kind", G.KINDS, ids=G.KIND_IDS)
def test_batch_independence(kind):
    G.case_batch_independence(kind)


@pytest.mark.parametrize("kind", G.KINDS[:2], ids=G.KIND_IDS[:2])
def test_minimal_solvers(kind):
    G.case_minimal_solvers(kind)


def test_degenerate_samples():
    G.case_degenerate_samples()


@pytest.mark.parametrize("kind", G.KINDS, ids=G.KIND_IDS)
def test_sample_draw(kind):
    G.case_sample_draw(kind)


@pytest.mark.parametrize("kind", G.KINDS, ids=G.KIND_IDS)
def test_search_properties(kind):
    G.case_search_properties(kind)


@pytest.mark.parametrize("name", sorted(G.scenes()))
def test_scene(name):
    G.case_scene(name)


def test_scenes_in_one_batch():
    G.case_scenes_in_one_batch()


def test_public_function():
    G.case_public_function()


def test_validation():
    G.case_validation()


def test_command(tmp_path):
    from colmap_amd import __main__ as M

    def main(argv):
        err = io.StringIO()
        with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
            rc = M.main(["geometric_verifier"] + argv)
        return rc, err.getvalue()
    G.case_command(tmp_path, main)
