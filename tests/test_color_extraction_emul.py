"""colmap_amd/csrc/color_extract.hip -- the sample kernel, the two point kernels and their host code -- run on the CPU
through the stand-in build of the unmodified source (tests/hip_emul/build_color.sh), against tests/color_reference.py.
The GPU tests run the same case functions through the hipcc build (tests/test_color_extraction_gpu.py)."""
import ctypes as C
import os
import subprocess

import pytest

import test_color_extraction_gpu as G
from colmap_amd import _lib as package_lib
from colmap_amd import color_extraction as CE

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_emul = None


def _emul_lib():
    global _emul
    if _emul is None:
        so, src = os.path.join(EMUL, "libcolor_emul.so"), os.path.join(EMUL, "..", "..", "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("color_extract.hip", "color_plan.h")] + \
               [os.path.join(EMUL, "hip", "hip_runtime.h"), os.path.join(EMUL, "..", "..", "include", "colmap_amd_color.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_color.sh")])
        _emul = C.CDLL(so)
    return _emul


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library CE.lib() returns -- what the GPU cases call -- is the CPU build, with the package's prototypes."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(package_lib, "lib", _emul_lib)   # CE.lib() sets argtypes / restype on what this returns


def test_emulated_library_is_the_one_under_test():
    assert CE.lib() is _emul_lib()
    assert hasattr(CE.lib(), "color_add_image")


def test_model_slots_match_checker_layout():
    G.case_layout_matches_checker()


def test_samples_match_checker():
    G.case_samples()


def test_colours_match_checker():
    G.case_colours()


def test_two_runs_are_byte_identical():
    G.case_determinism()


def test_extract_colors_for_all_images(tmp_path):
    G.case_all_images_on_a_model(tmp_path)


def test_reference_known_answer(tmp_path):
    G.case_reference_known_answer(tmp_path)


def test_half_rounds_away_from_zero(tmp_path):
    G.case_half_rounds_away_from_zero(tmp_path)


def test_extract_colors_for_image(tmp_path):
    G.case_for_image(tmp_path)


def test_color_extractor_command(tmp_path):
    G.case_command(tmp_path)


def test_errors():
    G.case_errors()
