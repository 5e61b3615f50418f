"""Colour extraction without a GPU: the exported symbols, the host-only plan (colmap_amd/csrc/color_plan.h) through a
stand-alone g++ program and through color_slot_layout of the hipcc-built library, how rare the exception of the GPU
parity rule is on the model of tests/test_color_extraction_gpu.py, and the loud failure without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import color_reference as CR
import test_color_extraction_gpu as TG
from colmap_amd import color_extraction as CE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from colmap_amd import build
    build.build()


def test_abi_exports_every_declared_color_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colmap_amd_color.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(color_[a-z0-9_]+)\s*\(", text)))
    assert {"color_create", "color_add_image", "color_finish", "color_samples", "color_destroy", "color_last_error",
            "color_slot_layout", "color_timing"} == set(names)
    from colmap_amd import build
    lib = ctypes.CDLL(build.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan_program(tmp_path, sanitize):
    """The slot layout of a 5-point model, and a duplicate slot, an out-of-range slot and a non-monotone ptr each refused
    with a message: tests/cpp/test_color_plan.cc, compiled with g++ alone."""
    exe = str(tmp_path / "test_color_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_color_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "color plan checks OK" in r.stdout


def test_slot_layout_of_the_library_matches_the_checker():
    rng = np.random.default_rng(3)
    n, P = 500, 60
    obs_point, obs_image = rng.integers(0, P, n), rng.integers(1, 9, n)
    obs_p2d = rng.permutation(n)
    ptr, slot = CE.SlotLayout(obs_point, obs_image, obs_p2d, P)
    want_ptr, want_slot = CR.slot_layout(obs_point, obs_image, obs_p2d, P)
    assert np.array_equal(ptr, want_ptr) and np.array_equal(slot, want_slot)
    assert sorted(slot) == list(range(n))
    with pytest.raises(CE.ColorError, match="point index 60 out of range"):
        CE.SlotLayout([0, 60], [1, 1], [0, 1], P)


def test_model_slots_match_the_checker_layout():
    TG.case_layout_matches_checker()


def test_checker_eligibility_share_is_small():
    """Observation coordinates have generic fractional parts: the share of channels whose double mean lies within 1e-4
    of a half-integer is about 2e-4 in expectation and must stay under the 1 % cap on the GPU tests' model."""
    e = TG.expected()
    assert e["near_half"].mean() <= 0.01
    assert e["valid"].sum() > 100 and (~e["valid"]).sum() >= 9
    k = e["pids"].index(TG.BLANK_POINT)
    assert e["count"][k] == 0 and tuple(e["colours"][k]) == (0, 0, 0)
    assert e["count"][e["pids"].index(TG.LONG_POINT)] == 71


def test_no_gpu_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(CE.ColorError, match="no HIP device available"):
        CE.ColorExtractor(4)
    model, bitmaps = TG.solid_model({1: (20, 40, 220)})
    TG.write_images(bitmaps, str(tmp_path))
    with pytest.raises(CE.ColorError, match="no HIP device available"):
        CE.ExtractColorsForAllImages(model, str(tmp_path))
    with pytest.raises(CE.ColorError, match="no HIP device available"):
        CE.ExtractColorsForImage(model, 1, str(tmp_path))
