"""The camera model table, stated once per language: include/colmap_amd/camera_models.hpp (device code, host code and
the C++ API) and colmap_amd/camera.py (Python). Both are held against tests/golden/camera_models.json, a fixture written
from the reference's sensor/models.h, and so against each other. The names that scene.py and workspace.py export are
derived from the Python table; their expected values are rebuilt here from the fixture, not from the code under test.
No GPU and no library: tests/cpp/test_camera_models.cc includes the table header alone and is built with g++, once
plainly and once as a stand-alone program under the address and undefined-behaviour sanitizers (the out-of-range ids
-1 and 18 must not read past the table)."""
import json
import os
import subprocess

import pytest

from colmap_amd import camera, scene, workspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX_KEYS = ("focal_length_idxs", "principal_point_idxs", "extra_params_idxs")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "camera_models.json")) as f:
        models = json.load(f)
    assert [m["id"] for m in models] == list(range(18))
    return models


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_cpp_table_equals_fixture(tmp_path, golden, sanitize):
    exe = str(tmp_path / "test_camera_models")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_camera_models.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dump = json.loads(r.stdout)
    assert dump["num_models"] == 18 and dump["max_params"] == 16
    assert dump["max_params"] == max(m["num_params"] for m in golden)
    by_id = {m["id"]: m for m in dump["models"]}
    assert sorted(by_id) == list(range(-1, 19))
    for want in golden:
        got = by_id[want["id"]]
        for key in ("name", "num_params", "is_fisheye", "is_spherical") + IDX_KEYS:
            assert got[key] == want[key], (want["id"], key)
        assert got["one_focal"] == (len(want["focal_length_idxs"]) == 1), want["id"]
        assert got["is_perspective"] == (not want["is_spherical"]), want["id"]
    for not_a_model in (-1, 18):
        got = by_id[not_a_model]
        assert got["name"] is None and got["num_params"] < 0
        assert not (got["one_focal"] or got["is_fisheye"] or got["is_spherical"] or got["is_perspective"])


def test_cpp_model_info_equals_fixture(tmp_path, golden):
    """GetCameraModelInfo is what the C++ BundleAdjuster frees parameters by: EQUIRECTANGULAR's (width, height) are in
    none of the three lists."""
    exe = str(tmp_path / "test_camera_model_info")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_camera_model_info.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    by_id = {m["id"]: m for m in json.loads(r.stdout)}
    assert sorted(by_id) == list(range(-1, 19))
    for want in golden:
        got = by_id[want["id"]]
        assert got["known"]
        for key in ("num_params",) + IDX_KEYS:
            assert got[key] == want[key], (want["id"], key)
    assert not by_id[-1]["known"] and not by_id[18]["known"]
    assert all(by_id[17][key] == [] for key in IDX_KEYS)


def test_python_table_equals_fixture(golden):
    assert len(camera.MODELS) == 18
    for want in golden:
        got = camera.model(want["id"])
        for key in ("name", "num_params", "is_fisheye", "is_spherical") + IDX_KEYS:
            assert getattr(got, key) == want[key], (want["id"], key)
    assert camera.model(-1) is None and camera.model(18) is None


def test_exported_names_keep_their_values(golden):
    """scene.MODEL_* and workspace.CAMERA_MODELS as they stood before they were derived from the table."""
    ids = [m["id"] for m in golden]
    for name, key in (("MODEL_NAMES", "name"), ("MODEL_NUM_PARAMS", "num_params"), ("MODEL_FOCAL_IDXS", "focal_length_idxs"),
                      ("MODEL_PP_IDXS", "principal_point_idxs"), ("MODEL_EXTRA_IDXS", "extra_params_idxs")):
        assert getattr(scene, name) == {m["id"]: m[key] for m in golden}, name
    for m in golden:
        assert getattr(scene, m["name"]) == m["id"]
        f, pp = m["focal_length_idxs"], m["principal_point_idxs"]
        # (name, number of parameters, fx, fy, cx, cy): one focal length serves both axes; None where there is none
        want = (m["name"], m["num_params"]) + ((f[0], f[-1], pp[0], pp[1]) if f else (None,) * 4)
        assert workspace.CAMERA_MODELS[m["id"]] == want
    assert sorted(workspace.CAMERA_MODELS) == ids
    assert workspace.CAMERA_MODEL_IDS == {m["name"]: m["id"] for m in golden}


def test_one_camera_class():
    assert scene.Camera is workspace.SparseCamera is camera.Camera
    c = scene.Camera(3, scene.PINHOLE, 640, 480, [500.0, 510.0, 320.0, 240.0])
    assert (c.camera_id, c.model_id, c.width, c.height) == (3, 1, 640, 480)
    assert c.CalibrationMatrix().tolist() == [[500.0, 0.0, 320.0], [0.0, 510.0, 240.0], [0.0, 0.0, 1.0]]


def test_public_headers_compile_together(tmp_path):
    """One translation unit with every C++ header: before colmap_amd::Camera was one type, bundle_adjustment.hpp and
    undistortion.hpp each defined it and this failed with "redefinition of 'struct colmap_amd::Camera'"."""
    headers = ("bundle_adjustment.hpp", "ba_covariance.hpp", "undistortion.hpp", "observation_manager.hpp", "mvs.hpp",
               "model.hpp")
    src = tmp_path / "all_headers.cc"
    src.write_text("".join(f'#include "colmap_amd/{h}"\n' for h in headers) +
                   "static_assert(std::is_same<colmap_amd::obs::Camera, colmap_amd::Camera>::value, \"one Camera\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
