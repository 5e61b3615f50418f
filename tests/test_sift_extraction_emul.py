"""colmap_amd/csrc/sift.hip -- the SIFT kernels and their host walk over the octaves -- run on the CPU through the stand-in
build of the unmodified source (tests/hip_emul/build_sift.sh), against tests/sift_reference.py and the VLFeat fixture.
The GPU tests run the same case functions through the hipcc build (tests/test_sift_extraction_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_sift_extraction_gpu as G
from colmap_amd import feature_extraction as FE

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_lib = None


def emul_lib():
    global _lib
    if _lib is None:
        root = os.path.join(EMUL, "..", "..")
        so, src = os.path.join(EMUL, "libsift_emul.so"), os.path.join(root, "colmap_amd", "csrc")
        deps = [os.path.join(src, f) for f in ("sift.hip", "sift_plan.h", "sift_solvers.h")]
        deps += [os.path.join(EMUL, "hip", "hip_runtime.h"), os.path.join(EMUL, "sift", "hipcub", "hipcub.hpp"),
                 os.path.join(EMUL, "build_sift.sh"), os.path.join(root, "include", "colmap_amd_sift.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["sh", os.path.join(EMUL, "build_sift.sh")])
        _lib = C.CDLL(so)
    return _lib


def have_host_compiler():
    return os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or "HIP_EMUL_CXX" in os.environ


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library FE.lib() returns -- what the GPU cases call -- is the CPU build."""
    if not have_host_compiler():
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(FE, "lib", emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert FE.lib() is emul_lib()
    G.case_sizes()


@pytest.mark.parametrize("name", G.CASES)
def test_device_equals_checker(name):
    G.case_device_equals_checker(name)


@pytest.mark.parametrize("name", G.CASES)
def test_device_equals_vlfeat_fixture(name):
    G.case_device_equals_fixture(name)


def test_independence_of_history_and_capacity():
    G.case_independence()


def test_validation():
    G.case_validation()


def test_descriptor_early_return():
    G.case_descriptor_early_return()


def test_scale_back_and_skip(tmp_path):
    G.case_scale_back(tmp_path)


def test_database_round_trip(tmp_path, monkeypatch):
    """feature_extractor -> exhaustive_matcher -> geometric_verifier, each through its CPU build."""
    import test_feature_matching_emul as ME
    import test_two_view_geometry_emul as TE
    from colmap_amd import feature_matching as FM
    from colmap_amd import two_view_geometry as TV
    monkeypatch.setattr(FM, "lib", ME.emul_lib)
    monkeypatch.setattr(TV, "lib", TE.emul_lib)
    G.case_database_round_trip(tmp_path, G.run_main)


def test_c_abi_through_ctypes():
    """include/colmap_amd_sift.h called directly: options, create, extract, counts, copies, errors, timing."""
    import sift_cases as SC
    L = emul_lib()
    L.sift_last_error.restype = C.c_char_p
    L.sift_options_check.restype = C.c_char_p
    L.sift_num_features.restype = C.c_int64
    L.sift_num_features.argtypes = [C.c_void_p]
    L.sift_destroy.restype = None
    L.sift_destroy.argtypes = [C.c_void_p]
    o = FE._Options()
    L.sift_options_init(C.byref(o))
    assert (o.max_num_features, o.first_octave, o.num_octaves, o.octave_resolution, o.max_num_orientations) == (8192, -1, 4, 3, 2)
    assert C.sizeof(FE._Options) == 48 and FE.DETECTION_DTYPE.itemsize == 32
    assert L.sift_options_check(C.byref(o)) == b""
    o.max_num_features = 0
    assert b"max_num_features" in L.sift_options_check(C.byref(o))
    o.max_num_features = 8192
    h = C.c_void_p()
    assert L.sift_create(C.c_int32(0), C.byref(h)) == 0
    c = SC.fixture()["odd67"]
    img = np.ascontiguousarray(c["image"])
    assert L.sift_extract(h, img.ctypes.data_as(C.c_void_p), C.c_int32(img.shape[1]), C.c_int32(img.shape[0]), C.byref(o)) == 0
    n = L.sift_num_features(h)
    assert n == c["num_out"]
    kp = np.zeros((n, 4), np.float32)
    assert L.sift_copy_keypoints(h, kp.ctypes.data_as(C.c_void_p), C.c_int64(n)) == 0
    G.same(kp, c["keypoints"], "keypoints through the C ABI")
    assert L.sift_copy_keypoints(h, kp.ctypes.data_as(C.c_void_p), C.c_int64(n - 1)) != 0
    assert b"capacity" in L.sift_last_error()
    assert L.sift_extract(h, None, C.c_int32(4), C.c_int32(4), C.byref(o)) != 0
    assert L.sift_num_features(h) == 0   # a failed call leaves no result behind
    k, t, s = C.c_double(), C.c_double(), (C.c_double * 4)()
    assert L.sift_extract(h, img.ctypes.data_as(C.c_void_p), C.c_int32(img.shape[1]), C.c_int32(img.shape[0]), C.byref(o)) == 0
    L.sift_last_timing(C.byref(k), C.byref(t), s)
    assert t.value > 0 and abs(sum(s) - k.value) < 1e-9
    L.sift_destroy(h)
