"""The C++ surface of SIFT extraction (include/colmap_amd/feature_extraction.hpp) from g++:
tests/cpp/test_sift_host.cc, compiled and linked against the library like tests/test_cpp_host.py compiles its host
programs."""
import subprocess

import pytest

import test_cpp_host


@pytest.fixture(scope="session")
def sift_host(tmp_path_factory):
    return test_cpp_host._compile("test_sift_host", tmp_path_factory)


def test_cpp_keypoint_and_options(sift_host):
    r = subprocess.run([sift_host, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stderr


def test_cpp_extractor_without_a_gpu_fails_loudly(sift_host):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sift_host, "nodevice"], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device available" in r.stderr


@pytest.mark.gpu
def test_cpp_extractor_finds_a_blob(sift_host):
    r = subprocess.run([sift_host, "blob"], capture_output=True, text=True)
    assert r.returncode == 0 and "blob OK" in r.stdout, r.stderr
