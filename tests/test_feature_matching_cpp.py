"""The C++ surface of descriptor matching (include/colmap_amd/feature_matching.hpp) from g++:
tests/cpp/test_match_host.cc, compiled and linked against the library like tests/test_cpp_host.py compiles its host
programs."""
import subprocess

import pytest

import test_cpp_host


@pytest.fixture(scope="session")
def match_host(tmp_path_factory):
    return test_cpp_host._compile("test_match_host", tmp_path_factory)


def test_cpp_matcher_without_a_gpu_fails_loudly(match_host):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([match_host, "nodevice"], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device available" in r.stderr


@pytest.mark.gpu
def test_cpp_matcher_finds_a_permuted_copy(match_host):
    r = subprocess.run([match_host, "known"], capture_output=True, text=True)
    assert r.returncode == 0 and "known OK" in r.stdout, r.stderr
