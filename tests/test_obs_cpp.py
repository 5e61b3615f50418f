"""The C++ surface of observation filtering (include/colmap_amd/observation_manager.hpp) from g++:
tests/cpp/test_obs_host.cc, compiled like tests/test_cpp_host.py compiles its host programs. The host logic (defaults,
flattening, statistics, a rejected model) runs without a GPU; the reference's known answers run on the GPU."""
import subprocess

import pytest

import test_cpp_host


@pytest.fixture(scope="session")
def obs_host(tmp_path_factory):
    return test_cpp_host._compile("test_obs_host", tmp_path_factory)


def test_cpp_host_logic(obs_host):
    r = subprocess.run([obs_host, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stderr


def test_cpp_filter_without_a_gpu_fails_loudly(obs_host):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([obs_host, "nodevice"], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device available" in r.stderr


@pytest.mark.gpu
def test_cpp_known_answers_of_the_reference(obs_host):
    r = subprocess.run([obs_host, "known"], capture_output=True, text=True)
    assert r.returncode == 0 and "known OK" in r.stdout, r.stderr
