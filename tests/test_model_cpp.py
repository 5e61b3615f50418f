"""The C++ surface of the model statistics (include/colmap_amd/model.hpp) from g++: tests/cpp/test_model_host.cc. Linked
to the CPU stand-in build of model_stats.hip (tests/hip_emul/build_model.sh) the reference's known answers run without a
GPU; linked to the library, as tests/test_cpp_host.py links its host programs, they run on the device."""
import os
import subprocess

import pytest

import test_cpp_host
import test_model_statistics_emul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def model_host(tmp_path_factory):
    return test_cpp_host._compile("test_model_host", tmp_path_factory)


@pytest.fixture(scope="session")
def model_host_emul(tmp_path_factory):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    E._emul_lib()  # built, and newer than its sources
    out = str(tmp_path_factory.mktemp("cpp") / "test_model_host_emul")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_model_host.cc"), "-L", E.EMUL, "-l:libmodel_emul.so",
                           "-Wl,-rpath," + E.EMUL, "-o", out])
    return out


def test_cpp_host_logic(model_host):
    r = subprocess.run([model_host, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stderr


def test_cpp_known_answers_on_the_stand_in(model_host_emul):
    r = subprocess.run([model_host_emul, "known"], capture_output=True, text=True)
    assert r.returncode == 0 and "known OK" in r.stdout, r.stderr
    r = subprocess.run([model_host_emul, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stderr


def test_cpp_statistics_without_a_gpu_fail_loudly(model_host):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([model_host, "nodevice"], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device available" in r.stderr


@pytest.mark.gpu
def test_cpp_known_answers_of_the_reference(model_host):
    r = subprocess.run([model_host, "known"], capture_output=True, text=True)
    assert r.returncode == 0 and "known OK" in r.stdout, r.stderr
