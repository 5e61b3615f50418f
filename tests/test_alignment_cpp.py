"""The C++ surface of model alignment (include/colmap_amd/alignment.hpp) from g++: tests/cpp/test_align_host.cc,
compiled and linked against the library like tests/test_cpp_host.py compiles its host programs. The host logic (Sim3d
files, Inverse, ComputeImageAlignmentError, the association step) runs without a GPU; the alignments run on the GPU."""
import subprocess

import pytest

import test_cpp_host


@pytest.fixture(scope="session")
def align_host(tmp_path_factory):
    return test_cpp_host._compile("test_align_host", tmp_path_factory)


def test_cpp_host_logic(align_host, tmp_path):
    r = subprocess.run([align_host, "host", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stderr


def test_cpp_alignment_without_a_gpu_fails_loudly(align_host):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([align_host, "nodevice"], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device available" in r.stderr


@pytest.mark.gpu
def test_cpp_alignments_recover_a_known_similarity(align_host):
    r = subprocess.run([align_host, "known"], capture_output=True, text=True)
    assert r.returncode == 0 and "known OK" in r.stdout, r.stderr
