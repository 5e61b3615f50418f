"""The host-only plan of SIFT extraction (colmap_amd/csrc/sift_plan.h): tests/cpp/test_sift_plan.cc checks the options
and their messages, the octave sizes with odd halves, the sigmas and the `sa > sb` tests, the Gaussian taps and the
exp(-x) table against their stated recipe, the order key, the candidate capacity and its growth, the cut to
max_num_features with the level that crosses the limit kept whole, and the UBC permutation. Compiled with g++ alone: the
header needs neither the HIP runtime nor the library. The second build runs the same stand-alone program under the address
and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan(tmp_path, sanitize):
    exe = str(tmp_path / "test_sift_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_sift_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "sift plan checks OK" in r.stdout
