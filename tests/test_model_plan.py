"""The host-only plan of the model statistics (colmap_amd/csrc/model_plan.h): tests/cpp/test_model_plan.cc checks the
input validation, the by-image observation order, the lane-group and selection classes, the pair totals, the limits and
the rows made of a count table against brute-force code of its own. Compiled with g++ alone: the header needs neither the
HIP runtime nor the library. The second build runs the same stand-alone program under the address and
undefined-behaviour sanitizers: the rejected inputs sit in exactly sized heap arrays, so a read through a bad offset or
index before its check would be reported."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan_against_brute_force(tmp_path, sanitize):
    exe = str(tmp_path / "test_model_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_model_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "model plan checks OK" in r.stdout
