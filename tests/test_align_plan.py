"""The host-only plan of model alignment (colmap_amd/csrc/align_plan.h): tests/cpp/test_align_plan.cc checks the input
validation, the wave-padded record layout, the Sim3 algebra, ComputeNumTrials, the sample stream and the LORANSAC loop --
driven by a scripted scorer and compared, for batch sizes 1 to 1000, with a one-at-a-time loop of its own. Compiled with
g++ alone: the header needs neither the HIP runtime nor the library. The second build runs the same stand-alone program
under the address and undefined-behaviour sanitizers: the rejected inputs sit in exactly sized heap arrays, so a read
through a bad index before its check would be reported."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan_against_brute_force(tmp_path, sanitize):
    exe = str(tmp_path / "test_align_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_align_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "align plan checks OK" in r.stdout
