"""The host-only plan of PatchMatch (colmap_amd/csrc/pm_host_plan.h): tests/cpp/test_pm_host_plan.cc checks the input
validation, pose tables, shape scalars, source-image span, re-homing order, run compatibility, run shape, sweep
schedule with its parameter blocks and the sub-batch sizes against brute-force code of its own. Compiled with g++ alone:
the header needs neither the HIP runtime nor the library. The second build runs the same program under the address and
undefined-behaviour sanitizers: the rejected problems sit in exactly sized heap arrays, so a read through a bad index
before its check would be reported."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan_against_brute_force(tmp_path, sanitize):
    exe = str(tmp_path / "test_pm_host_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_pm_host_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "pm host plan checks OK" in r.stdout
