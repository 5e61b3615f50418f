"""The bound behind the prune of the 11 x 11 sweep kernels (pm_kernels.hip: sweep_wave_body): tests/cpp/test_pm_prune_bound.cc
accumulates a million random cost sums in draw order in float, with an arbitrary subset of the non-negative terms
replaced by +0, and checks that the partial sum never exceeds the finished one and that a pruned hypothesis loses the
argmin with either value. Compiled with g++ alone (-ffp-contract=off, as in the product's build); the second build runs
the same program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_partial_sum_is_a_lower_bound(tmp_path, sanitize):
    exe = str(tmp_path / "test_pm_prune_bound")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "cpp", "test_pm_prune_bound.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pm prune bound checks OK" in r.stdout
