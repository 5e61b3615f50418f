"""The host-only plan of descriptor matching (colmap_amd/csrc/match_plan.h): tests/cpp/test_match_plan.cc checks the
finish on scripted (idx, best, second) triples (all-zero row, best == second, a single column, the thresholds' edges, the
cross check, the min_num_inliers cut), the tile table for sizes 0, 1, 16, 17, around the tile and for mixed batches, the
device image of a set with the exactness of the biased product over the full 0..255, and the argument checks. Compiled
with g++ alone: the header needs neither the HIP runtime nor the library. The second build runs the same stand-alone
program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan(tmp_path, sanitize):
    exe = str(tmp_path / "test_match_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_match_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "match plan checks OK" in r.stdout
