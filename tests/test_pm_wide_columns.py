"""The host-only step that gives a run three columns per wave (colmap_amd/csrc/pm_host_plan.h: PlanWideColumns):
tests/cpp/test_pm_wide_columns.cc runs it behind PlanRunShape over the benchmark's launch, one or two problems alive,
small images, requested columns, the COLS / HELP / WIDE switches, the geometric pass, S = 32 and the neighbours of S = 21,
a shape that does not fit, another window and the two neighbours of the oversubscription threshold. Compiled with g++
alone; the second build runs the same program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_wide_columns_plan(tmp_path, sanitize):
    exe = str(tmp_path / "test_pm_wide_columns")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_pm_wide_columns.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pm wide columns checks OK" in r.stdout
