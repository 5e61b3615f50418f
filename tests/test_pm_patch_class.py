"""The task classes of the 11 x 11 wave kernels (colmap_amd/csrc/pm_patch_class.h): tests/cpp/test_pm_patch_class.cc
draws more than a million random and adversarial centred homographies and, for every one the outside rule accepts,
restates the per-tap arithmetic of the kernel and checks that all taps have finite coordinates and read the zero ring.
Compiled with g++ alone (-ffp-contract=off: fused multiply-adds only where the source says fmaf, as in the product's
build); the second build runs the same program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_accepted_patches_read_only_the_zero_ring(tmp_path, sanitize):
    exe = str(tmp_path / "test_pm_patch_class")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_pm_patch_class.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pm patch class checks OK" in r.stdout
