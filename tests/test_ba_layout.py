"""The host-only layout of a bundle-adjustment solve (colmap_amd/csrc/ba_layout.h): tests/cpp/test_ba_layout.cc builds
small problems in memory and checks make_layout against brute-force code of its own. Compiled with g++ alone: the
header needs neither the HIP runtime nor the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_against_brute_force(tmp_path):
    exe = str(tmp_path / "test_ba_layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ba_layout.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "layout checks OK" in r.stdout
