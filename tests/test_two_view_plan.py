"""The host-only plan of two-view geometry estimation (colmap_amd/csrc/two_view_plan.h): tests/cpp/test_two_view_plan.cc
drives the LORANSAC walk with a scripted backend against hand-written traces -- the stop inside a sample's model loop, a
sample without a model, min_num_trials, the clamp, local refits that stop at the first non-improvement and at ten,
several sets that park and resume in shared launches -- and checks the trial budget, the router on every branch of
EstimateTwoViewGeometry, the option checks, the layout, the sample draw, the solvers on exact data and the decisions.
Compiled with g++ alone: the header needs neither the HIP runtime nor the library. The second build runs the same
stand-alone program under the address and undefined-behaviour sanitizers. The Jacobi SVD is compared with
numpy.linalg.svd on a 2N x 9 homography system in pixel units."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, sanitize):
    exe = str(tmp_path / "test_two_view_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_two_view_plan.cc"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan_against_traces(tmp_path, sanitize):
    r = subprocess.run([_build(tmp_path, sanitize)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "two-view plan checks OK" in r.stdout


def test_jacobi_svd_against_numpy(tmp_path):
    """A 2N x 9 DLT system in pixel units (condition number around 1e6): the singular values agree to a few ulps of the
    largest, and the null vector to the bound of a backward-stable SVD, 64 eps sigma_1 / (sigma_8 - sigma_9)."""
    exe = _build(tmp_path, [])
    rng = np.random.default_rng(3)
    Ht = np.array([[1.1, 0.02, 30.0], [-0.03, 0.95, -12.0], [1e-5, -2e-5, 1.0]])
    for n, noise in ((5, 0.0), (40, 0.0), (200, 0.5)):
        p1 = np.stack([rng.uniform(0, 1000, n), rng.uniform(0, 800, n)], 1)
        q = (Ht @ np.hstack([p1, np.ones((n, 1))]).T).T
        p2 = q[:, :2] / q[:, 2:] + noise * rng.normal(size=(n, 2))
        A = np.zeros((2 * n, 9))
        for i, ((x1, y1), (x2, y2)) in enumerate(zip(p1, p2)):
            A[2 * i] = [x1, y1, 1, 0, 0, 0, -x2 * x1, -x2 * y1, -x2]
            A[2 * i + 1] = [0, 0, 0, x1, y1, 1, -y2 * x1, -y2 * y1, -y2]
        path = tmp_path / f"a{n}.txt"
        with open(path, "w") as f:
            f.write(f"{2 * n}\n")
            for row in A:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
        out = subprocess.run([exe, "svd", str(path)], capture_output=True, text=True, check=True).stdout.split("\n")
        sigma = np.array(out[0].split(), np.float64)
        null = np.array(out[1].split(), np.float64)
        _, s, vt = np.linalg.svd(A)
        eps = np.finfo(np.float64).eps
        assert s[0] / s[7] > 1e5                                   # the system is as ill-conditioned as said
        assert np.abs(sigma - s).max() <= 64 * eps * s[0]
        bound = 64 * eps * s[0] / (s[7] - s[8])
        assert min(np.linalg.norm(null - vt[8]), np.linalg.norm(null + vt[8])) <= bound, (n, bound)
        assert abs(np.linalg.norm(null) - 1) < 1e-14
        assert int(out[2]) == (8 if noise == 0.0 else 9)
        if noise == 0.0:   # the eigenvectors of A^T A would have lost this: sigma_9^2 is below eps sigma_1^2
            assert np.linalg.norm(A @ null) <= 64 * eps * s[0]
