"""The covariance path of ba_kernels.hip / ba_schur_explicit.hip -- point pass, permuted formation, blocked Cholesky,
triangular inverse on the (emulated) f64 matrix cores, block extraction -- run on the CPU through the stand-in build
of the unmodified sources (tests/hip_emul, see tests/test_ba_emul.py), against tests/ba_cov_reference.py. The GPU
tests run the same case functions through the hipcc build."""
import os

import pytest

import test_ba_covariance_gpu as G
import test_ba_emul
from colmap_amd import estimators as est


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """The library est.lib() returns -- what the GPU cases call -- is the CPU build (same rule as tests/test_ba_emul.py)."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(est, "lib", test_ba_emul._emul_lib)


def test_emulated_library_is_the_one_under_test():
    assert est.lib() is test_ba_emul._emul_lib()
    assert hasattr(est.lib(), "ba_estimate_covariance")


@pytest.mark.parametrize("params,fixed_points,fixed_poses,fixed_intrinsics", G.REFERENCE_CASES)
def test_reference_parameterisations(params, fixed_points, fixed_poses, fixed_intrinsics):
    G.case_reference(params, fixed_points, fixed_poses, fixed_intrinsics)


def test_not_estimable():
    G.case_not_estimable()


def test_crossing_panels():
    G.case_crossing_panels()


def test_conditioning_bound_on_a_panel_crossing_problem():
    """The conditioning-derived bound of the large GPU case, on a smaller problem the stand-in affords."""
    fp = G._flat_problem(48, 150, 8, seed=5, mixed=True)
    est.solve_flat(fp, est.SolverOptions(linear_solver_type=est.SOLVER_DENSE_SCHUR), gpu_index=0)
    G.case_conditioned(fp, G.P.ALL)
    G.case_conditioned(fp, G.P.POSES)
