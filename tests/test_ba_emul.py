"""colmap_amd/csrc/ba_kernels.hip + ba_schur_explicit.hip -- the UNMODIFIED product sources, host loop and kernels --
executed on the CPU against the fp64 checker (oracle/ba_oracle.c), by running parity tests of tests/test_ba_gpu.py
with the library swapped for a CPU build of the same files.

tests/hip_emul/ is a HIP stand-in for exactly this purpose (the lanes of a workgroup as fibers, cross-lane
primitives and __syncthreads as barriers, v_mfma_f64_16x16x4_f64 with the hardware's operand / result layout,
streams synchronous): test infrastructure, never loaded by the product, whose library is built by hipcc and has
no CPU path. What these tests pin without a GPU: the linearisation of every camera-model family, the c-order /
p-order layouts and the tiled point passes, the wave-per-chunk reductions, the Schur-Jacobi blocks on the (emulated)
matrix cores, the pipelined PCG with its device-side stopping test, the LM loop, both exact tiers (explicit reduced
camera system with fixed-point accumulation, blocked Cholesky), priors, rigs, robust losses, the adapters. Sizes are
the small ones of the GPU suite (a lane is a fiber here: ~1 us per cross-lane primitive and lane). The GPU tests
run the same functions through the hipcc build."""
import ctypes as C
import os
import subprocess

import pytest

import ba_explicit_cases as X
import ba_step_cases as S
import test_ba_gpu as G
from colmap_amd import estimators as est

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_emul")
_CSRC = os.path.join(os.path.dirname(_HERE), "..", "colmap_amd", "csrc")
_LIB = None


def _emul_lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libba_emul.so")
        deps = [os.path.join(_CSRC, f) for f in ("ba_kernels.hip", "ba_schur_explicit.hip", "ba_schur_explicit.h", "ba_layout.h",
                                                   "ba_probe.h")]
        deps += [os.path.join(_HERE, "hip", "hip_runtime.h"), os.path.join(_HERE, "rccl", "rccl.h"),
                 os.path.join(_HERE, "build_ba.sh"), os.path.join(os.path.dirname(_HERE), "..", "include", "colmap_amd_ba.h"),
                 os.path.join(os.path.dirname(_HERE), "..", "include", "colmap_amd", "camera_models.hpp")]
        if not os.path.exists(path) or any(os.path.getmtime(d) > os.path.getmtime(path) for d in deps):
            subprocess.check_call(["sh", os.path.join(_HERE, "build_ba.sh")])
        _LIB = C.CDLL(path)
        _LIB.ba_last_error.restype = C.c_char_p
    return _LIB


@pytest.fixture(autouse=True)
def emulated_library(monkeypatch):
    """est.solve_flat(..., gpu_index=0) -- what the GPU tests call -- reaches ba_solve of the CPU build."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and "HIP_EMUL_CXX" not in os.environ:
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(est, "lib", _emul_lib)


def test_emulated_library_is_the_one_under_test():
    L = est.lib()
    assert L is _emul_lib() and os.path.basename(L._name) == "libba_emul.so"
    est._check_abi(L)


@pytest.mark.parametrize("frames,points,track,mixed", [(6, 40, 4, True), (12, 300, 5, False)])
def test_solution_matches_oracle(frames, points, track, mixed):
    G.test_solution_matches_oracle(frames, points, track, mixed)


def test_constant_blocks_gauges_and_partial_problems():
    G.test_constant_blocks_are_untouched_bitwise()
    G.test_shared_intrinsics_and_three_point_gauge()
    G.test_heavy_blocks_reduce_their_chunks_first()
    G.test_pair_terms_per_incidence_equal_per_observation()
    G.test_only_points_variable_and_only_cameras_variable()
    G.test_error_behaviour()
    G.test_iteration_callback_stops_with_the_last_accepted_state()


def test_reference_backend_cases_and_golden_fixture():
    G.test_backend_interface_reference_cases()
    G.test_against_committed_golden_fixture()
    G.test_reference_pose_prior_backend_case()


def test_exact_tiers():
    """DENSE_SCHUR / AUTO against the checker's exact tier; explicit formation against operator products."""
    G.test_dense_schur_tier_matches_oracle()
    G.test_exact_tier_explicit_formation_equals_operator_products()
    G.test_exact_tier_pair_major_formation_equals_point_major(60, 3000, 6, True)


def test_blocked_cholesky_beyond_one_panel():
    """n_c = 700: eleven 64-wide panels, three outer panels of 256, the two-stream lookahead order; the panel and
    trailing-update kernels on the emulated matrix cores (four waves per workgroup)."""
    fp = G._flat(120, 1500, 6, seed=120)
    assert est.fix_gauge_two_cams(fp)
    (a, want), (b, got) = G._both(fp, max_num_iterations=3, linear_solver_type=est.SOLVER_AUTO)
    assert got.linear_solver_used == want.linear_solver_used == est.SOLVER_SPARSE_SCHUR
    assert (got.log_linear_iters[:got.num_iterations] == 1).all()
    import numpy as np
    np.testing.assert_allclose(got.log_cost, want.log_cost, rtol=1e-7)
    np.testing.assert_allclose(b.poses, a.poses, atol=1e-6)


@pytest.mark.parametrize("model", [9, 14, 17])
def test_camera_model_families(model):
    """RADIAL_FISHEYE, SIMPLE_FISHEYE (no distortion parameter), EQUIRECTANGULAR; SIMPLE_RADIAL / PINHOLE / OPENCV
    variants run in the mixed problems above."""
    params = {9: (900.0, 512.0, 384.0, 0.03, -0.004), 14: (900.0, 512.0, 384.0), 17: (1024.0, 768.0)}[model]
    G._model_matches_oracle(model, params)


def test_rigs_priors_and_robust_loss():
    G.test_rig_frames_match_oracle()
    G.test_constant_rig_from_world_rotation_matches_oracle()
    G.test_pose_prior_adjuster_on_rigs_matches_oracle()
    G.test_robust_losses_match_oracle(est.LossFunctionType.SOFT_L1, 1.0)


# ------------------------------------------------------------------------------------------------
# ba_schur_explicit.h called directly (an internal C++ interface: mangled names): the case functions of
# tests/ba_explicit_cases.py on host buffers; tests/test_ba_explicit_gpu.py runs the same cases on the hipcc build
# ------------------------------------------------------------------------------------------------

def _host():
    return X.HostBuffers(_emul_lib())


@pytest.mark.parametrize("scale,expect_bad", [(0.1, False), (100.0, True)])
def test_fixed_point_formation_and_its_overflow_flag(scale, expect_bad):
    """form_kernel<.., FIXED> on two observations of one point against numpy, exact to the quantum; a term the fixed
    point cannot hold raises FormArgs::bad, finish() poisons S[0][0] and the factorisation answers NaN."""
    X.case_fixed_point_overflow(_host(), scale, expect_bad)


@pytest.mark.parametrize("shared_cams,rigs,fixed", [(False, False, True), (True, False, True), (True, True, True),
                                                    (True, True, False)])
def test_pair_major_formation_against_numpy_and_the_point_major_kernel(shared_cams, rigs, fixed):
    """form() both ways on a random linearisation -- per-image cameras; cameras shared between images (their blocks are
    reached from many pairs of images, and a pair of observations of one shared block meets its diagonal twice); rig
    frames (several images per pose block: runs of one pair of pose blocks change their targets) -- with constant poses,
    cameras, sensors and points and 5-wide pose blocks: the pair-major formation (records, incidence lists sorted by
    pose pair, one wave per 64 incidences) and the point-major kernel (one atomic per term) against numpy, fixed-point
    and fp64 accumulation. Widths 10 and 20 (kd = 4)."""
    P = X.formation_problem(11 + 2 * shared_cams + rigs, 9, 60, shared_cams, rigs)
    X.case_formation(_host(), P, fixed, legacy_bars=True)


@pytest.mark.parametrize("kd,rigs,fixed", [(8, False, True), (4, True, False), (16, False, True), (16, True, True),
                                           (16, True, False)])
def test_formation_widths_and_chunked_tracks(kd, rigs, fixed):
    """Widths 14 (kd = 8), 20, 28 (kd = 16, exactly full with a variable sensor) of both formations, with tracks of
    1 / 2 / 15 / 16 / 17 / 33 observations: form_kernel stages a point 16 observations at a time, so these reach its
    second and third chunk, and for the constant points with 17 and 33 observations the chunks it skips."""
    X.case_formation(_host(), X.formation_problem(100 + kd + rigs, 12, 40, True, rigs, kd=kd, long_tracks=True), fixed)


@pytest.mark.parametrize("fixed", [True, False])
def test_prior_rows_and_lm_diagonal(fixed):
    X.case_prior_rows_and_lm_diagonal(_host(), fixed)


@pytest.mark.parametrize("n,min_rows128", [(45, 12 * 128), (64, 12 * 128), (333, 12 * 128), (900, 256)])
def test_blocked_cholesky_directly_against_numpy(n, min_rows128):
    """factor_solve on a random SPD matrix: the factor, the stored inverses of its diagonal blocks and the solution
    against numpy, and the componentwise backward bounds. n = 45 / 64: one (short / full) diagonal block --
    chol_diag_kernel alone (blocked over 16 x 16 tiles, the inverse of the triangle riding along); 333: six panels, a
    ragged last block, two outer panels; 900 with the tile threshold lowered: the 128 x 128 trailing update (the columns
    right of the next outer panel) with its register prefetch, including diagonal tiles and a ragged edge."""
    X.case_cholesky(_host(), n, min_rows128)


@pytest.mark.parametrize("n", [1, 65, 255, 256, 257])
def test_blocked_cholesky_around_block_and_panel_edges(n):
    X.case_cholesky(_host(), n)


def test_blocked_cholesky_lookahead_call_order():
    """The two-stream call order (synchronous here: the overlap itself is a GPU test) on three outer panels."""
    X.case_cholesky(_host(), 600, 256, lookahead=True)


def test_blocked_cholesky_reports_a_failed_pivot():
    X.case_failed_pivot(_host(), 100, 70)


def test_blocked_cholesky_reports_a_failed_pivot_in_a_later_outer_panel():
    X.case_failed_pivot(_host(), 300, 270)


@pytest.mark.parametrize("n,j0", [(64, 0), (130, 0), (130, 1), (333, 0), (333, 2), (333, 5)])
def test_tri_inverse_directly(n, j0):
    X.case_tri_inverse(_host(), n, j0)


def test_extract_cov_blocks_directly():
    X.case_extract_cov_blocks(_host())


# ------------------------------------------------------------------------------------------------
# the iterative tier step by step through the probe (colmap_amd/csrc/ba_probe.h): the small cases of
# tests/ba_step_cases.py; tests/test_ba_steps_gpu.py runs all of them on the hipcc build
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,split", [("plain", True), ("narrow", False), ("kd8", True), ("kd16", True)])
def test_steps_of_the_width_tiers(kind, split):
    S.case_tier(_emul_lib(), kind, split)


def test_steps_with_jacobi_scaling_and_a_robust_loss():
    S.case_jacobi_scaling(_emul_lib())
    S.case_loss(_emul_lib(), est.LossFunctionType.CAUCHY, 2.0)


@pytest.mark.parametrize("model", S.OTHER_MODELS)
def test_linearisation_of_the_other_models_against_the_checker(model):
    S.case_model(_emul_lib(), model)


def test_steps_of_rig_frames_and_position_priors():
    L = _emul_lib()
    S.case_rig(L, False)
    S.case_rig(L, True)
    S.case_priors(L, est.LossFunctionType.TRIVIAL)
    S.case_priors(L, est.LossFunctionType.CAUCHY)


def test_steps_of_pair_terms_heavy_blocks_chunk_edges_and_degenerate_problems():
    L = _emul_lib()
    S.case_shared_intrinsics(L, True)
    S.case_shared_intrinsics(L, False)
    S.case_heavy_blocks(L)
    S.case_chunk_edges(L)
    S.case_tiles(L, "pts")
    S.case_degenerate(L, "points_only")
    S.case_degenerate(L, "cameras_only")


# ------------------------------------------------------------------------------------------------
# sharded solves: N > 1 ranks of the HIP solver on the CPU (gloo + the sum-over-ranks callback)
# ------------------------------------------------------------------------------------------------

def _emul_sharded_worker(*args, **kw):
    """Child process of the sharded GPU tests (spawned: a fresh interpreter): the same worker, its library swapped."""
    from colmap_amd import estimators as est_child
    est_child.lib = _emul_lib
    import test_ba_gpu as G_child
    G_child._sharded_worker(*args, **kw)


@pytest.fixture
def sharded_workers_on_the_stand_in(monkeypatch):
    monkeypatch.setattr(G, "_sharded_worker", _emul_sharded_worker)


def test_two_rank_point_sharded_solve(sharded_workers_on_the_stand_in):
    """ba_solve_sharded, observations sharded by point, two ranks: every rank linearises its own observations, one
    fused all-reduce per linearisation and one per implicit product; ranks agree bitwise and with the single-rank solve."""
    G.test_two_rank_sharded_solve_matches_single_gpu(est.SHARD_BY_POINT, False)


def test_three_rank_image_sharded_solve_with_shared_intrinsics(sharded_workers_on_the_stand_in):
    """Image sharding over three ranks with intrinsics blocks shared across ranks: the all-reduced incidence products
    (ba_inc_* kernels) give the sharded solve the single-rank Schur-Jacobi preconditioner -- the same CG iteration counts."""
    G.test_three_rank_sharded_solve_with_shared_intrinsics(est.SHARD_BY_IMAGE)


def test_two_rank_sharded_exact_tier(sharded_workers_on_the_stand_in):
    """DENSE_SCHUR sharded by point: the ranks' explicitly formed partial systems are summed (fixed point) and factored."""
    G.test_two_rank_sharded_exact_tier(est.SHARD_BY_POINT)


# ------------------------------------------------------------------------------------------------
# COLMAP_AMD_TEST_SLOW=1: the remaining comparisons of the GPU suite that take 15-100 s each on the stand-in
# ------------------------------------------------------------------------------------------------

_slow = pytest.mark.skipif(os.environ.get("COLMAP_AMD_TEST_SLOW", "0") == "0", reason="COLMAP_AMD_TEST_SLOW=1 runs the long stand-in cases")


@_slow
def test_slow_kernel_variants():
    G.test_split_linearisation_is_bit_identical(False)
    G.test_split_linearisation_is_bit_identical("three")
    for m in ("SIMPLE_RADIAL", "PINHOLE", "SIMPLE_PINHOLE"):
        G.test_plain_linearisation_is_bit_identical(m)
    G.test_run_to_run_determinism()
    G.test_tracks_longer_than_a_tile()


@_slow
def test_slow_models_priors_and_operator_precision():
    G.test_variable_sensor_from_rig_matches_oracle()
    G.test_radial_model_matches_oracle()
    G.test_opencv_model_matches_oracle()
    G.test_position_priors_match_oracle(est.LossFunctionType.TRIVIAL)
    G.test_position_priors_match_oracle(est.LossFunctionType.CAUCHY)
    G.test_robust_losses_match_oracle(est.LossFunctionType.CAUCHY, 1.0)
    G.test_robust_losses_match_oracle(est.LossFunctionType.HUBER, 2.0)
    G.test_fp32_operator_reaches_the_fp64_solution(40, 2000, 8, True)
    G.test_solution_matches_oracle(40, 2000, 8, True)
