"""The exact-tier kernels of colmap_amd/csrc/ba_schur_explicit.hip on the GPU, each called directly and compared with a
plain numpy reference (tests/ba_explicit_cases.py; tests/test_ba_emul.py runs the small cases on the CPU stand-in).
What only hardware can show is pinned here: the operand / result layout of v_mfma_f64_16x16x4_f64, the 64-bit integer
atomics of the fixed-point formation, and the overlap of the two streams of the Cholesky lookahead."""
import pytest
import torch  # before the library is loaded: the two then share one HIP runtime (ba_explicit_cases.TorchBuffers)

import ba_explicit_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ad():
    from colmap_amd import _lib
    return X.TorchBuffers(_lib.lib())


@pytest.mark.parametrize("scale,expect_bad", [(0.1, False), (100.0, True)])
def test_fixed_point_formation_and_its_overflow_flag(ad, scale, expect_bad):
    X.case_fixed_point_overflow(ad, scale, expect_bad)


@pytest.mark.parametrize("shared_cams,rigs,fixed", [(False, False, True), (True, False, True), (True, True, True),
                                                    (True, True, False)])
def test_formation_short_tracks(ad, shared_cams, rigs, fixed):
    """The problems of the stand-in suite (widths 10 and 20, tracks of 1-7), with its flat bars as well."""
    P = X.formation_problem(11 + 2 * shared_cams + rigs, 9, 60, shared_cams, rigs)
    X.case_formation(ad, P, fixed, legacy_bars=True)


@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("rigs", [False, True])
@pytest.mark.parametrize("kd", [4, 8, 16])
def test_formation_widths_and_chunked_tracks(ad, kd, rigs, fixed):
    """All four instantiated widths -- 10 (kd 4), 14 (kd 8), 20 (kd 4 or 8 with rigs), 28 (kd 16; exactly full with a
    variable sensor) -- of both formations, fixed point and fp64, with tracks of 1 / 2 / 15 / 16 / 17 / 33 observations:
    form_kernel's second and third chunk of 16 staged observations, and the chunks it skips for constant points."""
    X.case_formation(ad, X.formation_problem(100 + kd + rigs, 12, 40, True, rigs, kd=kd, long_tracks=True), fixed)


@pytest.mark.parametrize("fixed", [True, False])
def test_prior_rows_and_lm_diagonal(ad, fixed):
    X.case_prior_rows_and_lm_diagonal(ad, fixed)


@pytest.mark.parametrize("n", [1, 45, 64, 65, 255, 256, 257, 333])
def test_blocked_cholesky(ad, n):
    X.case_cholesky(ad, n)


@pytest.mark.parametrize("n,min_rows128", [(900, 256), (2100, 12 * 128)])
def test_blocked_cholesky_with_and_without_lookahead(ad, n, min_rows128):
    """900 with the tile threshold lowered; 2100 is the production path: default threshold, 128-tiles in the first
    second-stream update, 64-tiles in the next, a ragged last panel. Two runs with lookahead are bit-identical."""
    X.case_cholesky_lookahead(ad, n, min_rows128)


@pytest.mark.parametrize("n,pivot", [(100, 70), (300, 270)])
def test_blocked_cholesky_reports_a_failed_pivot(ad, n, pivot):
    X.case_failed_pivot(ad, n, pivot)


@pytest.mark.parametrize("n,j0", [(64, 0), (130, 0), (130, 1), (333, 0), (333, 2), (333, 5), (900, 3)])
def test_tri_inverse(ad, n, j0):
    X.case_tri_inverse(ad, n, j0)


def test_extract_cov_blocks(ad):
    X.case_extract_cov_blocks(ad)
