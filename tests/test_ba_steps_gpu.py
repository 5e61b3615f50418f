"""The iterative tier of colmap_amd/csrc/ba_kernels.hip step by step on the GPU: the step probe (colmap_amd/csrc/ba_probe.h)
stops the solver after each named step of Solver::run and every result is compared with an independent value -- the
linearisation with the checker, everything after it with longdouble arithmetic on the device's own residuals and Jacobian
(tests/ba_step_cases.py; tests/test_ba_emul.py runs the small cases on the CPU stand-in). Every case asserts the path
facts that name it."""
import pytest
import torch  # noqa: F401  before the library is loaded: the two then share one HIP runtime (tests/test_ba_explicit_gpu.py)

import ba_step_cases as S
from colmap_amd import estimators as est

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from colmap_amd import _lib
    yield _lib.lib()
    print("\nlargest error / bar per step:", {k: float("%.3g" % v) for k, v in S.RATIOS.items()})


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("kind", ["plain", "narrow", "kd8", "kd12", "kd16"])
def test_width_tiers(lib, kind, split):
    S.case_tier(lib, kind, split)


def test_plain_model_through_the_generic_kernels(lib):
    S.case_tier(lib, "plain", True, plain=False)


def test_jacobi_scaling(lib):
    S.case_jacobi_scaling(lib)


@pytest.mark.parametrize("model", S.OTHER_MODELS)
def test_linearisation_of_the_other_models(lib, model):
    S.case_model(lib, model)


@pytest.mark.parametrize("loss,scale", [(est.LossFunctionType.CAUCHY, 2.0), (est.LossFunctionType.HUBER, 1.0)])
def test_robust_losses(lib, loss, scale):
    S.case_loss(lib, loss, scale)


@pytest.mark.parametrize("variable_sensors", [False, True])
def test_rig_frames(lib, variable_sensors):
    S.case_rig(lib, variable_sensors)


@pytest.mark.parametrize("loss", [est.LossFunctionType.TRIVIAL, est.LossFunctionType.CAUCHY])
def test_position_priors_take_the_step_by_step_pcg(lib, loss):
    S.case_priors(lib, loss)


@pytest.mark.parametrize("incidences", [True, False])
def test_shared_intrinsics_pair_terms(lib, incidences):
    S.case_shared_intrinsics(lib, incidences)


def test_heavy_blocks(lib):
    S.case_heavy_blocks(lib)


def test_chunk_edges(lib):
    S.case_chunk_edges(lib)


@pytest.mark.parametrize("kind", ["pts", "obs511", "obs512", "obs513", "track512", "track513"])
def test_point_tiles(lib, kind):
    S.case_tiles(lib, kind)


def test_fp32_operator(lib):
    S.case_tiles(lib, "pts", operator_f32=True)


@pytest.mark.parametrize("kind", ["points_only", "cameras_only"])
def test_degenerate_problems(lib, kind):
    S.case_degenerate(lib, kind)
