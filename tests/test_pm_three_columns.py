"""GPU: three columns per wave (pm_sweep_quad_kernel at C = 3) through the automatic path against the oracle and
against the two-column run of the same build, bit for bit, with the prune and without -- tests/pm_three_columns_cases.py
says why each shape is what it is. The stand-in twin is tests/test_pm_three_columns_emul.py."""
import pytest

import pm_three_columns_cases as T

pytestmark = pytest.mark.gpu
SMALL = False


def _lib():
    from colmap_amd import mvs
    return mvs.lib()


@pytest.mark.parametrize("prune", [1, 0], ids=["prune", "single_stage"])
@pytest.mark.parametrize("name", T.NAMES)
def test_three_columns_equal_two_and_the_oracle(pm_oracle, request, name, prune):
    T.check(pm_oracle, _lib(), request, name, SMALL, prune)
