"""CPU stand-in: three columns per wave (pm_sweep_quad_kernel at C = 3) through the automatic path against the
oracle and against the two-column run of the same build, bit for bit, with the prune and without --
tests/pm_three_columns_cases.py says why each shape is what it is. The twin of tests/test_pm_three_columns.py: the same
checks through the CPU build of the unmodified kernels (tests/test_pm_emul.py), at the stand-in's shapes."""
import pytest

import pm_three_columns_cases as T
from test_pm_emul import _emul_lib, emulated_library  # noqa: F401  (autouse fixture: mvs.lib -> the CPU build)

SMALL = True


@pytest.mark.parametrize("prune", [1, 0], ids=["prune", "single_stage"])
@pytest.mark.parametrize("name", T.NAMES)
def test_three_columns_equal_two_and_the_oracle(pm_oracle, request, name, prune):
    T.check(pm_oracle, _emul_lib(), request, name, SMALL, prune)
