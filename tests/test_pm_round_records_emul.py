"""CPU stand-in: the round records of the 11 x 11 wave kernels (pm_kernels.hip: batch_publish, ncc_rounds_wave) against the oracle,
bit for bit, at the smallest shapes at which the list handling can go wrong -- tests/pm_round_record_cases.py says why
each shape is what it is. The twin of tests/test_pm_round_records.py: the same checks through the CPU build of the unmodified kernels
(tests/test_pm_emul.py), at the stand-in's shapes."""
import pytest

import pm_round_record_cases as R
from test_pm_emul import _emul_lib, emulated_library  # noqa: F401  (autouse fixture: mvs.lib -> the CPU build)

SMALL = True


def _lib():
    return _emul_lib()


@pytest.mark.parametrize("name", ["odd_s5", "odd_s7", "one_task"])
def test_task_count_not_a_multiple_of_four(pm_oracle, name):
    """P6 batches of S - distinct tasks (odd counts, and a single task): the last round is padded, never stored."""
    R.check(pm_oracle, name, SMALL)


def test_more_tasks_than_one_batch(pm_oracle):
    """C = 2, S = 20, M = 15: up to 120 P4 tasks in batches of 56, 56 and 8 -- a later batch must not see an earlier
    batch's records or sums."""
    R.check(pm_oracle, "three_batches", SMALL, R.SWEPT)


def test_rounds_all_inside_all_outside_and_mixed(pm_oracle):
    """Sources smaller than the reference: n_inside = 6 on interior rows (not a multiple of four, by construction:
    pm_round_record_cases._border), falling to 0 at the border. The oracle's census confirms that the solve met taps on
    and beyond the border as well as interior ones."""
    counts = R.check(pm_oracle, "border", SMALL, census=True)
    assert 0 < counts["tap_outside"] <= counts["tap_border"] < counts["taps"], counts


def test_pair_kernel(pm_oracle, request):
    """The helper wave learns n_inside from the mailbox: mixed batches (border) and odd task counts (S = 5, M = 3). The
    kernel is forced with COLMAP_AMD_PM_HELP=2: the plan picks it by itself only for images of 512 pixels and more
    (PlanRunShape), far beyond a test's size, so the automatic choice is not what is tested here -- the kernel is."""
    R.with_switch(request, _lib(), "COLMAP_AMD_PM_HELP", "2")
    R.check(pm_oracle, "border", SMALL, kernel="pm_sweep_pair_kernel")
    R.check(pm_oracle, "odd_s5", SMALL, kernel="pm_sweep_pair_kernel")


def test_explicit_index_build(pm_oracle, request):
    R.with_switch(request, _lib(), "COLMAP_AMD_PM_FP_GLOBAL", "1")
    R.check(pm_oracle, "border", SMALL, kernel="pm_sweep_quad_kernel (explicit indices)")
    R.check(pm_oracle, "odd_s5", SMALL, kernel="pm_sweep_quad_kernel (explicit indices)")


def test_geometric_variant_with_both_filters(pm_oracle):
    R.check(pm_oracle, "border_geom", SMALL)


@pytest.mark.parametrize("name", ["initial_s3", "initial_s20"])
def test_initial_cost_wave_kernel(pm_oracle, name):
    """pm_initial_cost_wave_kernel, the other caller of ncc_rounds_wave: batches of 6 (S = 3) and of 40 (S = 20). For
    S = 3 (sources smaller than the reference) the oracle's census checks what pm_round_record_cases._border claims of
    the scene: some taps are clamped at the border, and more than half of all taps are interior ones -- there are
    evaluations on both sides, in batches of six."""
    counts = R.check(pm_oracle, name, SMALL, R.INITIAL, kernel=None, census=(name == "initial_s3"))
    if name == "initial_s3":
        assert 0 < counts["tap_border"] < counts["taps"] // 2, counts
