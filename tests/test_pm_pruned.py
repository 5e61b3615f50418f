"""GPU: the two-stage P4 of the 11 x 11 wave kernels and its prune (pm_kernels.hip: sweep_wave_body) against the oracle
and against the single-stage run of the same build, bit for bit -- tests/pm_pruned_cases.py says why each scene is what
it is. The stand-in twin is tests/test_pm_pruned_emul.py."""
import pytest

import pm_pruned_cases as P

pytestmark = pytest.mark.gpu
SMALL = False


def _lib():
    from colmap_amd import mvs
    return mvs.lib()


def test_mixed_rows_prune_something(pm_oracle):
    counts = P.check(pm_oracle, _lib(), "s5", SMALL)
    assert counts["pruned"] > 0, counts


def test_second_iteration_prunes_whole_rows(pm_oracle):
    """Second stages without a task or a round."""
    counts = P.check(pm_oracle, _lib(), "converged", SMALL)
    assert counts["pruned"] > 0, counts


def test_ties_at_the_bound_prune_nothing(pm_oracle):
    """Every cost is 2.0: a bound below the sum of hypothesis 0, never above it, and ties to the highest index."""
    counts = P.check(pm_oracle, _lib(), "flat_all", SMALL)
    assert counts["pruned"] == 0, counts


def test_flat_block(pm_oracle):
    P.check(pm_oracle, _lib(), "flat_block", SMALL)


@pytest.mark.parametrize("name", ["one_source", "two_sources", "few_draws"])
def test_no_second_stage(pm_oracle, name):
    """No column has more drawn views than the first stage takes: the bound is the finished sum."""
    counts = P.check(pm_oracle, _lib(), name, SMALL)
    assert counts["pruned"] == 0, counts


@pytest.mark.parametrize("columns", [1, 2, 3, 4])
def test_columns_per_group_and_a_last_group_of_one_column(pm_oracle, columns):
    counts = P.check(pm_oracle, _lib(), f"cols{columns}", SMALL)
    assert counts["pruned"] > 0, counts


def test_bench_source_count_all_four_directions(pm_oracle):
    counts = P.check(pm_oracle, _lib(), "s20", SMALL)
    assert counts["pruned"] > 0, counts


def test_geometric_variant_with_both_filters(pm_oracle):
    counts = P.check(pm_oracle, _lib(), "geom", SMALL)
    assert counts["pruned"] > 0, counts


@pytest.mark.parametrize("name", ["converged", "geom"])
def test_pair_kernel(pm_oracle, request, name):
    """Two waves per column group, what one problem alone runs at full size. That kernel is compiled without the prune
    (pm_kernels.hip: kPairPrune -- it measured slower with it), so the switch changes nothing in it: same bits, same
    evaluation count, nothing pruned."""
    P.with_switch(request, _lib(), "COLMAP_AMD_PM_HELP", "2")
    counts = P.check(pm_oracle, _lib(), name, SMALL, kernel="pm_sweep_pair_kernel")
    assert counts["pruned"] == 0, counts


def test_explicit_indices(pm_oracle, request):
    P.with_switch(request, _lib(), "COLMAP_AMD_PM_FP_GLOBAL", "1")
    P.check(pm_oracle, _lib(), "s5", SMALL, kernel="pm_sweep_quad_kernel (explicit indices)")
