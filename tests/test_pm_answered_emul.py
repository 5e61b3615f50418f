"""CPU stand-in: the answered task class of the 11 x 11 wave kernels (pm_patch_class.h; pm_kernels.hip: task_class,
batch_publish) against the oracle, bit for bit -- tests/pm_answered_cases.py says why each scene is what it is. The twin
of tests/test_pm_answered.py: the same checks through the CPU build of the unmodified kernels (tests/test_pm_emul.py), at
the stand-in's shapes."""
import pytest

import pm_answered_cases as A
from test_pm_emul import _emul_lib, emulated_library  # noqa: F401  (autouse fixture: mvs.lib -> the CPU build)

SMALL = True


def _lib():
    return _emul_lib()


def test_one_view_beside(pm_oracle):
    """Trailing answered tasks in counts that are not multiples of four: every pixel's evaluation against the displaced
    view is cut by the oracle at src_var, with all of its taps outside."""
    counts, answered = A.check(pm_oracle, "one_view_beside", SMALL)
    w, h = A.size(SMALL)
    assert counts["ncc_cut_src_var"] >= w * h and counts["tap_outside"] >= 121 * w * h, counts
    assert counts["ncc_cut_ref_var"] == 0, counts


def test_all_views_beside(pm_oracle):
    """Batches that run no round at all. Most evaluations of the solve are cut at src_var and most taps are outside (not
    all: a random plane at a grazing angle stretches its window back over the image). The initial cost's batches are the
    four evaluations of a column pair (the width is even), so its count moves in fours -- a batch with one task left to
    run runs all four -- and every four counted is a batch that ran no round; displaced by three widths, that is the
    majority of the pixels."""
    counts, answered = A.check(pm_oracle, "all_views_beside", SMALL)
    assert 2 * counts["ncc_cut_src_var"] > counts["ncc_evals"] and 2 * counts["tap_outside"] > counts["taps"], counts
    w, h = A.size(SMALL)
    assert answered[1] % 4 == 0 and w * h < answered[1] <= 2 * w * h, answered


def test_all_views_beside_pair_kernel(pm_oracle, request):
    """The helper wave meets a batch without rounds."""
    A.with_switch(request, _lib(), "COLMAP_AMD_PM_HELP", "2")
    A.check(pm_oracle, "all_views_beside", SMALL, kernel="pm_sweep_pair_kernel")


def test_all_views_beside_explicit_indices(pm_oracle, request):
    A.with_switch(request, _lib(), "COLMAP_AMD_PM_FP_GLOBAL", "1")
    A.check(pm_oracle, "all_views_beside", SMALL, kernel="pm_sweep_quad_kernel (explicit indices)")


def test_half_beside(pm_oracle):
    """All three classes along a row: taps inside, on the border and outside, and evaluations that are not cut."""
    counts, _ = A.check(pm_oracle, "half_beside", SMALL)
    assert 0 < counts["tap_outside"] < counts["tap_border"] < counts["taps"], counts
    assert 0 < counts["ncc_cut_src_var"] < counts["ncc_evals"] // 2, counts


def test_half_beside_pair_kernel(pm_oracle, request):
    A.with_switch(request, _lib(), "COLMAP_AMD_PM_HELP", "2")
    A.check(pm_oracle, "half_beside", SMALL, kernel="pm_sweep_pair_kernel")


def test_half_beside_explicit_indices(pm_oracle, request):
    A.with_switch(request, _lib(), "COLMAP_AMD_PM_FP_GLOBAL", "1")
    A.check(pm_oracle, "half_beside", SMALL, kernel="pm_sweep_quad_kernel (explicit indices)")


def test_half_beside_geometric_variant_with_both_filters(pm_oracle):
    counts, _ = A.check(pm_oracle, "half_beside_geom", SMALL)
    assert 0 < counts["ncc_cut_src_var"] < counts["ncc_evals"] // 2, counts


def test_flat_block(pm_oracle):
    """A constant block larger than the window in the reference: its interior pixels are flat (the oracle cuts their
    evaluations at ref_var), its rim and the rest of the image are not."""
    counts, answered = A.check(pm_oracle, "flat_block", SMALL)
    w, h = A.size(SMALL)
    assert A.flat_interior(SMALL) * 4 <= counts["ncc_cut_ref_var"] < w * h * 4 // 2, counts
    assert answered[1] >= A.flat_interior(SMALL) * 4, (answered, A.flat_interior(SMALL))


@pytest.mark.parametrize("name", ["one_view_beside_initial", "all_views_beside_initial", "half_beside_initial"])
def test_initial_cost_wave_kernel(pm_oracle, name):
    """max_sweeps = 0: pm_initial_cost_wave_kernel alone."""
    counts, answered = A.check(pm_oracle, name, SMALL)
    assert counts["ncc_cut_src_var"] > 0 and counts["ncc_cut_ref_var"] == 0, counts


def test_all_inside_answers_nothing(pm_oracle):
    """Sources at the reference's pose: the outside rule must not fire once (and the texture has no flat patch)."""
    counts, answered = A.check(pm_oracle, "all_inside", SMALL, expect_answered=False)
    assert counts["ncc_cut_ref_var"] == 0, counts
    assert answered == (0, 0), answered
