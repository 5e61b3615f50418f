"""colmap_amd/csrc/fusion.hip on the GPU at its product capacities, on the paths no other GPU test reaches: the stack of a
walk crossing from LDS into its HBM spill, the spill overflowing and growing (clamped, by the factor 4, twice), medians
above the staging size (radix select), a wave's record buffer filling, table tiers 1 and 0, overlap lists past 32 and
past 64 entries. tests/fusion_capacity_cases.py holds the inputs, shows from the checker alone that each reaches its
path, and compares with the checker's mode 1 bit for bit, twice. tests/test_fusion_capacity_emul.py runs the same cases
on the CPU stand-in."""
import pytest

import fusion_capacity_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def target():
    return K.gpu_target()


@pytest.mark.parametrize("side", ["below", "above"])
def test_hip_fusion_stack_in_lds_and_in_the_spill(target, side):
    K.case_stack_lds_border(target, side)


@pytest.mark.parametrize("name", list(K.SPILL_CASES))
def test_hip_fusion_spill_overflow_and_growth(target, name):
    K.case_spill(target, name)


@pytest.mark.parametrize("cap", list(K.MEDIAN_CASES))
def test_hip_fusion_staged_and_radix_select_medians(target, cap):
    K.case_median(target, cap)


def test_hip_fusion_record_buffer_full(target):
    K.case_record_buffer(target)


@pytest.mark.parametrize("tier", [0, 1])
def test_hip_fusion_table_tier_chosen_by_the_plan(target, tier):
    K.case_planned_tier(target, tier)


@pytest.mark.parametrize("tier", [0, 1])
def test_hip_fusion_table_tier_forced(target, tier):
    K.case_forced_tier(target, tier)


@pytest.mark.parametrize("n", K.OVERLAP_IMAGES)
def test_hip_fusion_overlap_list_lengths(target, n):
    K.case_overlap_length(target, n)
