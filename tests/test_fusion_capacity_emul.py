"""The cases of tests/fusion_capacity_cases.py through libfusion_emul.so: the unmodified colmap_amd/csrc/fusion.hip at
the PRODUCT's capacities on the CPU stand-in (tests/hip_emul). The twin of tests/test_fusion_capacity_gpu.py: it lets the
GPU tests be rehearsed without a GPU, and it keeps their preconditions -- that each input reaches the path it is named
for, shown by the checker alone -- checked in the CPU suite. The preconditions always run. Where the stand-in needs more
than about ten seconds for a case (seconds in the comments below: walks of thousands of pixels, lane by lane), it runs
the depth-first variant once, or, where that is still too long, only with COLMAP_AMD_TEST_SLOW=1, which runs every case
in full like the GPU does (11 minutes).

The mutations of fusion.hip these cases were tried against are listed in DESIGN.md ("Fusion at its product capacities").
The forced tiers also run in tests/test_fusion_emul.py (test_emulated_kernel_table_tiers); here they only rehearse the
GPU test."""
import os

import pytest

import fusion_capacity_cases as K

_SLOW = os.environ.get("COLMAP_AMD_TEST_SLOW", "0") != "0"
_ONCE = True if _SLOW else "once"


@pytest.fixture(scope="module")
def target():
    return K.emul_target()


@pytest.mark.parametrize("side", ["below", "above"])
def test_emulated_kernel_stack_in_lds_and_in_the_spill(target, side):
    K.case_stack_lds_border(target, side, run=_ONCE)   # in full 20 s, once 6 s


@pytest.mark.parametrize("name", list(K.SPILL_CASES))
def test_emulated_kernel_spill_overflow_and_growth(target, name):
    # in full: T1_* 36 s (once 8 s), clamp 152 s, factor4 80 s, second 114 s
    K.case_spill(target, name, run=_ONCE if name.startswith("T1_") else _SLOW)


@pytest.mark.parametrize("cap", list(K.MEDIAN_CASES))
def test_emulated_kernel_staged_and_radix_select_medians(target, cap):
    K.case_median(target, cap, run=_SLOW)   # 30 s each, 73 s at 10000


def test_emulated_kernel_record_buffer_full(target):
    K.case_record_buffer(target, run=_ONCE)   # in full 17 s, once 5 s


@pytest.mark.parametrize("tier", [0, 1])
def test_emulated_kernel_table_tier_chosen_by_the_plan(target, tier):
    K.case_planned_tier(target, tier)


@pytest.mark.parametrize("tier", [0, 1])
def test_emulated_kernel_table_tier_forced(target, tier):
    if _SLOW:   # 13 s each
        K.case_forced_tier(target, tier)


@pytest.mark.parametrize("n", K.OVERLAP_IMAGES)
def test_emulated_kernel_overlap_list_lengths(target, n):
    K.case_overlap_length(target, n)
