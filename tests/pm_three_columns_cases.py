"""The smallest PatchMatch problems at which three columns per wave (pm_sweep_quad_kernel at C = 3, chosen by
pm_host::PlanWideColumns) can go wrong. Shared by the GPU tests (tests/test_pm_three_columns.py) and their stand-in twin
(tests/test_pm_three_columns_emul.py, `small` shapes).

A run takes three columns on its own only where the GPU is full; COLMAP_AMD_PM_WIDE=2 drops that clause, so that these
images -- far too small to fill anything -- go through the automatic path: no columns requested, pm_pick_columns' two
at create time, three for the run. Every case compares every output map as 32-bit patterns, NaN positions included,
with the oracle and with the same problem at two columns (COLMAP_AMD_PM_WIDE=0), one iteration = all four sweep
directions, filter on.

    problem(name, small) -> (views, ref, src, option overrides, columns requested or 0)

Sizes (stand-in sizes in brackets): the sweep frame is W wide in directions 0 and 2, H wide in 1 and 3.
  65 x 48 [23 x 18]  65 = 21 x 3 + 2: a last group of TWO columns, 22 groups = five workgroups and two surplus waves;
                     48 = 16 x 3: whole groups, whole workgroups  [23 = 7 x 3 + 2, 8 groups; 18 = 6 x 3, 6 groups: two
                     surplus waves]
  64 x 49 [22 x 19]  64 = 21 x 3 + 1 and 49 = 16 x 3 + 1: a last group of ONE column in both orientations, 22 and 17
                     groups  [22 = 7 x 3 + 1, 19 = 6 x 3 + 1: 8 and 7 groups]
"""
from colmap_amd import synthetic as syn
from pm_common import hip_problem, oracle_inputs, paired_options, scene
from pm_round_record_cases import ALL, assert_same_bits, with_switch  # noqa: F401

WIDE, PRUNE = "COLMAP_AMD_PM_WIDE", "COLMAP_AMD_PM_PRUNE"
# a run the library widened says so; three columns at the caller's request report the plain name, as before
WIDE_KERNEL, QUAD_KERNEL = "pm_sweep_quad_kernel (three columns)", "pm_sweep_quad_kernel"
TASK_SLOTS = 56  # pm_kernels.hip: PM_QUAD_CAP, NCC task slots per batch
_PHOTO = dict(geom_consistency=0, filter=1, num_iterations=1)

NAMES = ["last_two", "last_one", "s20", "s21", "s22", "s3_m4"]


def _ring(S, w, h, arc):
    views = list(scene(S + 1, w, h, arc))
    ref = S // 2
    return views, ref, [i for i in range(S + 1) if i != ref]


def problem(name, small):
    two, one = ((23, 18), (22, 19)) if small else ((65, 48), (64, 49))
    if name == "last_two":
        # S = 5, M = 4: 15 (column, view) items, rows that mix columns with and without a second stage
        return _ring(5, *two, 24.0) + (dict(_PHOTO, num_samples=4), 0)
    if name == "last_one":
        return _ring(5, *one, 24.0) + (dict(_PHOTO, num_samples=4), 0)
    if name == "s20":
        # the benchmark's S = 20, M = 15: 60 of 64 lanes in the lane-per-(column, view) phases, 24 stage-1 tasks. One
        # iteration from a random start keeps the selection priors flat, a column draws up to 15 distinct views: up to
        # 3 x 4 x 13 = 156 stage-2 tasks and 3 x 19 winner tasks against 56 slots -- phases of two and three batches
        # (check() asserts from the evaluation counter that P4 overflows the slots)
        return _ring(20, *two, 3.6 * 20) + (dict(_PHOTO), 0)
    if name == "s21":
        # 63 of 64 lanes: the last source count the automatic rule accepts. (M = 13: with 15 samples the block of three
        # columns is 41 008 bytes, 48 more than a workgroup may have, and the run keeps two columns)
        return _ring(21, *one, 3.6 * 21) + (dict(_PHOTO, num_samples=13), 0)
    if name == "s22":
        # 66 (column, view) items: the smallest case in which those phases take a second pass. The automatic rule keeps
        # two columns here (asserted by the caller), so the three columns are the caller's request (M = 9: as above)
        return _ring(22, *two, 3.6 * 22) + (dict(_PHOTO, num_samples=9), 3)
    if name == "s3_m4":
        # S = 3, M = 4: a column that draws ONE distinct view leaves stage 1 short of its eight tasks, and only a column
        # that draws all three has anything left for stage 2 -- rows whose second stage is empty
        return _ring(3, *one, 24.0) + (dict(_PHOTO, num_samples=4), 0)
    raise KeyError(name)


_WANT = {}


def oracle_answer(pm_oracle, name, small):
    """The oracle's maps of a problem (device order), computed once per session and never modified."""
    key = (name, small)
    if key not in _WANT:
        views, ref, src, opt, _ = problem(name, small)
        dmin, dmax = syn.depth_range(views, ref)
        o, _ = paired_options(pm_oracle, depth_min=dmin, depth_max=dmax, **opt)
        _WANT[key] = pm_oracle.run(o, oracle_inputs(views), ref, src, want_cost=True)
    return _WANT[key]


def solve(pm_oracle, name, small, columns):
    from colmap_amd import mvs
    views, ref, src, opt, _ = problem(name, small)
    dmin, dmax = syn.depth_range(views, ref)
    if columns:
        opt = dict(opt, columns_per_group=columns)
    _, h = paired_options(pm_oracle, depth_min=dmin, depth_max=dmax, **opt)
    pm = mvs.PatchMatch(h, hip_problem(views, ref, src))
    pm.Run()
    got = dict(depth=pm.GetDepthMap(), normal=pm.GetNormalMap(), sel_prob=pm.GetSelProbMap(), cost=pm.GetCostMap(),
               mask=pm.GetConsistencyMask())
    counts = dict(evaluations=pm.GetEvaluationCount()[0], pruned=pm.GetPrunedCount(), kernel=pm.GetSweepKernelName())
    pm.close()
    return got, counts


def check(pm_oracle, lib, request, name, small, prune):
    """Three columns per wave against the oracle and against the two-column run of the same build."""
    from switches import set_switch
    with_switch(request, lib, PRUNE, "1" if prune else "0")
    want = oracle_answer(pm_oracle, name, small)
    columns = problem(name, small)[4]
    set_switch(lib, WIDE, "2")
    try:
        got, counts = solve(pm_oracle, name, small, columns)
        if columns:  # ... and what the automatic path makes of this problem: two columns
            _, auto_counts = solve(pm_oracle, name, small, 0)
            assert auto_counts["kernel"] == QUAD_KERNEL, auto_counts
        set_switch(lib, WIDE, "0")
        narrow, narrow_counts = solve(pm_oracle, name, small, 0)
    finally:
        set_switch(lib, WIDE, None)
    print(f"{name}: three columns {counts}, two columns {narrow_counts}")
    assert counts["kernel"] == (QUAD_KERNEL if columns else WIDE_KERNEL), counts
    assert narrow_counts["kernel"] == QUAD_KERNEL, narrow_counts
    assert_same_bits(want, got, ALL)
    assert_same_bits(narrow, got, ALL)
    # the evaluations a row lists do not depend on how the columns are grouped, nor does what the prune drops
    assert counts["evaluations"] == narrow_counts["evaluations"], (counts, narrow_counts)
    assert counts["pruned"] == narrow_counts["pruned"], (counts, narrow_counts)
    if name == "s20":
        # The phases of several batches, from the run's own counter. A pixel's sweep lists 4 evaluations per distinct
        # drawn view in P4 and at most S in P6, so 4 x (mean distinct views) >= e - S with e = evaluations per pixel
        # and sweep; a mean above a third of the cap means that some row of some full group of three columns lists
        # more than TASK_SLOTS evaluations in P4 -- one phase of two batches at least in the single-stage run, whose
        # P4 is that whole list (with the prune the list is split over the stages and a dead hypothesis leaves it:
        # there the overflow of stage 2 is likely, not proven).
        views, _, src, _, _ = problem(name, small)
        h, w = views[0].gray.shape
        e = counts["evaluations"] / (w * h * 4.0)
        print(f"{name}: {e:.2f} evaluations per pixel and sweep, P4 lists at least {3 * (e - len(src)):.1f} per row of three columns")
        assert 3 * (e - len(src)) > TASK_SLOTS, (e, counts)
    if not prune:
        assert counts["pruned"] == 0, counts
    elif name != "s3_m4":  # (few of its rows have a second stage at all: no claim)
        assert counts["pruned"] > 0, counts
    return counts
