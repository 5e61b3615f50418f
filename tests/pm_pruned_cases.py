"""The smallest PatchMatch problems at which the two-stage P4 of the 11 x 11 wave kernels (pm_kernels.hip:
sweep_wave_body -- stage 1 = hypotheses 1..4 against a column's first two drawn views, then a hypothesis whose partial
cost sum already exceeds the finished sum of hypothesis 0 is pruned: its other evaluations are never listed) can go
wrong: ties at the bound, columns without a second stage, rows whose second stage is empty, rows where nothing is pruned,
every column count, a last group of one column, more tasks than a batch holds, the geometric pass and the helper wave.
Shared by the GPU tests (tests/test_pm_pruned.py) and their stand-in twin (tests/test_pm_pruned_emul.py, `small` shapes).

Every case compares every output map (depth, normal, cost, selection probability, consistency mask) as 32-bit patterns,
NaN positions included, with the oracle -- which knows no prune -- and with the same build under COLMAP_AMD_PM_PRUNE=0,
whose evaluation count the pruned run must report unchanged.

    problem(name, small) -> (views, ref, src, maps or None, option overrides)

The pruned counter is one number per run. Where a scene claims "nothing may be pruned here" for a part of the image
(flat_block: the interior of the constant block), the claim is asserted on the scene in which that part is the whole
image (flat_all), and the mixed scene is held to the oracle's bits."""
import dataclasses

import numpy as np

from colmap_amd import synthetic as syn
from pm_common import hip_problem, oracle_inputs, paired_options, scene
from pm_answered_cases import flat_rect
from pm_round_record_cases import ALL, assert_same_bits, with_switch  # noqa: F401

SWITCH = "COLMAP_AMD_PM_PRUNE"
_PHOTO = dict(geom_consistency=0, filter=1, num_iterations=1, columns_per_group=2)


def size(small):
    return (48, 36) if small else (96, 72)


def _ring(S, w, h, arc=24.0):
    views = list(scene(S + 1, w, h, arc))
    ref = S // 2
    return views, ref, [i for i in range(S + 1) if i != ref]


def problem(name, small):
    w, h = size(small)
    if name == "s5":
        # S = 5, M = 4: a column draws 1..4 distinct views, so rows mix columns with and without a second stage
        views, ref, src = _ring(5, w, h)
        return views, ref, src, None, dict(_PHOTO, num_samples=4)
    if name == "converged":
        # the second iteration starts from a converged first one: the current plane beats most of the propagated and
        # perturbed ones after two views, and the second stage of many rows has no task and no round
        views, ref, src = _ring(5, w, h)
        return views, ref, src, None, dict(_PHOTO, num_samples=4, num_iterations=2)
    if name == "few_draws":
        # M = 2 draws: no column ever has a third drawn view, so no row has a second stage; first sweep, random start
        views, ref, src = _ring(5, w, h)
        return views, ref, src, None, dict(_PHOTO, num_samples=2, max_sweeps=1)
    if name == "one_source":
        # S = 1, M = 1: one drawn view at most, the bound IS the finished sum
        views, ref, src = _ring(1, w, h)
        return views, ref, src, None, dict(_PHOTO, num_samples=1)
    if name == "two_sources":
        # S = 2, M = 3: both views fit the first stage whatever is drawn
        views, ref, src = _ring(2, w, h)
        return views, ref, src, None, dict(_PHOTO, num_samples=3)
    if name in ("flat_block", "flat_all"):
        # a constant reference patch costs 2.0 against every view under every hypothesis: all five sums of a pixel tie, the
        # bound of a hypothesis with a view waiting lies BELOW the sum of hypothesis 0, nothing may be pruned, and the tie
        # must still go to the highest index (the oracle's bits). flat_all: the whole reference is such a patch (grey 0,
        # like what the window reads beyond the image's edge)
        views, ref, src = _ring(5, w, h)
        gray = views[ref].gray.copy()
        if name == "flat_all":
            gray[:] = 0
        else:
            x0, y0, bw, bh = flat_rect(small)
            gray[y0:y0 + bh, x0:x0 + bw] = 128
        views[ref] = dataclasses.replace(views[ref], gray=gray)
        return views, ref, src, None, dict(_PHOTO, num_samples=4)
    if name.startswith("cols"):
        # every column count of the wave kernels at an image width that leaves the last group ONE column:
        # 97 = 48 x 2 + 1 = 32 x 3 + 1 = 24 x 4 + 1, stand-in 49 = 24 x 2 + 1 = 16 x 3 + 1 = 12 x 4 + 1
        views, ref, src = _ring(5, w + 1, h)
        return views, ref, src, None, dict(_PHOTO, num_samples=4, columns_per_group=int(name[4:]))
    if name == "s20":
        # the benchmark's S = 20, M = 15 in all four sweep directions: up to 2 x 4 x 13 second-stage tasks against 56
        # slots per batch, and draws without a view
        ws, hs = (24, 18) if small else (64, 48)
        views = list(scene(21, ws, hs, 3.6 * 20))
        return views, 10, [i for i in range(21) if i != 10], None, dict(_PHOTO)
    if name == "geom":
        # geometric consistency with both filters: the waiting entries of the geometric cost read +0 in the bound too
        views, ref, src = _ring(5, w, h)
        maps = [(v.depth.copy(), v.normal.copy()) for v in views]
        return views, ref, src, maps, dict(geom_consistency=1, filter=1, num_iterations=1, columns_per_group=2,
                                           num_samples=4)
    raise KeyError(name)


_WANT = {}


def oracle_answer(pm_oracle, name, small):
    """The oracle's maps of a problem (device order), computed once per session and never modified."""
    key = (name, small)
    if key not in _WANT:
        views, ref, src, maps, opt = problem(name, small)
        dmin, dmax = syn.depth_range(views, ref)
        o, _ = paired_options(pm_oracle, depth_min=dmin, depth_max=dmax, **opt)
        _WANT[key] = pm_oracle.run(o, oracle_inputs(views, maps is not None, maps), ref, src, want_cost=True)
    return _WANT[key]


def solve(pm_oracle, name, small):
    from colmap_amd import mvs
    views, ref, src, maps, opt = problem(name, small)
    dmin, dmax = syn.depth_range(views, ref)
    _, h = paired_options(pm_oracle, depth_min=dmin, depth_max=dmax, **opt)
    pm = mvs.PatchMatch(h, hip_problem(views, ref, src, maps))
    pm.Run()
    got = dict(depth=pm.GetDepthMap(), normal=pm.GetNormalMap(), sel_prob=pm.GetSelProbMap(), cost=pm.GetCostMap(),
               mask=pm.GetConsistencyMask())
    counts = dict(evaluations=pm.GetEvaluationCount()[0], answered=pm.GetAnsweredCount()[0], pruned=pm.GetPrunedCount(),
                  kernel=pm.GetSweepKernelName())
    return got, counts


def check(pm_oracle, lib, name, small, kernel="pm_sweep_quad_kernel"):
    """The pruned run against the oracle and against the single-stage run of the same build; returns the pruned run's
    counters."""
    from switches import set_switch
    want = oracle_answer(pm_oracle, name, small)
    got, counts = solve(pm_oracle, name, small)
    set_switch(lib, SWITCH, "0")
    try:
        plain, plain_counts = solve(pm_oracle, name, small)
    finally:
        set_switch(lib, SWITCH, None)
    print(f"{name}: pruned run {counts}, single-stage run {plain_counts}")
    assert_same_bits(want, got, ALL)
    assert_same_bits(plain, got, ALL)
    assert counts["kernel"] == plain_counts["kernel"] == kernel, (counts, plain_counts)
    assert plain_counts["pruned"] == 0, plain_counts
    assert counts["evaluations"] == plain_counts["evaluations"], (counts, plain_counts)
    assert counts["pruned"] + counts["answered"] <= counts["evaluations"], counts
    return counts
