"""The smallest PatchMatch problems at which the third task class of the 11 x 11 wave kernels -- "answered": the patch lies
wholly beside its source image (three window sums of +0), or the reference patch is flat (cost 2 whatever the sums);
pm_patch_class.h, pm_kernels.hip: batch_publish -- can go wrong: trailing answered tasks in counts that are not
multiples of four, batches that run no round at all, all three classes in one batch, and a batch with nothing to answer.
Shared by the GPU tests (tests/test_pm_answered.py) and their stand-in twin (tests/test_pm_answered_emul.py, `small`
shapes). Every output map is compared with the oracle as 32-bit patterns, NaN positions included; the oracle's census
confirms what each scene claims and bounds the answered count from above: an answered task is an evaluation the oracle
cuts at `ref_var < 1e-5 || src_var < 1e-5`.

    problem(name, small) -> (views, ref, src, maps or None, option overrides)

A source is put "beside" the reference's footprint by moving its principal point: same pose, same positive projective
divisor, every projection displaced by a multiple of the image width."""
import dataclasses

import numpy as np

from colmap_amd import synthetic as syn
from pm_common import hip_problem, oracle_inputs, paired_options, scene
from pm_round_record_cases import ALL, INITIAL, assert_same_bits, with_switch  # noqa: F401

_PHOTO = dict(geom_consistency=0, filter=1, num_iterations=1, columns_per_group=2)
_INITIAL = dict(geom_consistency=0, filter=0, max_sweeps=0, columns_per_group=2)


def size(small):
    return (48, 36) if small else (96, 72)


def _shifted(view, dx):
    """The same camera with its principal point moved by dx pixels: every projection moves with it."""
    K = view.K.copy()
    K[0, 2] += np.float32(dx)
    return dataclasses.replace(view, K=K)


def _ring(S, small, arc=24.0):
    w, h = size(small)
    views = list(scene(S + 1, w, h, arc))
    ref = S // 2
    return views, ref, [i for i in range(S + 1) if i != ref]


# block of constant grey in the reference image of flat_block: (x0, y0, width, height); the window is 11 x 11
def flat_rect(small):
    return (16, 10, 16, 15) if small else (40, 24, 24, 21)


def flat_interior(small):
    """Pixels whose whole window lies in the block."""
    _, _, bw, bh = flat_rect(small)
    return (bw - 10) * (bh - 10)


def problem(name, small):
    w, _ = size(small)
    initial = name.endswith("_initial")
    base = name[:-len("_initial")] if initial else name
    opt = dict(_INITIAL) if initial else dict(_PHOTO)
    if base == "one_view_beside":
        # S = 3, the last source three image widths to the right. Initial cost: 2 columns x 3 views = 6 tasks, 2 of them
        # answered behind 4 that run; a border column has 3 tasks, 1 answered. P6: the winner against the views not
        # drawn, M = 2 draws leave 1 or 2 of 3.
        views, ref, src = _ring(3, small)
        views[src[-1]] = _shifted(views[src[-1]], 3 * w)
        return views, ref, src, None, dict(opt, num_samples=2)
    if base == "all_views_beside":
        # S = 2, both sources beside (one to the right, one to the left): every batch is answered, none runs a round
        views, ref, src = _ring(2, small)
        views[src[0]] = _shifted(views[src[0]], 3 * w)
        views[src[1]] = _shifted(views[src[1]], -3 * w)
        return views, ref, src, None, dict(opt, num_samples=1)
    if base == "half_beside":
        # S = 5; two sources see only one half of the reference's footprint each (moved by 0.55 widths, one to each
        # side): along a row the patches of such a source go from wholly beside it over its border into its interior
        views, ref, src = _ring(5, small)
        views[src[0]] = _shifted(views[src[0]], -0.55 * w)
        views[src[-1]] = _shifted(views[src[-1]], 0.55 * w)
        return views, ref, src, None, dict(opt, num_samples=3)
    if base == "half_beside_geom":
        views, ref, src, _, _ = problem("half_beside", small)
        maps = [(v.depth.copy(), v.normal.copy()) for v in views]
        return views, ref, src, maps, dict(geom_consistency=1, filter=1, num_iterations=1, columns_per_group=2,
                                           num_samples=3)
    if base == "flat_block":
        # S = 4: a column pair with one flat and one textured pixel is a batch of 4 + 4, so no answered task shares a
        # round with one that runs and the answered count of the initial cost is at least interior x S
        views, ref, src = _ring(4, small)
        x0, y0, bw, bh = flat_rect(small)
        gray = views[ref].gray.copy()
        gray[y0:y0 + bh, x0:x0 + bw] = 128
        views[ref] = dataclasses.replace(views[ref], gray=gray)
        return views, ref, src, None, dict(opt, num_samples=2)
    if base == "all_inside":
        # sources at the reference's own pose: every homography is the identity, nothing lies beside anything
        views, ref, src = _ring(3, small)
        for s in src:
            views[s] = dataclasses.replace(views[ref])
        return views, ref, src, None, dict(opt, num_samples=2)
    raise KeyError(name)


_WANT = {}


def oracle_answer(pm_oracle, name, small):
    """The oracle's maps (device order) and census counters of a problem, computed once per session."""
    key = (name, small)
    if key not in _WANT:
        views, ref, src, maps, opt = problem(name, small)
        dmin, dmax = syn.depth_range(views, ref)
        o, _ = paired_options(pm_oracle, depth_min=dmin, depth_max=dmax, **opt)
        _WANT[key] = pm_oracle.run_census(o, oracle_inputs(views, maps is not None, maps), ref, src, want_cost=True)
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
    return got, pm


def check(pm_oracle, name, small, kernel="pm_sweep_quad_kernel", expect_answered=True):
    """Same bits as the oracle; the answered counters against the census. Returns (census, (sweep, initial) answered)."""
    want, counts = oracle_answer(pm_oracle, name, small)
    got, pm = solve(pm_oracle, name, small)
    initial = name.endswith("_initial")
    assert_same_bits(want, got, INITIAL if initial else ALL)
    if kernel is not None and not initial:
        assert pm.GetSweepKernelName() == kernel
    answered = pm.GetAnsweredCount()
    cut = counts["ncc_cut_src_var"] + counts["ncc_cut_ref_var"]
    print(f"{name}: answered {answered}, census cut src_var {counts['ncc_cut_src_var']} ref_var {counts['ncc_cut_ref_var']}"
          f" of {counts['ncc_evals']} evaluations, taps outside {counts['tap_outside']} of {counts['taps']}")
    if expect_answered:
        assert 0 < sum(answered) <= cut, (answered, counts)
        assert answered[1] > 0 and (initial) == (answered[0] == 0), answered
    return counts, answered
