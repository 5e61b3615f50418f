"""The smallest PatchMatch problems at which the batch handling of the 11 x 11 wave kernels (pm_kernels.hip:
batch_publish / ncc_rounds_wave -- a round record per position of the inside-first order, batches padded to whole rounds
of four tasks, the unclamped rounds chosen from the count of inside tasks) can go wrong. Shared by the GPU tests
(tests/test_pm_round_records.py) and their stand-in twin (tests/test_pm_round_records_emul.py, `small` shapes: a lane is
a fiber there). Every output map is compared with the oracle as 32-bit patterns.

    problem(name, small) -> (views, ref, src, maps or None, option overrides)

The oracle's answer to a problem is computed once per session and shared by the tests that solve it again through
another kernel (pair, explicit indices)."""
import numpy as np

from colmap_amd import synthetic as syn
from pm_common import hip_problem, oracle_inputs, paired_options, scene

_PHOTO = dict(geom_consistency=0, filter=1, num_iterations=1)


def _ring(S, w, h, arc=24.0):
    views = list(scene(S + 1, w, h, arc))
    ref = S // 2
    return views, ref, [i for i in range(S + 1) if i != ref]


def _border(small):
    """Reference 96 x 72 (stand-in: 48 x 36) against three sources rendered at two thirds of that size from the same
    cameras: the patches of the reference's outer columns and rows fall half outside the sources, the interior ones
    inside. S = 3 at two columns per wave makes every initial-cost batch six tasks: a batch whose patches are all inside
    has n_inside = 6, NOT a multiple of four (one unclamped round, then a clamped round of two inside tasks and two
    padding slots) -- by construction, on every interior row; towards the border the count falls to 0 one view at a
    time (all-outside rounds). The sweeps' P4 batches (4 hypotheses x 3 views x 2 columns = 24) mix the same way."""
    bw, bh, sw, sh = (48, 36, 32, 24) if small else (96, 72, 64, 48)
    big, little = scene(4, bw, bh), scene(4, sw, sh)
    return [little[0], big[1], little[2], little[3]], 1, [0, 2, 3]


def problem(name, small):
    if name in ("odd_s5", "odd_s7"):
        # P6 evaluates the winner against the S - distinct views not drawn: M = 3 draws leave 2..4 of 5 and 4..6 of 7
        S = int(name[-1])
        views, ref, src = _ring(S, *((35, 27) if small else (96, 64)))
        return views, ref, src, None, dict(_PHOTO, num_samples=3)
    if name == "one_task":
        # S = 2, M = 1: one draw per pixel, the winner pass of a column is exactly the other view -- batches of 1 and 2
        views, ref, src = _ring(2, *((35, 27) if small else (96, 64)))
        return views, ref, src, None, dict(_PHOTO, num_samples=1)
    if name == "three_batches":
        # C = 2, S = 20, M = 15: P4 queues up to 2 x 4 x 15 = 120 tasks against 56 slots per batch
        w, h = (24, 18) if small else (64, 48)
        views = list(scene(21, w, h, 3.6 * 20))
        extra = dict(max_sweeps=2) if small else {}
        return views, 10, [i for i in range(21) if i != 10], None, dict(geom_consistency=0, filter=0, num_iterations=1,
                                                                        **extra)
    if name == "border":
        views, ref, src = _border(small)
        return views, ref, src, None, dict(_PHOTO)
    if name == "border_geom":
        views, ref, src = _border(small)
        maps = [(v.depth.copy(), v.normal.copy()) for v in views]
        return views, ref, src, maps, dict(geom_consistency=1, filter=1, num_iterations=1)
    if name == "initial_s3":
        views, ref, src = _border(small)
        return views, ref, src, None, dict(geom_consistency=0, filter=0, max_sweeps=0)
    if name == "initial_s20":
        w, h = (24, 18) if small else (64, 48)
        views = list(scene(21, w, h, 3.6 * 20))
        return views, 10, [i for i in range(21) if i != 10], None, dict(geom_consistency=0, filter=0, max_sweeps=0)
    raise KeyError(name)


_WANT = {}


def oracle_answer(pm_oracle, name, small, census=False):
    """The oracle's maps of a problem (device order), computed once; with `census` through the census build, whose bits
    are the plain build's (tests/test_pm_oracle.py), together with its counters."""
    key = (name, small)
    if key not in _WANT:
        views, ref, src, maps, opt = problem(name, small)
        dmin, dmax = syn.depth_range(views, ref)
        o, _ = paired_options(pm_oracle, depth_min=dmin, depth_max=dmax, **opt)
        imgs = oracle_inputs(views, maps is not None, maps)
        if census:
            _WANT[key] = pm_oracle.run_census(o, imgs, ref, src, want_cost=True)
        else:
            _WANT[key] = (pm_oracle.run(o, imgs, ref, src, want_cost=True), None)
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


def assert_same_bits(want, got, keys):
    for k in keys:
        a, b = np.ascontiguousarray(want[k]), np.ascontiguousarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{k}: {len(bad)} of {a.size} values differ, first at {bad[0]}: "
                                 f"oracle {want[k][tuple(bad[0])]!r} hip {got[k][tuple(bad[0])]!r}")


ALL = ("depth", "normal", "cost", "sel_prob", "mask")
SWEPT = ("depth", "normal", "cost", "sel_prob")
INITIAL = ("depth", "normal", "cost")


def check(pm_oracle, name, small, keys=ALL, kernel="pm_sweep_quad_kernel", census=False):
    want, counts = oracle_answer(pm_oracle, name, small, census)
    got, pm = solve(pm_oracle, name, small)
    assert_same_bits(want, got, keys)
    if kernel is not None:
        assert pm.GetSweepKernelName() == kernel
    return counts


def with_switch(request, lib, name, value):
    from switches import set_switch
    set_switch(lib, name, value)
    request.addfinalizer(lambda: set_switch(lib, name, None))
