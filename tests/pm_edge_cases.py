"""Degenerate PatchMatch problems: the inputs the kernels' border clamps, NaN handling, variance cut-off and divisor-sign
logic exist for, which colmap_amd/synthetic.py's renderer (24 degree arc, band-limited texture, tight depth range,
ground-truth source maps) never produces. Every case is a rendered scene plus deterministic edits -- a VALID problem the
C ABI accepts -- solved for one iteration at 48 x 36 (67 x 45 where a ragged width matters; the CPU stand-in takes
35 x 27 for those), the smallest shapes at which every kernel family still runs more than one column group and more
than one workgroup.

A case names the census counters (oracle/pm_oracle.c: PMO_CENSUS) it exists for, each with a floor: a condition the
oracle's solve of the case must meet for the case to mean anything (tests/test_pm_oracle.py), not a measurement.

    build(name, small) -> Problem(views, ref, src, maps or None, option overrides, (depth_min, depth_max))
"""
import dataclasses
import functools
from typing import NamedTuple, Optional

import numpy as np

from colmap_amd import synthetic as syn
from pm_common import scene


class Problem(NamedTuple):
    views: list
    ref: int
    src: list
    maps: Optional[list]
    options: dict
    depth_range: tuple


def _shape(ragged, small):
    if not ragged:
        return 48, 36
    return (35, 27) if small else (67, 45)


def _with_gray(view, gray):
    return dataclasses.replace(view, gray=np.ascontiguousarray(gray, np.uint8))


def _flat_blocks(view):
    """A mid-grey rectangle larger than the 11 x 11 window, a saturated block and a black block touching two corners."""
    g = view.gray.copy()
    h, w = g.shape
    g[h // 2 - 8:h // 2 + 8, w // 2 - 9:w // 2 + 9] = 128
    g[:min(8, h // 3), :min(8, w // 3)] = 255
    g[h - min(8, h // 3):, w - min(8, w // 3):] = 0
    return _with_gray(view, g)


def _benign(w, h, n=4):
    views = list(scene(n, w, h))
    return views, 1, [i for i in range(n) if i != 1]


def _photometric(**kw):
    return dict(geom_consistency=0, filter=1, num_iterations=1, **kw)


def _case_flat_blocks(small, **opt):
    views, ref, src = _benign(*_shape(True, small))
    views = [_flat_blocks(v) for v in views]
    return Problem(views, ref, src, None, _photometric(**opt), syn.depth_range(views, ref))


def _case_all_constant(small):
    views, ref, src = _benign(*_shape(False, small))
    views = [_with_gray(v, np.full_like(v.gray, 128)) for v in views]
    return Problem(views, ref, src, None, _photometric(), syn.depth_range(views, ref))


def _case_one_constant_source(small):
    views, ref, src = _benign(*_shape(False, small))
    views[src[0]] = _with_gray(views[src[0]], np.full_like(views[src[0]].gray, 90))
    return Problem(views, ref, src, None, _photometric(), syn.depth_range(views, ref))


def _case_ring_360(small, **opt):
    """Six views on the whole ring: sources 2, 3, 4 look from the far side."""
    w, h = _shape(False, small)
    views = list(scene(6, w, h, 360.0))
    return Problem(views, 0, [1, 2, 3, 4, 5], None, _photometric(**opt), syn.depth_range(views, 0))


def _case_wide_depth_range(small):
    views, ref, src = _benign(*_shape(False, small))
    return Problem(views, ref, src, None, _photometric(), (1e-3, 1e4))


def _case_collapsed_depth_range(small):
    views, ref, src = _benign(*_shape(False, small))
    d = float(np.median(views[ref].depth))
    return Problem(views, ref, src, None, _photometric(), (d, d))


def _case_smaller_than_window(small):
    views = list(scene(3, 9, 7))
    return Problem(views, 1, [0, 2], None, _photometric(filter_min_num_consistent=1), syn.depth_range(views, 1))


def _case_narrower_than_column_group(small):
    """3 columns: fewer than the four columns of a generic-family group, one and a half of the wave kernels' pairs."""
    views = list(scene(3, 3, 20))
    return Problem(views, 1, [0, 2], None,
                   _photometric(filter_min_num_consistent=1, columns_per_group=4, threads_per_group=128),
                   syn.depth_range(views, 1))


def _case_source_far_smaller(small):
    """Reference 48 x 36; one source 9 x 7 -- smaller than the window, in a slot the size of the other source."""
    big, tiny = scene(3, 48, 36), scene(3, 9, 7)
    views = [tiny[0], big[1], big[2]]
    return Problem(views, 1, [0, 2], None, _photometric(filter_min_num_consistent=1), syn.depth_range(views, 1))


def _case_source_far_larger(small):
    """Reference 9 x 7, smaller than the window; sources 48 x 36 and 96 x 72 share the larger slot."""
    tiny, mid, big = scene(3, 9, 7), scene(3, 48, 36), scene(3, 96, 72)
    views = [mid[0], tiny[1], big[2]]
    return Problem(views, 1, [0, 2], None, _photometric(filter_min_num_consistent=1), syn.depth_range(views, 1))


def _salt(a, rng, shares):
    """`shares`: (value, share) pairs; disjoint pixel sets drawn from one uniform field."""
    u = rng.random(a.shape[-2:])
    a = a.copy()
    lo = 0.0
    for value, share in shares:
        a[..., (u >= lo) & (u < lo + share)] = value
        lo += share
    return a


def _case_geom_holes(small, normals=False):
    """The geometric pass with both filters. Source depth maps: ground truth with about 10 % holes (0) and 3 % each of
    -1, NaN and +inf. `normals`: the depth maps stay clean and every NORMAL map -- the reference view's is the initial
    state of the solve -- gets 10 % zero vectors and 3 % NaN."""
    w, h = _shape(True, small)
    views = list(scene(3, w, h))
    rng = np.random.default_rng(20240229)
    maps = []
    for i, v in enumerate(views):
        d, n = v.depth.copy(), v.normal.copy()
        if normals:
            n = _salt(n, rng, ((0.0, 0.10), (np.nan, 0.03)))
        elif i != 1:
            d = _salt(d, rng, ((0.0, 0.10), (-1.0, 0.03), (np.nan, 0.03), (np.inf, 0.03)))
        maps.append((d, n))
    return Problem(views, 1, [0, 2], maps, dict(geom_consistency=1, filter=1, num_iterations=1),
                   syn.depth_range(views, 1))


def _case_source_rotated_in_place(small):
    """A source at the reference's own centre, turned by exactly 90 degrees about the vertical axis, with a power-of-two
    focal length and an integer principal point: the projective divisor of a tap is EXACTLY (x - cx) / 64 for every
    plane hypothesis, so the taps of column cx divide by zero -- one coordinate of the chunk is +-inf, the others of
    the shared division NaN -- and half of every window lies behind the source camera."""
    w, h = _shape(True, small)
    arc = syn.make_scene(3, w, h, focal=64.0, arc_deg=24.0)
    K = arc[0].K
    R = np.eye(3, dtype=np.float32)
    T = np.array([0.0, 1.25, 5.0], np.float32)
    turn = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.float32)
    views = [arc[0], arc[2]]
    for Rv, Tv in ((R, T), (turn @ R, turn @ T)):
        g, d, n = syn.render_view(K, Rv, Tv, w, h)
        views.append(syn.View(K, Rv, Tv, g.numpy(), d.numpy(), n.numpy()))
    return Problem(views, 2, [3, 0, 1], None, _photometric(), syn.depth_range(views, 2))


def _case_geom_scaled_normals(small):
    """The geometric pass started from a normal map that is not unit length (a ramp of factors 12 .. 17 across the
    image): the incident-angle likelihood exp(-0.617 (1 - cos)^2) passes through the smallest normal floats and
    through zero, the view-selection weights become subnormal, 1 / prob_sum overflows, and the CDF of a pixel reads
    [inf, .., NaN]: the one situation in which the view draw must scan and not bisect."""
    w, h = 67, 45       # the stand-in too: at 35 x 27 no pixel's weights land in the subnormal window
    views = list(scene(3, w, h))
    ramp = (12.0 + 5.0 * (np.arange(w, dtype=np.float32)[None, :] / (w - 1))
            + 0.05 * np.arange(h, dtype=np.float32)[:, None])
    maps = [(v.depth.copy(), (v.normal * ramp[None]).astype(np.float32) if i == 1 else v.normal.copy())
            for i, v in enumerate(views)]
    return Problem(views, 1, [0, 2], maps, dict(geom_consistency=1, filter=1, num_iterations=1),
                   syn.depth_range(views, 1))


# An 11 x 11 patch of grey levels 0 .. 3 whose bilateral-weighted variance at its centre, ref_sqsum - ref_sum * ref_sum
# as FilterKernel's sums give it (window 11 x 11, sigma_spatial 5, sigma_color 0.2), is the float 1e-5f EXACTLY
# (0x3727c5ac): found by a search over random dark block patterns with the oracle's pmo_filter_ref_image, about one
# window in 10^7 of those whose variance lies in the binade of 1e-5.
_PATCH_AT_CUTOFF = np.array([
    [2, 2, 2, 2, 2, 2, 0, 0, 0, 0, 2], [2, 2, 2, 2, 2, 2, 0, 0, 0, 0, 2], [3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1],
    [3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1], [3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1], [3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1],
    [2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 3], [2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 3], [2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 3],
    [2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 3], [0, 0, 0, 0, 0, 0, 3, 3, 3, 3, 1]], np.uint8)


def _case_variance_at_cutoff(small):
    """The reference image carries _PATCH_AT_CUTOFF: at its centre pixel the reference variance equals the cut-off, so
    `ref_color_var < 1e-5f` is false and the NCC is evaluated against the (textured) sources; `<=` would return 2.0."""
    views, ref, src = _benign(*_shape(False, small))
    g = views[ref].gray.copy()
    g[12:23, 18:29] = _PATCH_AT_CUTOFF
    views[ref] = _with_gray(views[ref], g)
    return Problem(views, ref, src, None, _photometric(), syn.depth_range(views, ref))


class Case(NamedTuple):
    make: object
    counters: dict          # census counter -> floor the oracle's solve must reach
    wave_families: bool = True     # False: another window than 11 x 11 -- only the generic family runs it


_TAPS = 121
CASES = {
    "flat_blocks": Case(_case_flat_blocks, dict(ncc_cut_ref_var=500, ncc_cut_src_var=500, tap_border=1000 * _TAPS)),
    "all_constant": Case(_case_all_constant, dict(ncc_cut_ref_var=10000, ncc_cut_src_var=500)),
    "one_constant_source": Case(_case_one_constant_source, dict(ncc_cut_src_var=1000)),
    "ring_360": Case(_case_ring_360, dict(corner_div_nonpos=10000, tap_outside=10000 * _TAPS, perturb_exhausted=5)),
    "wide_depth_range": Case(_case_wide_depth_range, dict(prob_sum_zero=100, cdf_nan=100, propagate_nonpos=20)),
    "collapsed_depth_range": Case(_case_collapsed_depth_range, dict(tap_border=1000 * _TAPS)),
    "smaller_than_window": Case(_case_smaller_than_window, dict(tap_border=300 * _TAPS, tap_outside=200 * _TAPS)),
    "narrower_than_column_group": Case(_case_narrower_than_column_group, dict(tap_border=300 * _TAPS)),
    "source_far_smaller": Case(_case_source_far_smaller, dict(tap_border=1000 * _TAPS, ncc_cut_src_var=1000)),
    "source_far_larger": Case(_case_source_far_larger, dict(tap_border=200 * _TAPS)),
    "geom_holes": Case(_case_geom_holes, dict(src_depth_zero=30000, src_depth_negative=4000,
                                              src_depth_nonfinite=10000)),
    "geom_holes_normals": Case(functools.partial(_case_geom_holes, normals=True),
                               dict(coord_nonfinite=1000 * _TAPS, ncc_src_var_nan=1000, corner_div_nonpos=4000,
                                    cdf_nan=300, propagate_nonfinite=50, perturb_exhausted=200)),
    "source_rotated_in_place": Case(_case_source_rotated_in_place,
                                    dict(coord_saturated=4000, coord_nonfinite=30000, ncc_src_var_nan=400,
                                         corner_div_nonpos=5000, cdf_nan=50)),
    "geom_scaled_normals": Case(_case_geom_scaled_normals, dict(prob_sum_zero=1000, cdf_nan_after_value=5)),
    "variance_at_cutoff": Case(_case_variance_at_cutoff, dict(ncc_ref_var_at_cut=3)),
    "flat_blocks_r2": Case(functools.partial(_case_flat_blocks, window_radius=2),
                           dict(ncc_cut_ref_var=2000, ncc_cut_src_var=1000), False),
    "flat_blocks_r8": Case(functools.partial(_case_flat_blocks, window_radius=8), dict(ncc_cut_src_var=400), False),
    "ring_360_r2": Case(functools.partial(_case_ring_360, window_radius=2),
                        dict(corner_div_nonpos=8000, ncc_cut_src_var=4000), False),
    "ring_360_r8": Case(functools.partial(_case_ring_360, window_radius=8),
                        dict(corner_div_nonpos=10000, tap_outside=1000000), False),
}


@functools.lru_cache(maxsize=None)
def build(name, small=False):
    return CASES[name].make(small)


# kernel family -> (development switch or None, its value, GetSweepKernelName() of the run)
FAMILIES = {
    "quad": (None, None, "pm_sweep_quad_kernel"),
    "explicit": ("COLMAP_AMD_PM_FP_GLOBAL", "1", "pm_sweep_quad_kernel (explicit indices)"),
    "pair": ("COLMAP_AMD_PM_HELP", "2", "pm_sweep_pair_kernel"),
    "generic": ("COLMAP_AMD_PM_WAVE", "0", "pm_sweep_kernel"),
    # max_sweeps = 0: the cost map is ComputeInitialCost's -- pm_initial_cost_wave_kernel under the default switches,
    # pm_initial_cost_kernel with the wave kernels switched off (pm_kernels.hip: plan.initial_cost; the handle has no
    # accessor for the initial-cost kernel, so the switch is what selects it) -- and no sweep kernel is reported
    "quad_initial": (None, None, ""),
    "generic_initial": ("COLMAP_AMD_PM_WAVE", "0", ""),
}


def case_family_pairs():
    """Every case through every kernel family that can run it."""
    return [(c, f) for c, case in CASES.items() for f in FAMILIES
            if case.wave_families or f.startswith("generic")]


# ---- the comparison, shared by tests/test_pm_gpu.py, test_pm_emul.py and test_pm_oracle.py ----

ALL_MAPS = ("depth", "normal", "cost", "sel_prob", "mask")
_REFERENCE = {}


def assert_same_bits(want, got, keys=ALL_MAPS):
    """Every value of every map as a 32-bit pattern (so -0.0 is not 0.0), no pixel skipped. NaNs must sit at the same
    positions; a NaN's payload and sign are not compared (IEEE 754 does not pin them down)."""
    for k in keys:
        a, b = np.ascontiguousarray(want[k]), np.ascontiguousarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            nan_a, nan_b = np.isnan(a), np.isnan(b)
            if not np.array_equal(nan_a, nan_b):
                bad = np.argwhere(nan_a != nan_b)
                raise AssertionError(f"{k}: NaN at {len(bad)} positions of one side only, first at {bad[0]}: "
                                     f"oracle {a[tuple(bad[0])]!r} hip {b[tuple(bad[0])]!r}")
            a = np.where(nan_a, np.uint32(0x7fc00000), a.view(np.uint32))
            b = np.where(nan_b, np.uint32(0x7fc00000), b.view(np.uint32))
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            i = tuple(bad[0])
            raise AssertionError(f"{k}: {len(bad)} of {a.size} values differ, first at {bad[0]}: "
                                 f"oracle {want[k][i]!r} ({int(a[i]):#x}) hip {got[k][i]!r} ({int(b[i]):#x})")


def paired_edge_options(pm_oracle, p, initial=False):
    from pm_common import paired_options
    kw = dict(p.options)
    if initial:    # no sweep: the cost map is ComputeInitialCost's
        kw.update(filter=0, max_sweeps=0)
    return paired_options(pm_oracle, depth_min=p.depth_range[0], depth_max=p.depth_range[1], **kw)


def reference(pm_oracle, name, small=False, initial=False):
    """The oracle's solve of a case in device order: computed once, shared by the families, never written to."""
    from pm_common import oracle_inputs
    key = (name, small, initial)
    if key not in _REFERENCE:
        p = build(name, small)
        o, _ = paired_edge_options(pm_oracle, p, initial)
        want = pm_oracle.run(o, oracle_inputs(p.views, p.maps is not None, p.maps), p.ref, p.src, want_cost=True)
        for v in want.values():
            v.setflags(write=False)
        _REFERENCE[key] = want
    return _REFERENCE[key]
