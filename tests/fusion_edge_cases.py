"""Degenerate depth-map fusion problems: the inputs the depth gates, the rounding of a projected coordinate, the three
bars at exact equality, the bounding-box faces, the median at a tie, the bitmap lookup and the limits of a walk exist
for, which the rendered, smooth maps of pm_common.scene() almost never reach. Every case is a VALID problem the C ABI
accepts, tiny (at most 32 x 24 pixels per image), shared by the checker tests, the CPU stand-in and the GPU
(tests/test_fusion.py, tests/test_fusion_emul.py); tests/fusion_edge_cases.md has what each one reaches.

The exact-arithmetic cases are built from powers of two (`_plane`): R = I, focal length 64, principal point at the
image centre, constant depth 4, translations that are multiples of 2^-6. A pixel (c, r) of such an image is the point
((c - cx) / 16 - Tx, (r - cy) / 16 - Ty, 4), and it projects into another such image at (c + 16 dTx, r + 16 dTy): every
product, quotient and difference on the way is exact in float, so which side of a comparison a pixel falls on is a
property of the input and not of anybody's rounding.

No case holds a non-finite depth or normal: the reference has no defined result for them (it casts a NaN coordinate
to int, runs nth_element over NaN, and an infinite depth becomes NaN in the un-projection).

A case names the census counters (oracle/fusion_oracle.cpp: FUO_CENSUS) it exists for, each with a floor: a condition
the checker's mode-1 solve of the case must meet for the case to mean anything, not a measurement.

    build(name) -> (StereoFusionOptions, [FusionImage], overlap lists)
"""
import functools
from typing import NamedTuple

import numpy as np

from colmap_amd import fusion
from pm_common import scene

f32 = np.float32
_ULP_4_5 = float(np.spacing(f32(4.5)))


def _overlap(n):
    return [[j for j in range(n) if j != i] for i in range(n)]


def _scene_images(views):
    out = []
    for v in views:
        h, w = v.gray.shape
        rgb = np.stack([v.gray, 255 - v.gray, (v.gray // 2)], -1)
        out.append(fusion.FusionImage(w, h, v.K, v.R, v.T, rgb, v.depth.copy(), v.normal.copy()))
    return out


def _plane(w=32, h=24, tx=0.0, ty=0.0, depth=4.0, normal=(0.0, 0.0, -1.0), grey=100):
    """One image of the exact set-up: fronto-parallel plane at `depth`, camera shifted by (tx, ty)."""
    K = np.array([[64, 0, w // 2], [0, 64, h // 2], [0, 0, 1]], f32)
    d = np.full((h, w), depth, f32)
    n = np.empty((3, h, w), f32)
    n[:] = np.asarray(normal, f32)[:, None, None]
    rgb = np.full((h, w, 3), grey, np.uint8)
    return fusion.FusionImage(w, h, K, np.eye(3, dtype=f32), np.array([tx, ty, 0], f32), rgb, d, n)


def _opt(**kw):
    return fusion.StereoFusionOptions(**kw)


# ---- the cases -------------------------------------------------------------------------------------------------------

def _case_depth_signs():
    """About 5 % of the pixels each: 0, -0.0, a negative value, a positive subnormal (> 0: walked; a device that flushed
    it would drop the pixel), a tiny normal and a large finite value."""
    images = _scene_images(scene(4, 32, 24))
    rng = np.random.default_rng(7)
    for im in images:
        pick = rng.random(im.depth_map.shape)
        for k, v in enumerate((0.0, -0.0, -3.5, 1e-40, 1e-30, 1e30)):
            im.depth_map[(pick >= 0.05 * k) & (pick < 0.05 * (k + 1))] = f32(v)
    return _opt(min_num_pixels=1, max_reproj_error=1.5, max_depth_error=0.02), images, _overlap(4)


def _case_behind_camera():
    """Two of four ring cameras turned about their own vertical axis to look outward (same centres): the points the other
    two absorb lie behind them and project with a non-positive third component, to negative and to mirrored in-image
    coordinates; the mirrored ones are read and fail the depth test, as in the reference."""
    views = scene(4, 32, 24)
    images = _scene_images(views)
    flip = np.diag([-1.0, 1.0, -1.0]).astype(f32)
    for i in (1, 3):
        images[i].R = flip @ np.asarray(images[i].R, f32)
        images[i].T = flip @ np.asarray(images[i].T, f32)
    return _opt(min_num_pixels=1), images, _overlap(4)


def _case_projection_pole():
    """Two cameras at the same centre at a right angle (exact rotation): the points of image 0's column cx have third
    component exactly 0 in image 1, so the projected coordinates are +-inf and, with Tx = 4, 0 / 0 = NaN; the columns to
    its left lie behind image 1. All rejected by the float-side range test."""
    a = _plane()
    b = _plane()
    b.R = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], f32)
    b.T = np.array([4, 0, 0], f32)
    c = _plane()
    c.R = b.R.copy()
    c.T = np.array([2, 0.25, 0], f32)
    return _opt(min_num_pixels=1), [a, b, c], _overlap(3)


def _case_rounding_ties():
    """Shifts of exactly k + 0.5 pixels in both signs (ties round away from zero: 2.5 -> 3, -0.5 -> -1, -1.5 -> -2), of
    -0.25 (column 0 lands on -0.25 -> -0.0 -> pixel 0) and coordinates of exactly width - 0.5 (round to width: out)."""
    s = 1.0 / 16.0
    images = [_plane(), _plane(tx=2.5 * s, ty=-1.5 * s, grey=110), _plane(tx=-0.5 * s, ty=0.5 * s, grey=121),
              _plane(tx=-0.25 * s, ty=-0.25 * s, grey=132)]
    return _opt(min_num_pixels=1), images, _overlap(4)


def _bars(max_normal_error, normals):
    """Image 0 (fused first) against image 1 in the same pose at depth 4: columns 0-7 at depth 4.5 (depth error exactly
    0.125 = the bar: kept), 8-11 one ulp above (rejected), 12-15 one ulp below (kept). Columns 16-31 at depth 4 against
    image 2, shifted by half a pixel: the tie rounds to the next column and leaves a residual of exactly 0.5 px, squared
    0.25 = the bar: kept."""
    a = _plane(normal=normals[0])
    a.depth_map[:, 0:8] = 4.5
    a.depth_map[:, 8:12] = 4.5 + _ULP_4_5
    a.depth_map[:, 12:16] = 4.5 - _ULP_4_5
    b = _plane(normal=normals[1], grey=111)
    b.depth_map[:, 16:] = 0.0       # the right half belongs to image 2
    c = _plane(tx=1.0 / 32.0, normal=normals[2], grey=122)
    c.depth_map[:, :17] = 0.0
    opt = _opt(min_num_pixels=1, max_depth_error=0.125, max_reproj_error=0.5, max_normal_error=max_normal_error)
    return opt, [a, b, c], _overlap(3)


def _case_bars_at_equality():
    """max_normal_error = 0 with identical axis normals: cosine 1 meets the bar 1."""
    return _bars(0.0, [(0, 0, -1)] * 3)


def _case_bars_at_equality_perpendicular():
    """max_normal_error = 90 with perpendicular axis normals: the bar is float(cos(pi / 2)) = 6.1e-17, not 0, so a cosine
    of exactly 0 is rejected -- by the library as by the reference."""
    return _bars(90.0, [(0, 0, -1), (0, -1, 0), (-1, 0, 0)])


def _case_normals_degenerate():
    """Three images in one pose, max_normal_error = 180 (bar -1). Row bands: zero normals (median 0: dropped); normals
    (0, 0, -1) against (0, 0, 1) in two images only (median 0: dropped); scaled by 1e-20 (squared norm subnormal, norm
    1e-20 < FLT_EPSILON: dropped), by 1e-23 (squared norm underflows to 0), by 1e18 (finite: kept); of length exactly
    FLT_EPSILON (not below: kept)."""
    images = [_plane(), _plane(grey=111), _plane(grey=122)]
    for k, im in enumerate(images):
        n = im.normal_map
        n[:, 0:4] = 0.0
        if k == 1:
            n[2, 4:8] = 1.0
        if k == 2:
            im.depth_map[4:8] = 0.0
        n[:, 8:12] *= f32(1e-20)
        n[:, 12:14] *= f32(1e-23)
        n[:, 14:18] *= f32(1e18)
        n[:, 18:22] *= f32(2.0 ** -23)
    return _opt(min_num_pixels=1, max_normal_error=180.0), images, _overlap(3)


def _case_median_shapes():
    """min_num_pixels = 1; four images in one pose (so every coordinate of a support ties) plus one unused. Masks leave
    supports of 4, 3, 2 and 1 pixels in the four column bands; the lower rows carry depths 4 (1 + k 2^-9) so that medians
    there interpolate between distinct values; column cx and row cy are zeros of x and y, the normals of two images are
    (-0.0, -0.0, -1) so zeros of both signs meet in a median; grey values 10, 13, 20, 31: an even support's colour median
    ends in .5."""
    images = []
    for k, g in enumerate((10, 13, 20, 31)):
        im = _plane(grey=g, normal=(-0.0, -0.0, -1.0) if k % 2 else (0.0, 0.0, -1.0))
        im.depth_map[12:] = f32(4.0 * (1.0 + k * 2.0 ** -9))
        m = np.zeros((24, 32), np.uint8)
        if k >= 1:
            m[:, 24:] = 1
        if k >= 2:
            m[:, 16:24] = 1
        if k >= 3:
            m[:, 8:16] = 1
        im.mask = m
        images.append(im)
    images.append(fusion.FusionImage(32, 24, images[0].K, images[0].R, images[0].T, None, None, None, used=False))
    return _opt(min_num_pixels=1), images, _overlap(5)


def _case_bitmap_scale():
    """Model images 33 x 25 with depth maps 16 x 12: the bitmap lookup is round(col / (16 / 33)). Image 0 has a full
    bitmap; image 1 one of 31 x 23, so the last column and row land on exactly its width and height (outside); image 2
    one of 20 x 15."""
    views = scene(4, 16, 12)
    rng = np.random.default_rng(5)
    images = []
    for k, v in enumerate(views):
        K = np.asarray(v.K, f32).copy()
        K[0] *= f32(33.0 / 16.0)
        K[1] *= f32(25.0 / 12.0)
        bw, bh = [(33, 25), (31, 23), (20, 15), (33, 25)][k]
        rgb = rng.integers(0, 256, size=(bh, bw, 3), dtype=np.uint8)
        images.append(fusion.FusionImage(33, 25, K, v.R, v.T, rgb, v.depth.copy(), v.normal.copy()))
    return _opt(min_num_pixels=1, max_reproj_error=3.0, max_depth_error=0.05, max_normal_error=30.0), images, _overlap(4)


def _case_ragged_sizes():
    """One run over images of 1 x 1, 1 x 23, 23 x 1 and 8 x 9, 8 x 10, 8 x 11 (one stripe, exactly one, one and a tenth),
    a lone image with an empty overlap list that nobody lists, and a pair of which one image is unused."""
    sizes = [(1, 1), (1, 23), (23, 1), (8, 9), (8, 10), (8, 11)]
    images = [_plane(w, h, grey=100 + 7 * k) for k, (w, h) in enumerate(sizes)]
    images.append(_plane(5, 4, grey=200))
    images.append(_plane(6, 12, grey=210))
    images.append(fusion.FusionImage(6, 12, images[-1].K, images[-1].R, images[-1].T, None, None, None, used=False))
    overlap = [[j for j in range(6) if j != i] for i in range(6)] + [[], [8], [7]]
    return _opt(min_num_pixels=1), images, overlap


def _case_box_faces():
    """Bounding box [-0.5, 0.5] x [-0.5, 0.25] x [4, 4]: its faces lie exactly on the points of columns 8 and 24, rows 4
    and 16 and on the plane itself (equal is inside). Seeds left, right, above and below are outside; image 1 is shifted
    by half a pixel, so the neighbour of a seed on the right face is 1 / 32 beyond it."""
    images = [_plane(), _plane(tx=1.0 / 32.0, grey=111), _plane(ty=-2.0 / 16.0, grey=122)]
    opt = _opt(min_num_pixels=1, bounding_box=((-0.5, -0.5, 4.0), (0.5, 0.25, 4.0)))
    return opt, images, _overlap(3)


def _chain(mask_period):
    """Four images in one pose on a chain overlap 0 -> 1 -> 2 -> 3: a walk from image 0 takes one pixel per image, one
    level each. Image 1 is masked on every `mask_period`-th column: walks from there end with a support of 1."""
    images = [_plane(grey=100 + 10 * k) for k in range(4)]
    m = np.zeros((24, 32), np.uint8)
    m[:, ::mask_period] = 1
    images[1].mask = m
    return images, [[1], [2], [3], []]


def _case_limits_exact(min_num_pixels, max_num_pixels, max_traversal_depth):
    images, overlap = _chain(5)
    return _opt(min_num_pixels=min_num_pixels, max_num_pixels=max_num_pixels,
                max_traversal_depth=max_traversal_depth), images, overlap


class Case(NamedTuple):
    make: object
    counters: dict          # census counter -> floor the checker's mode-1 solve must reach


# floors: at most a quarter of the count measured when the case was written (tests/fusion_edge_cases.md), at least 1
CASES = {
    "depth_signs": Case(_case_depth_signs, dict(seed_depth_nonpos=100, nb_depth_nonpos=20, depth_subnormal=20)),
    "behind_camera": Case(_case_behind_camera, dict(proj_z_nonpos=300)),
    "projection_pole": Case(_case_projection_pole, dict(coord_nonfinite=10, proj_z_nonpos=100)),
    "rounding_ties": Case(_case_rounding_ties, dict(coord_tie=500, coord_neg_zero=20, coord_far_edge=20)),
    "bars_at_equality": Case(_case_bars_at_equality, dict(depth_err_at_bar=40, reproj_at_bar=80, cos_at_bar=100)),
    "bars_at_equality_perpendicular": Case(_case_bars_at_equality_perpendicular, dict(cos_zero_below_bar=50)),
    "normals_degenerate": Case(_case_normals_degenerate, dict(normal_too_short=100, normal_at_epsilon=20)),
    "median_shapes": Case(_case_median_shapes, dict(support_1=40, support_2=40, support_even=80, support_odd=80,
                                                    median_tie=100, colour_tie=80)),
    "bitmap_scale": Case(_case_bitmap_scale, dict(colour_outside=35)),
    "ragged_sizes": Case(_case_ragged_sizes, dict(support_1=10)),
    "box_faces": Case(_case_box_faces, dict(seed_out_of_box=100, nb_out_of_box=3, on_box_face=100)),
    # walks that reach max_num_pixels exactly, with values 2 and 3; supports that equal min_num_pixels exactly;
    # max_traversal_depth of 2 and 3 on the chain
    "limits_exact_cap2": Case(functools.partial(_case_limits_exact, 2, 2, 3), dict(cap_reached=100, below_min_pixels=30)),
    "limits_exact_cap3": Case(functools.partial(_case_limits_exact, 3, 3, 100), dict(cap_reached=100, below_min_pixels=30)),
    "limits_exact_depth2": Case(functools.partial(_case_limits_exact, 2, 100, 2), dict(level_bound=100, below_min_pixels=30)),
    "limits_exact_depth3": Case(functools.partial(_case_limits_exact, 3, 100, 3), dict(level_bound=100, below_min_pixels=30)),
}


@functools.lru_cache(maxsize=None)
def _built(name):
    opt, images, overlap = CASES[name].make()
    for im in images:       # shared by every test of the case: never written to
        for a in (im.depth_map, im.normal_map, im.rgb, im.mask):
            if a is not None:
                a.setflags(write=False)
    return opt, images, overlap


def build(name, **option_overrides):
    """(options, images, overlap) of a case; the images are shared and read-only."""
    import dataclasses
    opt, images, overlap = _built(name)
    return dataclasses.replace(opt, **option_overrides), images, overlap


# ---- the comparison --------------------------------------------------------------------------------------------------

_REFERENCE = {}


def reference(fusion_oracle, name, mode=1, **option_overrides):
    """The checker's solve of a case: computed once, shared by the tests that need it, never written to. No NaN in it
    (asserted here), so an array comparison against it is a bit comparison up to the sign of a zero."""
    key = (name, mode, tuple(sorted(option_overrides.items())))
    if key not in _REFERENCE:
        want = fusion_oracle.fuse(*build(name, **option_overrides), mode=mode)
        assert not np.isnan(want.xyz).any() and not np.isnan(want.normal).any(), name
        for a in (want.xyz, want.normal, want.rgb):
            a.setflags(write=False)
        _REFERENCE[key] = want
    return _REFERENCE[key]


def assert_same(want, got, what=""):
    """Points, normals, colours and visibility lists, value for value (no NaN on the `want` side: equal values are equal
    bit patterns except that -0.0 equals 0.0 -- which of several equal zeros a median returns is not defined by the
    reference's nth_element either)."""
    assert len(got.xyz) == len(want.xyz), (what, len(got.xyz), len(want.xyz))
    for k in ("xyz", "normal", "rgb"):
        a, b = getattr(want, k), getattr(got, k)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what} {k}: {len(bad)} of {a.size} values differ, first at {bad[0]}: "
                                 f"want {a[tuple(bad[0])]!r} got {b[tuple(bad[0])]!r}")
    assert len(want.visibility) == len(got.visibility), what
    for i, (u, v) in enumerate(zip(want.visibility, got.visibility)):
        assert np.array_equal(u, v), (what, "visibility of point", i, list(u), list(v))
