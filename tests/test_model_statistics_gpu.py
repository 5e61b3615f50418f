"""The model statistics on the GPU (include/colmap_amd_model.h, colmap_amd/csrc/model_stats.hip) against the sequential
checker, the methods of colmap_amd.workspace.Model. The case functions are run twice: here through the hipcc build on the
device, and by tests/test_model_statistics_emul.py through the CPU stand-in build of the same source.

Comparison rule
  exact (array_equal)   the CSR structure of the pair statistics (row_offsets, other), the shared counts, the overlap
                        lists for (K, min angle) in {(3, 0), (20, 1), (50, 0), (3, 89)} and the (-1, -1) depth ranges.
  angle threshold       an overlap list only means something away from the threshold: each overlap case first asserts,
                        on the checker's values, that every pair's 75th-percentile angle is at least 1 % away from the
                        min_rad in use. The generator provides that; nothing is excluded from the comparison.
  percentile angles     within 4 float ulps of the checker's value (4 * 2^-23 relative). Both sides form an angle in
                        double and narrow it to float, which can differ by one ulp where the double arithmetic differs by
                        1e-10; both interpolate in double and narrow once more; the bar is twice that. Preconditions,
                        asserted on the generator: every angle but the constructed zero is above 0.1 degrees, where acos
                        is well-conditioned; and the float projection centre -R^T T of every image is exact (R and T lie
                        on a grid of 2^-10), so that both sides start from the same centres -- a centre that is one float
                        ulp off, as another summation order gives, moves an angle by more than the bar. The worst
                        difference is printed.
  depth ranges          within 1e-6 relative: four float roundings on terms no larger than 1.6 x the depth (asserted on
                        the generated poses and points), 4 * 1.6 * 2^-24 = 3.8e-7, and one more for the stretch.
  reproducibility       every call is made twice and all outputs are byte-identical between the runs.
The checker's results are computed once per process and shared by both test modules.
"""
import ctypes as C

import numpy as np
import pytest

from colmap_amd import model_statistics as MS
from colmap_amd import workspace as W

NUM_GENERAL = 70
RADIUS = 5.0
SPECIAL = ["none", "away", "ident", "heavy_a", "heavy_b", "three", "c1", "c2", "c3", "c4", "c5", "c9", "c64", "c65",
           "c99", "c100", "c101", "c200"]
IDX = {name: NUM_GENERAL + k for k, name in enumerate(SPECIAL)}
NUM_IMAGES = NUM_GENERAL + len(SPECIAL)
COUNTS = [1, 2, 3, 4, 5, 9, 64, 65, 99, 100, 101, 200]
NUM_HEAVY, NUM_DUPLICATES = 1100, 60
OVERLAP_CASES = [(3, 0.0), (20, 1.0), (50, 0.0), (3, 89.0)]
PERCENTILES = [0.0, 50.0, 75.0, 100.0]
K_ = np.array([[100, 0, 50], [0, 100, 50], [0, 0, 1]], np.float32)


def _look_at_origin(center, away=False):
    c = np.asarray(center, np.float64)
    z = -c / np.linalg.norm(c)
    if away:
        z = -z
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    # R and T on a grid of 2^-10: every product and sum of -R^T T is then exact in float, so the projection centre is
    # the same float whatever order (or fused multiply-add) a BLAS, Eigen or the device sums it in. R is a rotation to
    # 5e-4 only, which no statistic asks about.
    R = np.round(np.stack([x, y, z]) * 1024.0) / 1024.0
    return R.astype(np.float32), (np.round(-R @ c * 1024.0) / 1024.0).astype(np.float32)


def _image(R, T):
    return W.ModelImage("", 100, 100, K_, np.asarray(R, np.float32).reshape(3, 3), np.asarray(T, np.float32).reshape(3))


def _point(xyz, track):
    x, y, z = (float(np.float32(v)) for v in xyz)  # the floats mvs::Model holds
    return W.ModelPoint(x, y, z, [int(i) for i in track])


def build_model(seed=11):
    rng = np.random.default_rng(seed)
    m = W.Model()
    n = NUM_IMAGES
    # A Fibonacci lattice on a cap of 30 degrees around the -z pole of the radius-5 sphere: centres at least 0.4 apart
    # and rays to two of them less than 87 degrees apart at any point of the unit ball, so that every percentile angle
    # stays clear of the 1 and 89 degree thresholds. heavy_b sits on the far side: the rays of the heavy pair are
    # obtuse, min(a, pi - a) takes its second argument.
    def lattice(i):
        zc = 1.0 - (1.0 - np.cos(np.deg2rad(30.0))) * (2.0 * i + 1.0) / n
        phi = i * np.pi * (3.0 - np.sqrt(5.0))
        return RADIUS * np.array([np.sqrt(1 - zc * zc) * np.cos(phi), np.sqrt(1 - zc * zc) * np.sin(phi), -zc])

    for i in range(n):
        c = lattice(i)
        if i == IDX["heavy_b"]:
            c = -lattice(IDX["heavy_a"]) + np.array([1.75, 0.0, 0.0])
            c *= RADIUS / np.linalg.norm(c)
        if i == IDX["ident"]:  # identity rotation, integer translation: centre (0, 0, -5) exactly, the pole of the cap
            m.images.append(_image(np.eye(3), [0, 0, 5]))
        else:
            m.images.append(_image(*_look_at_origin(c, away=(i == IDX["away"]))))

    def ball(count):
        v = rng.normal(size=(count, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v * rng.uniform(0.05, 1.0, (count, 1)) ** (1 / 3)

    def general_track(length):
        return rng.choice(NUM_GENERAL, length, replace=False)

    lengths = [0] * 5 + [1] * 300 + [2] * 60 + [3] * 40 + list(rng.integers(4, 16, 150)) + [16] * 10 + [17] * 10 + \
        [20, 33, 47, 63] + [64] * 5 + [65] * 3 + [66, 68, 70]
    for L, X in zip(lengths, ball(len(lengths))):
        m.points.append(_point(X, general_track(int(L))))
    m.points.append(_point(ball(1)[0], [3, 7, 3]))  # a repeated image: (3, 7) counted twice, (3, 3) never
    for k, X in enumerate(ball(30)):  # the image that looks away still shares points
        m.points.append(_point(X, list(general_track(4)) + [IDX["away"]]))
    # exactly on a projection centre: the zero-norm branch. Its depth is 0 in the one image and negative in the other.
    m.points.append(_point([0, 0, -5], [IDX["ident"], IDX["away"]]))
    for X in ball(10):
        m.points.append(_point(X, [IDX["ident"], 6]))
    heavy = ball(NUM_HEAVY)
    heavy[100:100 + NUM_DUPLICATES] = heavy[99]  # equal angle bits: ties inside the select
    for X in heavy:
        m.points.append(_point(X, [IDX["heavy_a"], IDX["heavy_b"]]))
    for k, X in enumerate(ball(3)):  # exactly three candidates in its row
        m.points.append(_point(X, [IDX["three"], 10 + k]))
    for k, cnt in enumerate(COUNTS):  # a cell of exactly cnt angles, an image of exactly cnt positive depths
        for X in ball(cnt):
            m.points.append(_point(X, [IDX[f"c{cnt}"], 20 + k]))
    order = rng.permutation(len(m.points))  # the classes are spread over the point order
    m.points = [m.points[i] for i in order]
    return m


_cache = {}


def model():
    if "model" not in _cache:
        _cache["model"] = build_model()
    return _cache["model"]


def flat():
    if "flat" not in _cache:
        _cache["flat"] = MS.flatten(model())
    return _cache["flat"]


def checker(what, *args):
    """workspace.Model, computed once per (method, arguments)."""
    key = (what,) + args
    if key not in _cache:
        _cache[key] = getattr(model(), what)(*args)
    return _cache[key]


def _as_csr(dicts, dtype):
    row_offsets = np.zeros(len(dicts) + 1, np.int64)
    other, values = [], []
    for i, d in enumerate(dicts):
        for o in sorted(d):
            other.append(o)
            values.append(d[o])
        row_offsets[i + 1] = len(other)
    return row_offsets, np.array(other, np.int32), np.array(values, dtype)


def _all_angles(m):
    """Every pair angle of the model, vectorised (a precondition on the generator, not the checker)."""
    centers = np.array([(-im.R.T @ im.T).astype(np.float64) for im in m.images])
    out = []
    for pt in m.points:
        tr = np.array(pt.track, int)
        if len(tr) < 2:
            continue
        i, j = np.tril_indices(len(tr), -1)
        keep = tr[i] != tr[j]
        v1 = np.array([pt.x, pt.y, pt.z]) - centers[tr[i][keep]]
        v2 = np.array([pt.x, pt.y, pt.z]) - centers[tr[j][keep]]
        n = np.sqrt((v1 * v1).sum(1) * (v2 * v2).sum(1))
        with np.errstate(invalid="ignore", divide="ignore"):
            a = np.arccos(np.clip((v1 * v2).sum(1) / n, -1, 1))
        a = np.where(n == 0, 0.0, a)
        out.append(np.minimum(a, np.pi - a))
    return np.concatenate(out)


def case_model_shape():
    m = model()
    f = flat()
    lengths = np.diff(f.track_offsets)
    for L in (0, 1, 2, 3, 16, 17, 64, 65):  # both sides of each lane-group edge (model_plan.h: 1 / 16 / 64 lanes)
        assert (lengths == L).any(), L
    per_class = [((lengths >= 2) & (lengths <= 16)).sum(), ((lengths > 16) & (lengths <= 64)).sum(), (lengths > 64).sum()]
    for count, width in zip(per_class, (1, 16, 64)):  # more points than one workgroup of 256 lanes holds, no multiple
        assert count > 256 // width and count % (256 // width) != 0, (count, width)
    assert any(len(p.track) == 3 and p.track[0] == p.track[2] != p.track[1] for p in m.points)
    shared = checker("ComputeSharedPoints")
    sizes = {c for d in shared for c in d.values()}
    assert set(COUNTS) <= sizes and max(sizes) > 1024                      # 64 | 65: the selection boundary
    assert shared[IDX["heavy_a"]][IDX["heavy_b"]] == NUM_HEAVY
    assert shared[3][7] >= 2 and 3 not in shared[3]
    assert shared[IDX["none"]] == {} and len(shared[IDX["away"]]) > 0
    assert len(shared[IDX["three"]]) == 3
    assert any(len(set(d.values())) < len(d) for d in shared)               # equal counts within a row
    assert max(len(d) for d in shared) > 50                                 # K = 50 smaller than the candidates
    # depths: the special images, and the bound the depth tolerance rests on
    positive = np.zeros(len(m.images), int)
    observed = np.zeros(len(m.images), int)
    for pt in m.points:
        X = np.array([pt.x, pt.y, pt.z], np.float64)
        for idx in pt.track:
            im = m.images[idx]
            terms = np.array([im.R[2, 0] * X[0], im.R[2, 1] * X[1], im.R[2, 2] * X[2], im.T[2]], np.float64)
            depth = terms.sum()
            observed[idx] += 1
            if depth > 0:
                positive[idx] += 1
                partial = np.abs(np.array([terms[0], terms[1], terms[0] + terms[1], terms[2], terms[:3].sum(), terms[3]]))
                assert partial.max() <= 1.6 * depth
                assert depth > 1e-3
            else:
                assert depth < -1e-3 or depth == 0.0                         # never within rounding of zero
    for cnt in (1, 99, 100, 101, 200):
        assert positive[IDX[f"c{cnt}"]] == cnt
    assert observed[IDX["none"]] == 0
    assert observed[IDX["away"]] > 0 and positive[IDX["away"]] == 0
    assert observed[IDX["heavy_a"]] > 1024
    assert checker("ComputeDepthRanges")[IDX["away"]] == (-1.0, -1.0)
    for im in m.images:  # the float projection centre is exact, whatever the order of the sum
        for k in range(3):
            p = [np.float64(im.R[j, k]) * np.float64(im.T[j]) for j in range(3)]
            for v in p + [p[0] + p[1], p[1] + p[2], p[0] + p[2], p[0] + p[1] + p[2]]:
                assert np.float64(np.float32(v)) == v
    # angles: exactly one zero (the point on the centre), everything else well above 0.1 degrees; >= 50 equal values
    angles = _all_angles(m)
    assert (angles == 0).sum() == 1 and np.sort(angles)[1] > np.deg2rad(0.1)
    assert checker("ComputeTriangulationAngles", 50.0)[IDX["ident"]][IDX["away"]] == 0.0
    a = np.array([v for d in checker("ComputeTriangulationAngles", 75.0) for v in d.values()])
    assert a.max() < np.deg2rad(87.0) and np.sort(a)[2] > np.deg2rad(2.0)  # but the zero, in both directions
    assert len(angles) < 200_000


def case_depth_ranges():
    got = MS.depth_ranges_flat(flat())
    again = MS.depth_ranges_flat(flat())
    assert got.tobytes() == again.tobytes()
    want = np.array(checker("ComputeDepthRanges"), np.float32)
    none = want[:, 0] == -1.0
    assert none.sum() >= 2 and np.array_equal(got[none], want[none])
    rel = np.abs(got[~none].astype(np.float64) - want[~none]) / want[~none]
    print(f"depth ranges: worst relative difference {rel.max():.3g}")
    assert np.array_equal(got[:, 0] == -1.0, none) and rel.max() <= 1e-6
    assert MS.compute_depth_ranges(model())[IDX["none"]] == (-1.0, -1.0)


def case_pair_statistics(percentile):
    got = MS.pair_statistics_flat(flat(), percentile)
    again = MS.pair_statistics_flat(flat(), percentile)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    row_offsets, other, count, angle = got
    want_rows, want_other, want_count = _as_csr(checker("ComputeSharedPoints"), np.int32)
    _, _, want_angle = _as_csr(checker("ComputeTriangulationAngles", percentile), np.float32)
    assert np.array_equal(row_offsets, want_rows) and np.array_equal(other, want_other)
    assert np.array_equal(count, want_count)
    diff = np.abs(angle.astype(np.float64) - want_angle.astype(np.float64))
    bar = 4 * 2.0 ** -23 * np.abs(want_angle.astype(np.float64))
    worst = (diff / np.maximum(np.abs(want_angle), 1e-30) / 2.0 ** -23).max()
    print(f"percentile {percentile}: worst angle difference {worst:.3g} ulp over {len(angle)} entries")
    assert (diff <= bar).all()
    # symmetric: both directions of a pair hold the same multiset
    lookup = {(i, int(o)): a for i in range(len(row_offsets) - 1)
              for o, a in zip(other[row_offsets[i]:row_offsets[i + 1]], angle[row_offsets[i]:row_offsets[i + 1]])}
    assert all(lookup[(b, a)].tobytes() == v.tobytes() for (a, b), v in lookup.items())
    if percentile == 75.0:  # the mirror returns the checker's structures
        assert MS.compute_shared_points(model()) == checker("ComputeSharedPoints")
        mirror = MS.compute_triangulation_angles(model(), 75.0)
        assert [sorted(d) for d in mirror] == [sorted(d) for d in checker("ComputeTriangulationAngles", 75.0)]
        assert all(isinstance(v, np.float32) for d in mirror for v in d.values())


def assert_threshold_margin(angles75, min_deg):
    min_rad = np.float32(np.deg2rad(min_deg))
    values = np.array([v for d in angles75 for v in d.values()], np.float64)
    assert (np.abs(values - min_rad) >= 0.01 * min_rad).all(), "a percentile angle lies within 1 % of the threshold"


def case_overlap(num_images, min_deg):
    assert_threshold_margin(checker("ComputeTriangulationAngles", 75.0), min_deg)
    got = MS.max_overlapping_images_flat(flat(), num_images, min_deg)
    again = MS.max_overlapping_images_flat(flat(), num_images, min_deg)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    want = checker("GetMaxOverlappingImages", num_images, min_deg)
    ptr, idx = got
    lists = [[int(j) for j in idx[ptr[i]:ptr[i + 1]]] for i in range(len(ptr) - 1)]
    assert lists == want
    assert MS.get_max_overlapping_images(model(), num_images, min_deg) == want
    # the query form: nulls give the total alone
    b, total = MS._Bound(flat()), C.c_size_t()
    assert MS.lib().model_get_max_overlapping_images(C.byref(b.struct), C.c_int64(num_images), C.c_double(min_deg), None,
                                                     None, C.byref(total), C.c_int32(0)) == 0
    assert total.value == len(idx)
    if (num_images, min_deg) == (3, 0.0):
        assert len(want[IDX["three"]]) == 3 and len(want[IDX["c1"]]) == 1 and len(want[0]) == 3
        shared = checker("ComputeSharedPoints")
        assert any(shared[i][a] == shared[i][b] and a < b for i, l in enumerate(want) for a, b in zip(l, l[1:]))  # a tie, by index
    if min_deg == 89.0:
        assert sum(len(l) for l in want) < sum(len(d) for d in checker("ComputeSharedPoints"))


def _small(images, points):
    m = W.Model()
    for T in images:
        m.images.append(_image(np.eye(3), T))
    for xyz, track in points:
        m.points.append(_point(xyz, track))
    return m


def case_reference_expectations():
    """mvs/model_test.cc:82-190, rebuilt as data."""
    m = _small([[0, 0, 0], [-1, 0, 0], [-2, 0, 0]], [((5, 0, 10), [0, 1]), ((6, 0, 10), [0, 1, 2])])
    shared = MS.compute_shared_points(m)
    assert len(shared) == 3 and shared[0][1] == 2 and shared[1][0] == 2
    assert shared[0][2] == 1 and shared[2][0] == 1 and shared[1][2] == 1 and shared[2][1] == 1
    m = _small([[0, 0, 0]], [((0, 0, float(i)), [0]) for i in range(1, 101)])
    assert MS.compute_depth_ranges(m) == [(1.5, 125.0)]
    assert MS.compute_depth_ranges(_small([[0, 0, 0]], [])) == [(-1.0, -1.0)]
    m = _small([[0, 0, 0], [-1, 0, 0]], [((0.5, 0, 10), [0, 1])])
    angles = MS.compute_triangulation_angles(m, 50.0)
    assert len(angles) == 2 and abs(angles[0][1] - 2.0 * np.arctan(0.5 / 10.0)) <= 1e-5
    assert angles[0][1].tobytes() == angles[1][0].tobytes()
    m = _small([[0, 0, 0], [-1, 0, 0], [-2, 0, 0]],
               [((0.5, 0, 5.0 + i), [0, 1]) for i in range(10)] + [((1, 0, 10), [0, 2])])
    over = MS.get_max_overlapping_images(m, 2, 0.0)
    assert len(over) == 3 and over[0][0] == 1 and over == m.GetMaxOverlappingImages(2, 0.0)


def case_empty_models():
    empty = W.Model()
    assert MS.compute_depth_ranges(empty) == [] and MS.compute_shared_points(empty) == []
    assert MS.compute_triangulation_angles(empty, 75.0) == [] and MS.get_max_overlapping_images(empty, 5, 0.0) == []
    one = _small([[0, 0, 0]], [((0, 0, 2), [0]), ((0, 0, 3), [0, 0])])  # (a, a) is no pair
    assert MS.compute_shared_points(one) == [{}] and MS.get_max_overlapping_images(one, 5, 0.0) == [[]]
    assert MS.compute_depth_ranges(one) == one.ComputeDepthRanges()
    bare = _small([[0, 0, 0], [-1, 0, 0], [0, 1, 0]], [])
    assert MS.compute_depth_ranges(bare) == [(-1.0, -1.0)] * 3
    assert MS.compute_shared_points(bare) == [{}, {}, {}] and MS.compute_triangulation_angles(bare, 50.0) == [{}, {}, {}]
    assert MS.get_max_overlapping_images(bare, 2, 0.0) == [[], [], []]


def case_input_validation():
    """Every rejected input raises before anything is launched."""
    good = MS.flatten(_small([[0, 0, 0], [-1, 0, 0]], [((0.5, 0, 10), [0, 1]), ((0.5, 0, 9), [1, 0])]))

    def changed(**kw):
        f = MS.FlatModel(good.R, good.T, good.points, good.track_offsets.copy(), good.track_image.copy())
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def every_entry(f, match):
        for call in (lambda: MS.depth_ranges_flat(f), lambda: MS.pair_statistics_flat(f, 75.0),
                     lambda: MS.max_overlapping_images_flat(f, 2, 0.0)):
            with pytest.raises(MS.ModelStatisticsError, match=match):
                call()

    every_entry(changed(track_offsets=np.array([1, 2, 4], np.int64)), "Check failed: track_offsets must start at 0")
    every_entry(changed(track_offsets=np.array([0, 3, 2], np.int64)), "Check failed: track_offsets decreases at point 1")
    every_entry(changed(track_offsets=np.array([0, 2, 3], np.int64)), "Check failed: track_offsets must end at num_observations")
    every_entry(changed(track_image=np.array([0, 1, 2, 0], np.int32)), "Check failed: observation 2: image index 2 out of range")
    every_entry(changed(track_image=np.array([0, -1, 1, 0], np.int32)), "Check failed: observation 1: image index -1 out of range")
    for p in (-0.5, 100.5, float("nan")):
        with pytest.raises(MS.ModelStatisticsError, match="Check failed: percentile must lie in \\[0, 100\\]"):
            MS.pair_statistics_flat(good, p)
    with pytest.raises(MS.ModelStatisticsError, match="Check failed: num_images_wanted must not be negative"):
        MS.max_overlapping_images_flat(good, -1, 0.0)
    for call in (lambda: MS.depth_ranges_flat(good, gpu_index=1 << 20), lambda: MS.pair_statistics_flat(good, 75.0, -1),
                 lambda: MS.max_overlapping_images_flat(good, 2, 0.0, gpu_index=1 << 20)):
        with pytest.raises(MS.ModelStatisticsError, match="gpu_index -?\\d+ out of range"):
            call()
    n = 8193  # one image over the limit of the dense pair table
    many = MS.FlatModel(np.tile(np.eye(3, dtype=np.float32).ravel(), (n, 1)), np.zeros((n, 3), np.float32),
                        np.zeros((0, 3), np.float32), np.zeros(1, np.int64), np.zeros(0, np.int32))
    every_entry(many, "Check failed: num_images 8193 exceeds the limit of the dense pair table, 8192 images")
    assert MS.pair_statistics_flat(good, 75.0)[2].tolist() == [2, 2]  # and the good model goes through


def case_patch_match_config():
    """read_patch_match_config(..., model_statistics=device) equals the Python route on the `__auto__` lines, on the
    model shape of tests/test_workspace.py."""
    import test_workspace as TW
    m = W.Model.FromSparseModel(TW._sparse_model(5, 80, seed=1), "")
    cfg = ["img00.png", "__all__", "img01.png", "img00.png, img02.png ,img04.png", "img02.png", "__auto__, 2",
           "img03.png", "__auto__, 50", "img04.png", "__auto__, 2"]
    device = MS.DeviceStatistics(0)
    for min_deg in (0.0, 1.0):
        assert_threshold_margin(m.ComputeTriangulationAngles(75.0), min_deg)
        want = W.read_patch_match_config(cfg, m, min_triangulation_angle=min_deg)
        assert W.read_patch_match_config(cfg, m, min_triangulation_angle=min_deg, model_statistics=device) == want
        assert len(want) == 5
    warned = []
    assert W.read_patch_match_config(["img02.png", "__auto__, 2"], m, min_triangulation_angle=80.0, warn=warned.append,
                                     model_statistics=device) == [] and "img02.png" in warned[0]
    got, want = device.compute_depth_ranges(m), m.ComputeDepthRanges()
    assert np.allclose(np.array(got), np.array(want), rtol=1e-6, atol=0)


def case_from_workspace(tmp_path):
    """PatchMatchController.FromWorkspace: the device route gives the problems and depth ranges of the Python route."""
    import os
    from PIL import Image as PILImage
    import test_workspace as TW
    from colmap_amd import mvs
    ws = tmp_path / "dense"
    sm = TW._sparse_model(4, 60, seed=3, w=40, h=30)
    W.write_model_binary(sm, str(ws / "sparse"))
    os.makedirs(ws / "images"); os.makedirs(ws / "stereo")
    for im in sm.images.values():
        PILImage.fromarray(np.zeros((30, 40, 3), np.uint8)).save(ws / "images" / im.name)
    W.write_patch_match_config(str(ws / "stereo" / "patch-match.cfg"), [im.name for im in sm.images.values()])
    options = mvs.PatchMatchOptions(gpu_index="0", min_triangulation_angle=0.0)
    want = mvs.PatchMatchController.FromWorkspace(options, str(ws))
    got = mvs.PatchMatchController.FromWorkspace(options, str(ws), model_statistics=MS.DeviceStatistics(0))
    assert got.problems_ == want.problems_ and len(got.problems_) == 4
    for a, b in zip(got.images_, want.images_):
        assert np.allclose(a.depth_range, b.depth_range, rtol=1e-6, atol=0)


pytestmark = pytest.mark.gpu


def test_generated_model_has_the_shapes():
    case_model_shape()


def test_depth_ranges_match_checker():
    case_depth_ranges()


@pytest.mark.parametrize("percentile", PERCENTILES)
def test_pair_statistics_match_checker(percentile):
    case_pair_statistics(percentile)


@pytest.mark.parametrize("num_images,min_deg", OVERLAP_CASES)
def test_overlap_lists_match_checker(num_images, min_deg):
    case_overlap(num_images, min_deg)


def test_expectations_of_the_reference():
    case_reference_expectations()


def test_empty_models():
    case_empty_models()


def test_input_validation():
    case_input_validation()


def test_patch_match_config_auto_lines():
    case_patch_match_config()


def test_from_workspace_device_route(tmp_path):
    case_from_workspace(tmp_path)
