"""Two-view geometry estimation on the GPU (colmap_amd/csrc/two_view.hip behind colmap_amd/two_view_geometry.py) against
the numpy checker tests/two_view_reference.py: exact scores, batch independence, the minimal solvers against a
50-digit solve, the sample draw, the properties of the search, unambiguous scenes and the command. The case functions
are shared with tests/test_two_view_geometry_emul.py, which runs them through the CPU build of the unmodified source."""
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import two_view_reference as R
from colmap_amd import database as DB
from colmap_amd import two_view_geometry as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1000, 800
K = np.array([[800.0, 0, 500.0], [0, 800.0, 400.0], [0, 0, 1]])
MAX_ERROR = 4.0
PINHOLE = TV.CameraInfo(1, W, H, 1)    # PINHOLE
PINHOLE2 = TV.CameraInfo(1, W, H, 2)
FISHEYE = TV.CameraInfo(5, W, H, 3)    # OPENCV_FISHEYE


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


R2 = _rot([0.1, 1.0, 0.05], 0.15)
T2 = np.array([1.0, 0.1, 0.2])


def _project(X, Rm, t):
    x = (K @ (Rm @ X.T + t[:, None])).T
    return x[:, :2] / x[:, 2:]


def _cross(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def scene(kind, n_in, n_out, seed, Rm=R2, t=T2):
    """(pts [n][4], truth mask): exact inliers of a two-camera set-up followed by gross outliers, then shuffled.
    kind: `general` (points in a box), `plane` (points on a plane), `rotation` (t = 0). An outlier's second point lies
    60 to 200 px from the true epipolar line (general) or from the true transfer (plane, rotation): more than 10 x
    MAX_ERROR by construction."""
    rng = np.random.default_rng(seed)
    if kind == "rotation":
        t = np.zeros(3)
    n = n_in + n_out
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.6, 1.6, n), rng.uniform(4, 8, n)], 1)
    if kind == "plane":
        X[:, 2] = 6.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    p1, p2 = _project(X, np.eye(3), np.zeros(3)), _project(X, Rm, t)
    d = rng.uniform(60, 200, n_out) * rng.choice([-1.0, 1.0], n_out)
    if kind == "general":
        F = np.linalg.inv(K).T @ _cross(t) @ Rm @ np.linalg.inv(K)
        l = (F @ np.hstack([p1[n_in:], np.ones((n_out, 1))]).T).T
        normal = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
    else:
        ang = rng.uniform(0, 2 * np.pi, n_out)
        normal = np.stack([np.cos(ang), np.sin(ang)], 1)
    p2[n_in:] += d[:, None] * normal
    pts = np.hstack([p1, p2])
    truth = np.concatenate([np.ones(n_in, np.uint8), np.zeros(n_out, np.uint8)])
    order = rng.permutation(n)
    return np.ascontiguousarray(pts[order]), truth[order]


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _ransac(**kw):
    return TV.RANSACOptions(random_seed=3, **kw)


def _ref_ransac(o: TV.RANSACOptions):
    return R.ransac_options(max_error=o.max_error, min_inlier_ratio=o.min_inlier_ratio, confidence=o.confidence,
                            dyn_num_trials_multiplier=o.dyn_num_trials_multiplier, min_num_trials=o.min_num_trials,
                            max_num_trials=o.max_num_trials, random_seed=o.random_seed)


# ---- 1. scores are exact -----------------------------------------------------------------------------------------------

def edge_sets():
    L = TV.match_tile()
    sizes = [7, 8, 63, 64, 65, L - 1, 0, L + 1, 2 * L + 3]
    return [scene("general" if i % 2 == 0 else "plane", n - n // 3, n // 3, 100 + i)[0] for i, n in enumerate(sizes)]


def edge_models(kind, sets, rng):
    """(model_set, models): per set a random model, a model that fits the set, the zero matrix, and for H a matrix with
    a zero third row."""
    model_set, models = [], []
    for s, pts in enumerate(sets):
        mine = [rng.normal(size=9)]
        if len(pts) >= R.MIN_SAMPLES[kind]:
            fit = R.solve_minimal(kind, pts[:R.MIN_SAMPLES[kind]])
            mine += [m for m in fit[:1]]
        mine.append(np.zeros(9))
        if kind == R.KIND_H:
            mine.append(np.array([1.0, 0, 3, 0, 1, -2, 0, 0, 0]))
        model_set += [s] * len(mine)
        models += mine
    return np.array(model_set, np.int32), np.array(models)


def case_scores_exact(kind):
    sets = edge_sets()
    model_set, models = edge_models(kind, sets, np.random.default_rng(7 + kind))
    with TV.PointSets() as ps:
        ps.set_points(sets, list(range(len(sets))))
        n, s, masks = ps.score(kind, MAX_ERROR, model_set, models, masks=True)
        n2, s2 = ps.score(kind, MAX_ERROR, model_set, models)
    assert (n == n2).all() and (_bits(s) == _bits(s2)).all()
    some_inliers = False
    for m in range(len(models)):
        want = R.support(kind, models[m], sets[model_set[m]], MAX_ERROR)
        assert n[m] == want[0], (m, n[m], want[0])
        assert (masks[m] == want[2]).all(), m
        assert _bits(s[m]) == _bits(want[1]), (m, s[m], want[1])
        some_inliers |= 0 < want[0]
    assert some_inliers


# ---- 2. batch independence -----------------------------------------------------------------------------------------------

def case_batch_independence(kind):
    M = TV.model_tile()
    rng = np.random.default_rng(11)
    pts, _ = scene("general", 90, 40, 5)
    other, _ = scene("plane", 50, 20, 6)
    target = R.solve_minimal(kind, pts[:R.MIN_SAMPLES[kind]])[0]
    want = R.support(kind, target, pts, MAX_ERROR)
    with TV.PointSets() as ps:
        ps.set_points([pts], [1])
        alone = ps.score(kind, MAX_ERROR, [0], target[None], masks=True)
        assert alone[0][0] == want[0] and _bits(alone[1][0]) == _bits(want[1]) and (alone[2][0] == want[2]).all()
        # every position of a tile, and the first position of the next one
        n, s = ps.score(kind, MAX_ERROR, [0] * (M + 1), np.tile(target, (M + 1, 1)))
        assert (n == want[0]).all() and (_bits(s) == _bits(want[1])).all()
        for others in (M - 1, M, M + 1):
            models = rng.normal(size=(others + 1, 9))
            pos = int(rng.integers(0, others + 1))
            models[pos] = target
            n, s = ps.score(kind, MAX_ERROR, [0] * (others + 1), models)
            assert n[pos] == want[0] and _bits(s[pos]) == _bits(want[1]), others
        # the set among others, and models of several sets in one launch
        ps.set_points([other, pts, other[:9]], [5, 1, 9])
        n, s, masks = ps.score(kind, MAX_ERROR, [0, 1, 2, 1], np.stack([target] * 4), masks=True)
        for m in (1, 3):
            assert n[m] == want[0] and _bits(s[m]) == _bits(want[1]) and (masks[m] == want[2]).all()


# ---- 3. minimal solvers --------------------------------------------------------------------------------------------------

SOLVER_FLOOR_FACTOR = 32.0   # the device is a second elimination order with a rounding of its own
# 7-point samples, chosen on the CPU among the candidates 0..599 of solver_samples() so that the cubic's leading
# coefficient is above 1e-9 (the solver rejects below 1e-16) and no two of its roots are closer than 0.01 (relative):
# twelve with one real root, twelve with three. The case asserts the condition on every one of them.
F_CANDIDATES = [31, 49, 71, 86, 92, 113, 119, 122, 127, 132, 137, 145, 4, 10, 27, 36, 42, 47, 48, 50, 58, 62, 73, 74]
H_CANDIDATES = list(range(24))


def solver_samples(kind):
    """Seeded samples in pixel units: matches of a general scene (F) or of a plane (H) with 0.5 px of noise, so that
    the cubic of a 7-point sample has one real root for some and three for others."""
    pts, _ = scene("general" if kind == R.KIND_F else "plane", 400, 0, 77)
    k = R.MIN_SAMPLES[kind]
    out = []
    for c in (F_CANDIDATES if kind == R.KIND_F else H_CANDIDATES):
        rng = np.random.default_rng(5000 + c)
        out.append(np.ascontiguousarray(pts[rng.choice(len(pts), k, replace=False)] + rng.normal(scale=0.5, size=(k, 4))))
    return out


def _pair_models(got, want, up_to_sign):
    """The largest distance of a model of `want` to its nearest model of `got`."""
    return max(min(R.model_distance(g, w, up_to_sign) for g in got) for w in want)


def case_minimal_solvers(kind, report=None):
    samples = solver_samples(kind)
    sign = kind == R.KIND_F
    roots = set()
    worst = 0.0
    with TV.PointSets() as ps:
        # one set per sample, as large as the sample: its only sample is the set itself, in some order
        ps.set_points(samples, list(range(len(samples))))
        num, models = ps.hypothesize(kind, 0, [(s, 0, 1) for s in range(len(samples))])
    for s, p in enumerate(samples):
        if kind == R.KIND_F:
            lead, gap = R.cubic_condition(p)
            assert lead > 1e-9 and gap > 1e-2, (s, lead, gap)  # away from a zero leading coefficient and a double root
        exact = R.f7_mp(p) if kind == R.KIND_F else R.h4_mp(p)
        mine = R.solve_minimal(kind, p)
        assert len(mine) == len(exact) and len(exact) > 0, s
        assert num[s] == len(exact), (s, num[s], len(exact))
        roots.add(len(exact))
        floor = _pair_models(mine, exact, sign)
        dev = _pair_models(models[s, :num[s]], exact, sign)
        ratio = dev / floor if floor > 0 else (0.0 if dev == 0 else np.inf)
        worst = max(worst, ratio)
        if report is not None:
            report.append((s, len(exact), floor, dev, ratio))
        else:
            print(f"sample {s}: models {len(exact)} floor {floor:.3e} device {dev:.3e} ratio {ratio:.2f}")
    if report is None:
        if kind == R.KIND_F:
            assert roots == {1, 3}, roots
        assert worst <= SOLVER_FLOOR_FACTOR, worst
    return worst


def case_degenerate_samples():
    # repeated points: the 7 x 9 system has rank 6, no model; 4 collinear points: the homography is rejected
    rng = np.random.default_rng(5)
    six = rng.uniform(0, 800, (6, 4))
    repeated = np.vstack([six, six[2:3]])
    x = np.array([10.0, 200.0, 350.0, 700.0])
    collinear = np.stack([x, np.zeros(4), x + 5.0, np.zeros(4)], 1)
    with TV.PointSets() as ps:
        ps.set_points([repeated, collinear], [1, 2])
        nf, _ = ps.hypothesize(R.KIND_F, 0, [(0, 0, 3)])
        nh, _ = ps.hypothesize(R.KIND_H, 0, [(1, 0, 3)])
    assert (nf == 0).all() and (nh == 0).all()
    assert len(R.solve_h4(collinear)) == 0


# ---- 4. the sample draw --------------------------------------------------------------------------------------------------

def case_sample_draw(kind):
    sizes = [7, 8, 9, 1000]
    rng = np.random.default_rng(1)
    sets = [rng.uniform(0, 800, (n, 4)) for n in sizes]
    streams = [0, 1, 2 ** 63 + 12345, 2 ** 64 - 1]
    items = [(0, 0, 5), (3, 10 ** 12, 70), (1, 3, 4), (2, 0, 9), (3, 0, 3)]
    with TV.PointSets() as ps:
        ps.set_points(sets, streams)
        _, _, samples = ps.hypothesize(kind, 17, items, samples=True)
    g = 0
    for s, first, count in items:
        for t in range(first, first + count):
            want = R.draw_sample(17, streams[s], kind, t, sizes[s])
            assert (samples[g] == want).all(), (s, t, samples[g], want)
            assert (TV.draw_sample(17, streams[s], kind, t, sizes[s]) == want).all()
            assert len(set(want.tolist())) == R.MIN_SAMPLES[kind] and want.max() < sizes[s]
            g += 1


# ---- 5. properties of the search -----------------------------------------------------------------------------------------

def search_sets():
    return [scene("general", 100, 50, 21)[0], scene("plane", 70, 30, 22)[0], scene("general", 5, 1, 23)[0],
            scene("rotation", 30, 45, 24)[0]]


def _same(a: TV.Report, b: TV.Report):
    return (a.success == b.success and a.num_trials == b.num_trials and a.num_inliers == b.num_inliers and
            _bits(a.residual_sum) == _bits(b.residual_sum) and (_bits(a.model) == _bits(b.model)).all() and
            (a.inlier_mask == b.inlier_mask).all())


def case_search_properties(kind):
    sets, streams = search_sets(), [11, 12, 13, 14]
    T = TV.trial_round()
    o = _ransac()
    with TV.PointSets() as ps:
        ps.set_points(sets, streams)
        base = ps.estimate(kind, o)
        again = ps.estimate(kind, o)
        for s, (r, pts) in enumerate(zip(base, sets)):
            assert _same(r, again[s]), s
            if len(pts) < R.MIN_SAMPLES[kind]:
                assert not r.success and r.num_trials == 0
                continue
            clamp = R.clamped_max_num_trials(_ref_ransac(o), o.min_inlier_ratio, R.MIN_SAMPLES[kind])
            assert r.success and r.num_trials >= min(o.min_num_trials, clamp) + 1
            want = R.support(kind, r.model, pts, o.max_error)
            assert (r.inlier_mask == want[2]).all() and r.num_inliers == want[0] == int(r.inlier_mask.sum())
            assert _bits(r.residual_sum) == _bits(want[1])
        for per_round in (1, T - 1, T + 1):
            other = ps.estimate(kind, _ransac(trials_per_round=per_round))
            assert all(_same(a, b) for a, b in zip(base, other)), per_round
            if per_round == 1:
                assert other[0].num_launches > base[0].num_launches
        # another batch composition: one set alone, and the sets in another order
        ps.set_points([sets[1]], [streams[1]])
        assert _same(ps.estimate(kind, o)[0], base[1])
        ps.set_points(sets[::-1], streams[::-1])
        assert all(_same(a, b) for a, b in zip(ps.estimate(kind, o), base[::-1]))


# ---- 6. unambiguous scenes -----------------------------------------------------------------------------------------------

def _border_translation(n, seed):
    rng = np.random.default_rng(seed)
    p1 = np.stack([rng.uniform(5, 110, n), rng.uniform(5, 790, n)], 1)
    return np.hstack([p1, p1 + np.array([3.0, 2.0])]), np.ones(n, np.uint8)


def _two_motions(seed):
    a, ta = scene("general", 80, 0, seed)
    b, tb = scene("general", 60, 0, seed + 1, _rot([1.0, 0.2, 0.0], -0.12), np.array([-0.3, 0.8, 0.1]))
    c, tc = scene("general", 0, 10, seed + 2)
    return np.vstack([a, b, c]), np.concatenate([ta, tb, tc])


def _stationary(seed):
    pts, truth = scene("general", 60, 20, seed)
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0, W, 80), rng.uniform(0, H, 80)], 1)
    assert (((pts[:, :2] - pts[:, 2:]) ** 2).sum(1) > 16.0)[truth.astype(bool)].all()
    return np.vstack([pts, np.hstack([p, p])]), np.concatenate([truth, np.zeros(80, np.uint8)])


def scenes():
    """name -> (cameras, pts, truth, options, expected config)."""
    O = TV.TwoViewGeometryOptions
    seeded = dict(ransac_options=_ransac())
    # A fundamental matrix fitted to coplanar points (or to a rotation) keeps a free epipole and can always reach
    # through it for gross outliers; where it then counts more inliers than the homography, the reference returns ITS
    # mask (two_view_geometry.cc:311-314). So the scenes whose inlier set must equal the ground truth carry no outliers,
    # and the `_outliers` scenes assert what holds with them: see case_scene.
    general, plane, rotation = scene("general", 120, 60, 31), scene("plane", 120, 0, 32), scene("rotation", 120, 0, 33)
    plane_out, rotation_out = scene("plane", 120, 60, 32), scene("rotation", 120, 60, 33)
    return {
        "general": ((PINHOLE, PINHOLE2), *general, O(**seeded), TV.UNCALIBRATED),
        "plane": ((PINHOLE, PINHOLE2), *plane, O(**seeded), TV.PLANAR_OR_PANORAMIC),
        "rotation": ((PINHOLE, PINHOLE2), *rotation, O(**seeded), TV.PLANAR_OR_PANORAMIC),
        "plane_outliers": ((PINHOLE, PINHOLE2), *plane_out, O(**seeded), TV.PLANAR_OR_PANORAMIC),
        "rotation_outliers": ((PINHOLE, PINHOLE2), *rotation_out, O(**seeded), TV.PLANAR_OR_PANORAMIC),
        "fourteen": ((PINHOLE, PINHOLE2), general[0][:14], np.zeros(14, np.uint8), O(**seeded), TV.DEGENERATE),
        "two_motions": ((PINHOLE, PINHOLE2), *_two_motions(34), O(multiple_models=True, **seeded), TV.MULTIPLE),
        "watermark": ((PINHOLE, PINHOLE2), *_border_translation(60, 35), O(**seeded), TV.WATERMARK),
        "stationary": ((PINHOLE, PINHOLE2), *_stationary(36), O(filter_stationary_matches=True, **seeded), TV.UNCALIBRATED),
        "forced_h_plane": ((PINHOLE, PINHOLE2), *plane_out, O(force_H_use=True, **seeded), TV.PLANAR_OR_PANORAMIC),
        "forced_h_fisheye": ((FISHEYE, PINHOLE2), plane[0], np.zeros(len(plane[0]), np.uint8), O(force_H_use=True, **seeded),
                             TV.DEGENERATE),
        "fisheye": ((FISHEYE, PINHOLE2), general[0], np.zeros(len(general[0]), np.uint8), O(**seeded), TV.DEGENERATE),
    }


def _ref_options(o: TV.TwoViewGeometryOptions):
    return R.tvg_options(min_num_inliers=o.min_num_inliers, max_H_inlier_ratio=o.max_H_inlier_ratio,
                         watermark_min_inlier_ratio=o.watermark_min_inlier_ratio, watermark_border_size=o.watermark_border_size,
                         detect_watermark=o.detect_watermark, multiple_ignore_watermark=o.multiple_ignore_watermark,
                         watermark_detection_max_error=o.watermark_detection_max_error,
                         filter_stationary_matches=o.filter_stationary_matches,
                         stationary_matches_max_error=o.stationary_matches_max_error, force_H_use=o.force_H_use,
                         multiple_models=o.multiple_models, ransac=_ref_ransac(o.ransac_options))


def checker_answer(name):
    """What the checker's own search and decisions give for a scene (run on the CPU before the cases were committed,
    and by tests/test_two_view_geometry.py)."""
    cams, pts, truth, o, config = scenes()[name]
    if not (cams[0].is_perspective_pinhole() and cams[1].is_perspective_pinhole()):
        return TV.DEGENERATE, np.zeros(len(pts), np.uint8)
    return R.estimate_two_view_geometry((W, H), (W, H), pts, 1000 + len(pts), _ref_options(o), o.force_H_use)


def case_scene(name):
    cams, pts, truth, o, config = scenes()[name]
    with TV.PointSets() as ps:
        geoms, stats = ps.verify_pairs([cams[0]], [cams[1]], [pts], [1000 + len(pts)], o)
    g = geoms[0]
    assert g.config == config, (name, g.config, config)
    if name.endswith("_outliers"):
        # the homography's own inliers are the ground truth exactly; the returned mask holds them all and, where the
        # fundamental matrix reached further, outliers on its epipolar lines
        assert (R.support(R.KIND_H, g.H, pts, MAX_ERROR)[2] == truth).all(), name
        assert (g.inlier_mask.astype(np.uint8) >= truth).all(), name
        extra = g.inlier_mask & ~truth.astype(bool)
        assert not extra.any() or (R.residuals(R.KIND_F, g.F, pts[extra]) <= MAX_ERROR ** 2).all()
        return
    assert (g.inlier_mask.astype(np.uint8) == truth).all(), (name, int(g.inlier_mask.sum()), int(truth.sum()))
    if config == TV.UNCALIBRATED:
        assert g.F is not None
        assert R.support(R.KIND_F, g.F, pts[truth.astype(bool)], MAX_ERROR)[0] == truth.sum()
    if config == TV.PLANAR_OR_PANORAMIC:
        assert g.H is not None
    if config == TV.MULTIPLE:
        assert g.F is None and g.H is None
    assert stats["num_launches"] > 0 or config == TV.DEGENERATE


def case_scenes_in_one_batch():
    """All scenes of the default options in ONE call give what they give alone, and a pair on an unbuilt route is named."""
    S = scenes()
    names = ["general", "plane", "rotation", "plane_outliers", "fourteen", "watermark"]
    cams1 = [S[n][0][0] for n in names] + [PINHOLE, FISHEYE]
    cams2 = [S[n][0][1] for n in names] + [PINHOLE, PINHOLE2]   # a shared camera without a prior; a fisheye
    pts = [S[n][1] for n in names] + [S["general"][1], S["general"][1]]
    alone = []
    for n in names:
        with TV.PointSets() as ps:
            alone.append(ps.verify_pairs([S[n][0][0]], [S[n][0][1]], [S[n][1]], [1000 + len(S[n][1])], S[n][3])[0][0])
    with TV.PointSets() as ps:
        geoms, _ = ps.verify_pairs(cams1, cams2, pts, [1000 + len(p) for p in pts], S["general"][3])
    for n, g, a in zip(names, geoms, alone):
        assert g.config == S[n][4], n
        assert n.endswith("_outliers") or (g.inlier_mask.astype(np.uint8) == S[n][2]).all(), n
        assert (g.inlier_mask == a.inlier_mask).all() and g.config == a.config, n
        for x, y in ((g.F, a.F), (g.H, a.H)):
            assert (x is None) == (y is None) and (x is None or (_bits(x) == _bits(y)).all()), n
    shared, fisheye = geoms[len(names)], geoms[len(names) + 1]
    assert shared.config == TV.NOT_BUILT and shared.route == TV.ROUTE_SHARED_FOCAL and not shared.inlier_mask.any()
    assert fisheye.config == TV.DEGENERATE and fisheye.route == TV.ROUTE_FISHEYE_DEGENERATE


def case_public_function():
    cams, pts, truth, o, config = scenes()["general"]
    kp1 = np.hstack([pts[:, :2], np.ones((len(pts), 2))]).astype(np.float32)   # keypoints with scale and orientation
    kp2 = pts[:, 2:].astype(np.float32)
    matches = np.stack([np.arange(len(pts)), np.arange(len(pts))], 1).astype(np.uint32)
    from colmap_amd import pipeline
    g = pipeline.estimate_two_view_geometry(cams[0], kp1, cams[1], kp2, matches, o, stream_id=5)
    assert g.config == TV.UNCALIBRATED and (g.inlier_matches[:, 0] == np.flatnonzero(truth)).all()
    with pytest.raises(TV.TwoViewGeometryError, match="shared focal"):
        pipeline.estimate_two_view_geometry(PINHOLE, kp1, PINHOLE, kp2, matches, o)


def case_validation():
    with TV.PointSets() as ps:
        ps.set_points([np.zeros((3, 4))], [0])
        with pytest.raises(TV.TwoViewGeometryError, match="fewer matches than a minimal sample"):
            ps.hypothesize(R.KIND_F, 0, [(0, 0, 1)])
        with pytest.raises(TV.TwoViewGeometryError, match="set out of range"):
            ps.score(R.KIND_F, 1.0, [1], np.zeros((1, 9)))
        with pytest.raises(TV.TwoViewGeometryError, match="kind"):
            ps.score(5, 1.0, [0], np.zeros((1, 9)))
        with pytest.raises(TV.TwoViewGeometryError, match="min_num_trials"):
            ps.estimate(R.KIND_F, TV.RANSACOptions(min_num_trials=10, max_num_trials=5))
        r = ps.estimate(R.KIND_F, TV.RANSACOptions())[0]
        assert not r.success and r.num_trials == 0
        ps.set_points([], [])
        assert ps.estimate(R.KIND_H, TV.RANSACOptions()) == []


# ---- 7. the command --------------------------------------------------------------------------------------------------------

def make_database(path):
    """Four images: 1 and 2 with cameras of their own (uncalibrated route), 3 sharing camera 1 (shared-focal route, not
    built), 4 with a fisheye camera. Matches: (1, 2) a general scene, (1, 3) and (1, 4) the same points, (2, 3) 10
    matches, (2, 4) a pair with an old geometry row without inliers."""
    pts, truth = scene("general", 120, 60, 31)
    n = len(pts)
    with DB.Database(path, create=True) as db:
        db.create_verification_tables()
        for cid, model in ((1, 1), (2, 1), (3, 5)):
            params = np.array([800.0, 800, 500, 400] + [0.0] * (4 if model == 5 else 0))
            db.con.execute("INSERT INTO cameras VALUES (?, ?, ?, ?, ?, 0)", (cid, model, W, H, params.tobytes()))
        for iid, cid in ((1, 1), (2, 2), (3, 1), (4, 3)):
            db.write_image(f"im{iid}.jpg", cid, iid)
        kp1 = np.hstack([pts[:, :2], np.ones((n, 2))]).astype(np.float32)       # 4 columns
        kp2 = pts[:, 2:].astype(np.float32)                                      # 2 columns
        for iid, kp in ((1, kp1), (2, kp2), (3, kp2), (4, kp2)):
            db.con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (iid, kp.shape[0], kp.shape[1], kp.tobytes()))
        m = np.stack([np.arange(n), np.arange(n)], 1)
        db.write_matches(1, 2, m)
        db.write_matches(1, 3, m)
        db.write_matches(1, 4, m)
        db.write_matches(2, 3, m[:10])
        db.write_matches(2, 4, m)
        db.write_two_view_geometry(2, 4, np.zeros((0, 2), np.uint32), 0)
    return pts.astype(np.float32).astype(np.float64), truth


def run_command(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "colmap_amd", "geometric_verifier"] + args, capture_output=True, text=True,
                          cwd=ROOT, env=env)


def case_command(tmp_path, main):
    """main(argv) -> (return code, stderr)."""
    path = str(tmp_path / "database.db")
    pts, truth = make_database(path)
    want_config, want_mask = R.estimate_two_view_geometry((W, H), (W, H), pts, DB.image_pair_to_pair_id(1, 2),
                                                          R.tvg_options(ransac=R.ransac_options(random_seed=3)))
    assert want_config == R.UNCALIBRATED
    rc, err = main(["--database_path", path, "--TwoViewGeometry.random_seed", "3"])
    assert rc == 0, err
    assert "shared focal" in err and "1 pair" in err
    con = sqlite3.connect(path)
    rows = {r[0]: r[1:] for r in con.execute("SELECT pair_id, rows, cols, data, config, F, E, H, qvec, tvec FROM two_view_geometries")}
    pid = DB.image_pair_to_pair_id
    assert set(rows) == {pid(1, 2), pid(1, 4), pid(2, 3), pid(2, 4)}          # (1, 3): shared focal, left rowless
    nrows, ncols, data, config, F, E, Hm, qvec, tvec = rows[pid(1, 2)]
    assert config == TV.UNCALIBRATED and ncols == 2 and E is None and qvec is None and tvec is None
    inl = np.frombuffer(data, np.uint32).reshape(nrows, 2)
    assert (inl[:, 0] == np.flatnonzero(want_mask)).all() and (inl[:, 0] == inl[:, 1]).all()
    assert len(F) == 72 and len(Hm) == 72
    Fm = np.frombuffer(F, np.float64)
    assert R.support(R.KIND_F, Fm, pts, MAX_ERROR)[0] == nrows
    assert (inl[:, 0] == np.flatnonzero(truth)).all()
    assert rows[pid(1, 4)][0] == 0 and rows[pid(1, 4)][3] == TV.UNDEFINED      # fisheye without a prior: DEGENERATE, no inliers
    assert rows[pid(2, 3)][0] == 0 and rows[pid(2, 3)][3] == TV.UNDEFINED      # fewer than min_num_inliers matches
    assert rows[pid(2, 4)][0] == 0
    before = con.execute("SELECT pair_id, rows, data, config, F, H FROM two_view_geometries ORDER BY pair_id").fetchall()
    con.close()
    # a second run recomputes only the rows without inliers and leaves the others as they are
    rc, err = main(["--database_path", path, "--TwoViewGeometry.random_seed", "3"])
    assert rc == 0, err
    con = sqlite3.connect(path)
    after = con.execute("SELECT pair_id, rows, data, config, F, H FROM two_view_geometries ORDER BY pair_id").fetchall()
    con.close()
    assert after == before
    for flag, word in (("--TwoViewGeometry.use_degensac", "use_degensac"), ("--TwoViewGeometry.compute_relative_pose", "compute_relative_pose"),
                       ("--FeatureMatching.rig_verification", "rig_verification"), ("--FeatureMatching.guided_matching", "guided")):
        rc, err = main(["--database_path", path, flag, "1"])
        assert rc == 1 and word in err and "not built" in err, (flag, err)


# ---- the GPU tests -----------------------------------------------------------------------------------------------------------

KINDS = [R.KIND_F, R.KIND_H, R.KIND_T]
KIND_IDS = ["F", "H", "T"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_scores_are_exact(kind):
    case_scores_exact(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_batch_independence(kind):
    case_batch_independence(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS[:2], ids=KIND_IDS[:2])
def test_minimal_solvers(kind):
    """Largest observed ratio of the device's distance to the 50-digit solve over the checker's: see DESIGN.md 2.4f."""
    case_minimal_solvers(kind)


@pytest.mark.gpu
def test_degenerate_samples():
    case_degenerate_samples()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_sample_draw(kind):
    case_sample_draw(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_search_properties(kind):
    case_search_properties(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(scenes()))
def test_scene(name):
    case_scene(name)


@pytest.mark.gpu
def test_scenes_in_one_batch():
    case_scenes_in_one_batch()


@pytest.mark.gpu
def test_public_function():
    case_public_function()


@pytest.mark.gpu
def test_validation():
    case_validation()


@pytest.mark.gpu
def test_command(tmp_path):
    def main(argv):
        r = run_command(argv)
        return r.returncode, r.stderr
    case_command(tmp_path, main)
