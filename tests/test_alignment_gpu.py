"""Model alignment on the GPU (colmap_amd/csrc/model_align.hip behind colmap_amd/alignment.py) against the sequential
numpy checker tests/align_reference.py: hypothesis scoring (exact integer counts), batch invariance, position scoring,
the LORANSAC report for several batch sizes, the point transform and input validation. The case functions are shared
with tests/test_alignment_emul.py, which runs them through the CPU build of the unmodified source."""
import ctypes as C
import types

import numpy as np
import pytest

import align_reference as A
import test_obs_filter_gpu as OG
from colmap_amd import alignment as AL
from colmap_amd import scene

MAX_REPROJ = 8.0
INLIER_PX, OUTLIER_PX = 0.3, 60.0
# common points per image: nothing, less than a wave, the wave edges 63 | 64 | 65 and 127 | 129, several waves, and a
# spread of others up to 40 images
EDGE_COUNTS = [0, 1, 2, 63, 64, 65, 127, 129, 300] + [3 + (7 * k) % 38 for k in range(31)]
TRUE_SIM = A.sim_from_srt(1.7, scene.quat_to_rot(np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9])),
                          np.array([0.5, -1.0, 2.0]))
CENTER_NOISE = 1e-3  # bound on the displacement of a src projection centre in the search pair


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    q = np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])
    return scene.quat_to_rot(q)


def _project(rec, image_id, xyz):
    img = rec.images[image_id]
    return OG.Q.img_from_cam(rec.cameras[img.camera_id], OG.Q.point_in_cam(img, xyz))


def build_pair(counts, seed, gross_outlier_images=(), center_noise=0.0, point_noise=1e-4):
    """(src, tgt): tgt is the model, src its copy under Inverse(TRUE_SIM) with points of its own (point_noise apart), its
    own measured pixels and, for every third image, a camera of another model. Every image i holds counts[i] point2D
    indices with a 3D point in both models (one in ten of them, in images of 10 and more, with a 60 px outlier on one
    side) and, for every second image, indices with a 3D point in one model only."""
    rng = np.random.default_rng(seed)
    src, tgt = scene.Reconstruction(), scene.Reconstruction()
    for k, m in enumerate(OG.ALL_MODELS):
        src.cameras[k + 1] = OG._camera(m, k + 1)
        tgt.cameras[k + 1] = OG._camera(m, k + 1)
    ncam = len(OG.ALL_MODELS)
    inv = A.sim_inverse(TRUE_SIM)
    R, s, t = A.sim_rotation(TRUE_SIM), TRUE_SIM[0], TRUE_SIM[5:8]
    for i, n in enumerate(counts, start=1):
        v = rng.uniform(-1, 1, 3)
        center = 5.0 * v / np.linalg.norm(v)
        tgt_pose = OG._look_at_origin(center)
        tgt.images[i] = scene.Image(i, (i - 1) % ncam + 1, tgt_pose)
        # the same camera seen from the src frame: X_cam = R_t (s R X_s + t) + t_t = s (R_t R X_s + (R_t t + t_t) / s)
        Rt = scene.quat_to_rot(tgt_pose[:4])
        Rs, ts = Rt @ R, (Rt @ t + tgt_pose[4:]) / s
        if i in gross_outlier_images:
            ts = ts + Rs @ rng.uniform(-2, 2, 3)
        elif center_noise > 0:
            d = rng.uniform(-1, 1, 3)
            ts = ts - Rs @ (center_noise * rng.uniform(0.2, 1.0) * d / np.linalg.norm(d))  # centre moves by at most center_noise
        src.images[i] = scene.Image(i, ((i + 5) % ncam + 1) if i % 3 == 0 else (i - 1) % ncam + 1,
                                    np.concatenate([scene.rot_to_quat(Rs), ts]))

        def add(rec, xyz, px):
            if xyz is None:
                rec.images[i].points2D.append(scene.Point2D(rng.uniform(0, 500, 2), -1))
                return
            pid = len(rec.points3D) + 1
            proj = _project(rec, i, xyz)
            assert proj is not None and np.isfinite(proj).all()
            ang = rng.uniform(0, 2 * np.pi)
            rec.images[i].points2D.append(scene.Point2D(proj + px * np.array([np.cos(ang), np.sin(ang)]), pid))
            rec.points3D[pid] = scene.Point3D(np.asarray(xyz, np.float64), [(i, len(rec.images[i].points2D) - 1)])

        kinds = ["both"] * n + (["src", "tgt", "src", "tgt"] if i % 2 == 0 else [])
        for j in rng.permutation(len(kinds)):
            X = rng.uniform(-0.6, 0.6, 3)
            Xs = A.sim_apply(inv, X) + point_noise * rng.uniform(-1, 1, 3)
            if i in gross_outlier_images:
                Xs = A.sim_apply(inv, rng.uniform(-0.6, 0.6, 3))
            outlier = n >= 10 and rng.uniform() < 0.1
            side = rng.integers(0, 2)
            add(src, Xs if kinds[j] != "tgt" else None, OUTLIER_PX if outlier and side == 0 else INLIER_PX)
            add(tgt, X if kinds[j] != "src" else None, OUTLIER_PX if outlier and side == 1 else INLIER_PX)
    return src, tgt


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def edge_pair():
    return cached("edge_pair", lambda: build_pair(EDGE_COUNTS, seed=11))


def edge_hypotheses():
    """tile + 1 hypotheses: the true transform, two perturbed ones, one that moves the points onto a projection centre,
    and three-image samples from the stream."""
    def make():
        src, tgt = edge_pair()
        ids = A.common_image_ids(src, tgt)
        a = np.array([src.ProjectionCenter(i) for i in ids])
        b = np.array([tgt.ProjectionCenter(i) for i in ids])
        R, s, t = A.sim_rotation(TRUE_SIM), TRUE_SIM[0], TRUE_SIM[5:8]
        hyps = [TRUE_SIM.copy(),
                A.sim_from_srt(s, _rot([1, 2, -1], 0.12) @ R, _rot([1, 2, -1], 0.12) @ t + [0.02, 0.0, -0.02]),
                A.sim_from_srt(s * 1.02, _rot([0, 1, 1], -0.04) @ R, t + [0.0, 0.06, 0.0]),
                A.sim_from_srt(s, R, t + tgt.ProjectionCenter(ids[3]))]
        samples = A.Samples(3)
        while len(hyps) < AL.hypothesis_tile() + 1:
            idx = samples.draw(len(ids))
            h = A.horn(a[idx], b[idx])
            if h is not None:
                hyps.append(h)
        return np.array(hyps)
    return cached("edge_hypotheses", make)


def edge_errors():
    """The checker's squared errors of every (hypothesis, observation) of the edge pair, computed once."""
    return cached("edge_errors", lambda: [A.observation_errors(*edge_pair(), h) for h in edge_hypotheses()])


def assert_reproj_margins(errors, max_reproj_error):
    """No reprojection error within 1e-6 relative of the threshold: far above the 1e-6 px bar of the fp64 camera models
    relative to 8 px. A seed that trips this is changed, not the margin."""
    for per_image in errors:
        for e in per_image:
            root = np.sqrt(e[np.isfinite(e) & (e < A.DBL_MAX)])
            assert (np.abs(root - max_reproj_error) > 1e-6 * max_reproj_error).all()


def case_pair_shape():
    src, tgt = edge_pair()
    pair = AL.flatten_pair(src, tgt)
    assert pair.num_images == len(EDGE_COUNTS) <= 40
    common = np.bincount(pair.rec_image, minlength=pair.num_images)
    assert list(common) == EDGE_COUNTS
    assert any(p.HasPoint3D() != q.HasPoint3D() for i in src.images for p, q in zip(src.images[i].points2D, tgt.images[i].points2D))
    models = {(src.cameras[src.images[i].camera_id].model_id, tgt.cameras[tgt.images[i].camera_id].model_id) for i in src.images}
    assert {m for m, _ in models} == set(range(18)) and {m for _, m in models} == set(range(18))
    assert any(a != b for a, b in models) and any(scene.EQUIRECTANGULAR in ab for ab in models)
    errors = edge_errors()
    ratios = np.array([n / np.maximum(c, 1) for n, c in (A.counts_from_errors(e, MAX_REPROJ) for e in errors)])
    assert (ratios[0][np.array(EDGE_COUNTS) >= 10] > 0.5).all()                      # the true transform
    for h in (1, 2):                                                               # perturbed: images on both sides of 0.3
        assert (ratios[h][np.array(EDGE_COUNTS) >= 10] < 0.3).any() and (ratios[h] > 0.3).any()
    assert any((e == A.DBL_MAX).any() for e in errors[3])                            # points behind cameras


@pytest.fixture(scope="module")
def edge_scorer():
    with AL.ReprojScorer(AL.flatten_pair(*edge_pair())) as scorer:
        yield scorer


def case_reproj_score(scorer, B):
    hyps, errors = edge_hypotheses()[:B], edge_errors()[:B]
    assert_reproj_margins(errors, MAX_REPROJ)
    inliers, common = scorer.score(hyps, MAX_REPROJ)
    assert inliers.shape == (B, len(EDGE_COUNTS)) and inliers.dtype == np.uint32
    for h in range(B):
        want_inliers, want_common = A.counts_from_errors(errors[h], MAX_REPROJ)
        assert np.array_equal(common, want_common)
        assert np.array_equal(inliers[h], want_inliers), f"hypothesis {h}"


def case_reproj_batch_invariance(scorer):
    hyps = edge_hypotheses()
    tile = AL.hypothesis_tile()
    alone = [scorer.score(hyps[h:h + 1], MAX_REPROJ)[0][0] for h in range(4)]
    for h in range(4):
        others = [hyps[k] for k in range(len(hyps)) if k != h]
        for pos in (0, tile // 2, tile, len(others)):  # first, in a tile, first of the second tile, last
            batch = others[:pos] + [hyps[h]] + others[pos:]
            assert np.array_equal(scorer.score(batch, MAX_REPROJ)[0][pos], alone[h])


# ----------------------------------------------------------------------------------------------------------------------
# positions
# ----------------------------------------------------------------------------------------------------------------------

POSITION_MAX_ERROR = 0.1
POSITION_SIM = A.sim_from_srt(1.3, _rot([1, 1, 0], 0.7), np.array([0.5, -0.3, 0.2]))


def position_sets(N):
    """src within +-5 and tgt = POSITION_SIM * src within +-10, moved by 0.04 .. 0.08 (squared residual >= 1.6e-3) for
    inliers and by 0.5 .. 1 for every fifth point."""
    def make():
        rng = np.random.default_rng(100 + N)
        src = rng.uniform(-5, 5, (N, 3))
        d = rng.normal(size=(N, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        size = np.where(np.arange(N) % 5 == 2, rng.uniform(0.5, 1.0, N), rng.uniform(0.04, 0.08, N))
        tgt = np.array([A.sim_apply(POSITION_SIM, x) for x in src]) + size[:, None] * d
        assert np.abs(src).max() <= 5 and np.abs(tgt).max() <= 10 + 1
        return src, tgt
    return cached(("positions", N), make)


def position_hypotheses(B):
    R, s, t = A.sim_rotation(POSITION_SIM), POSITION_SIM[0], POSITION_SIM[5:8]
    rng = np.random.default_rng(8)
    hyps = [POSITION_SIM.copy()]
    while len(hyps) < B:
        k = len(hyps)
        hyps.append(A.sim_from_srt(s * (1 + 1e-3 * rng.normal()), _rot(rng.normal(size=3), 2e-3 * k) @ R, t + 5e-3 * k * rng.normal(size=3)))
    return np.array(hyps)


def case_position_score(N, B):
    src, tgt = position_sets(N)
    hyps = position_hypotheses(B)
    with AL.PositionScorer(src, tgt) as scorer:
        n, total, mask = scorer.score(hyps, POSITION_MAX_ERROR, want_mask=True)
        n2, total2 = scorer.score(hyps, POSITION_MAX_ERROR)
    assert np.array_equal(n, n2) and np.array_equal(total.view(np.uint64), total2.view(np.uint64))
    for h in range(B):
        r = A.position_residuals(src, tgt, hyps[h])
        assert (np.abs(np.sqrt(r) - POSITION_MAX_ERROR) > 1e-6 * POSITION_MAX_ERROR).all()  # the margin rule
        want_n, want_sum, want_mask = A.position_support(r, POSITION_MAX_ERROR)
        if h == 0:
            assert r[want_mask].min() >= 1e-3 and 0 < want_n < N
        assert n[h] == want_n and np.array_equal(mask[h], want_mask)
        # each term is conditioned to about 1e4 * 2^-52 (coordinates up to 10, residuals from 1e-3), reordering adds at
        # most N * 2^-53: 1e-10 leaves roughly 50x over that
        assert abs(np.longdouble(total[h]) - want_sum) <= 1e-10 * want_sum


def case_position_batch_invariance():
    src, tgt = position_sets(1000)
    tile = AL.hypothesis_tile()
    hyps = position_hypotheses(tile + 1)
    with AL.PositionScorer(src, tgt) as scorer:
        for h in (0, 5):
            n0, s0 = scorer.score(hyps[h:h + 1], POSITION_MAX_ERROR)
            others = [hyps[k] for k in range(len(hyps)) if k != h]
            for pos in (0, tile // 2, tile, len(others)):
                n, s = scorer.score(others[:pos] + [hyps[h]] + others[pos:], POSITION_MAX_ERROR)
                assert n[pos] == n0[0] and s[pos:pos + 1].view(np.uint64)[0] == s0.view(np.uint64)[0]


# ----------------------------------------------------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------------------------------------------------

SEARCH_COUNTS = [8 + (5 * k) % 9 for k in range(20)]
SEARCH_OUTLIER_IMAGES = (4, 13)  # 10 % of the images: wrong pose, unrelated points


def search_pair():
    return cached("search_pair", lambda: build_pair(SEARCH_COUNTS, seed=23, gross_outlier_images=SEARCH_OUTLIER_IMAGES,
                                                    center_noise=CENTER_NOISE))


def search_options(**kw):
    # seed 35: the first three samples of the stream each contain a gross-outlier image, so the best model changes
    # hands inside the first batch (asserted on the checker's trace)
    return AL.RANSACOptions(min_inlier_ratio=0.2, random_seed=35, **kw)


def checker_report(name, **kw):
    return cached(("checker_report", name), lambda: A.align_via_reprojections(*search_pair(), 0.3, MAX_REPROJ, search_options(**kw)))


def assert_same_report(got, want):
    assert got.success == want["success"]
    assert got.num_trials == want["num_trials"]
    assert got.num_inliers == want["num_inliers"]
    if want["success"]:
        assert np.array_equal(got.inlier_mask, want["inlier_mask"])
        assert abs(got.residual_sum - want["residual_sum"]) <= 1e-12 * max(1.0, want["residual_sum"])
        # both sides use the same closed form on the same samples
        assert A.sim_distance(got.model.params(), want["model"]) <= 1e-12


def case_search_matches_checker(B):
    want = checker_report("default")
    assert want["success"] and want["num_inliers"] == len(SEARCH_COUNTS) - len(SEARCH_OUTLIER_IMAGES)
    assert want["trace"][-1] >= 3
    with AL.ReprojScorer(AL.flatten_pair(*search_pair())) as scorer:
        got = scorer.estimate(0.3, MAX_REPROJ, search_options(batch_size=B))
    assert_same_report(got, want)
    assert [not m for m in got.inlier_mask] == [i in SEARCH_OUTLIER_IMAGES for i in range(1, len(SEARCH_COUNTS) + 1)]
    # The model is the least-squares similarity of the inlier images' projection centres. The src centres were moved by
    # at most CENTER_NOISE; a least-squares fit is, to first order, an orthogonal projection of the data onto the
    # 7-parameter family, which does not expand: the RMS distance of the fitted from the true centres is at most the RMS
    # of the noise as seen in the tgt frame, scale * CENTER_NOISE. Factor 2 for the second-order terms and for the refit
    # running on the inlier set of the previous model.
    src, _ = search_pair()
    clean = [A.sim_apply(A.sim_inverse(TRUE_SIM), c) for c in
             (search_pair()[1].ProjectionCenter(i) for i in sorted(src.images) if i not in SEARCH_OUTLIER_IMAGES)]
    d = np.array([A.sim_apply(got.model.params(), x) - A.sim_apply(TRUE_SIM, x) for x in clean])
    assert np.sqrt((d * d).sum(1).mean()) <= 2.0 * TRUE_SIM[0] * CENTER_NOISE


def case_search_edges(name):
    kw = {"min_num_trials": dict(min_num_trials=40), "max_num_trials": dict(max_num_trials=5),
          "dynamic_stop": dict(dyn_num_trials_multiplier=1.0)}[name]
    want = checker_report(name, **kw)
    with AL.ReprojScorer(AL.flatten_pair(*search_pair())) as scorer:
        got = scorer.estimate(0.3, MAX_REPROJ, search_options(batch_size=7, **kw))
    assert_same_report(got, want)
    if name == "min_num_trials":
        assert got.num_trials > 40
    if name == "max_num_trials":
        assert got.num_trials == 6  # the fetch_add that finds the limit counts too (loransac.h:216-221, 358)
    if name == "dynamic_stop":
        assert got.num_trials < checker_report("default")["num_trials"]


def case_search_too_few_images():
    src, tgt = build_pair([5, 6], seed=2)
    with AL.ReprojScorer(AL.flatten_pair(src, tgt)) as scorer:
        got = scorer.estimate(0.3, MAX_REPROJ)
    assert not got.success and got.num_trials == 0
    assert AL.AlignReconstructionsViaReprojections(src, tgt) is None


def case_public_functions():
    src, tgt = search_pair()
    report = []
    sim = AL.AlignReconstructionsViaReprojections(src, tgt, 0.3, MAX_REPROJ, options=search_options(), report=report)
    assert sim is not None and A.sim_distance(sim.params(), checker_report("default")["model"]) <= 1e-12
    errors = AL.ComputeImageAlignmentError(src, tgt, sim)
    want = A.image_alignment_errors(src, tgt, sim.params())
    assert np.allclose([(e.rotation_error_deg, e.proj_center_error) for e in errors], want, rtol=0, atol=1e-9)
    good = [e.proj_center_error for e in errors if e.image_name not in SEARCH_OUTLIER_IMAGES]
    assert max(good) <= 4.0 * TRUE_SIM[0] * CENTER_NOISE
    centers = AL.AlignReconstructionsViaProjCenters(src, tgt, 0.05)
    assert centers is not None and A.sim_distance(centers.params(), TRUE_SIM) <= 10 * CENTER_NOISE


# ----------------------------------------------------------------------------------------------------------------------
# transform, validation
# ----------------------------------------------------------------------------------------------------------------------

def case_transform(N):
    rng = np.random.default_rng(N)
    rec = scene.Reconstruction()
    for k in range(N):
        rec.points3D[k + 1] = scene.Point3D(rng.uniform(-10, 10, 3) * 10.0 ** rng.integers(-2, 3))
    pts = np.array([rec.points3D[k + 1].xyz for k in range(N)]).reshape(-1, 3)
    sim = AL.Sim3d.from_params(TRUE_SIM)
    got = AL.transform_points(pts, sim)
    rec.Transform(sim.scale, sim.RotationMatrix(), sim.translation)
    want = np.array([rec.points3D[k + 1].xyz for k in range(N)]).reshape(-1, 3)
    ulp = np.finfo(np.float64).eps * np.linalg.norm(want, axis=1, keepdims=True)
    assert (np.abs(got - want) <= 4 * ulp).all()
    # Inverse round trip: every step rounds relative to the size of its terms, |X| and |R^T t| / s at the end
    back = AL.transform_points(got, AL.Inverse(sim))
    size = np.linalg.norm(pts, axis=1, keepdims=True) + np.linalg.norm(sim.translation) / sim.scale
    assert (np.abs(back - pts) <= 32 * np.finfo(np.float64).eps * size).all()
    assert A.sim_distance(AL.Inverse(AL.Inverse(sim)).params(), TRUE_SIM) <= 1e-15


def _raw_pair(pair, **null):
    """align_reproj_create on a hand-filled struct; fields named in `null` are passed as null pointers."""
    keep = []

    def ptr(name, a):
        if name in null:
            return None
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)
    sc, tc = AL._c_cameras(pair.src_cameras), AL._c_cameras(pair.tgt_cameras)
    arrays = dict(src_poses=np.ascontiguousarray(pair.src_poses, np.float64), tgt_poses=np.ascontiguousarray(pair.tgt_poses, np.float64),
                  src_num_points2D=np.ascontiguousarray(pair.src_num_points2D, np.int32),
                  tgt_num_points2D=np.ascontiguousarray(pair.tgt_num_points2D, np.int32),
                  rec_image=np.ascontiguousarray(pair.rec_image, np.int32), rec_src_xyz=np.ascontiguousarray(pair.rec_src_xyz, np.float64),
                  rec_tgt_xyz=np.ascontiguousarray(pair.rec_tgt_xyz, np.float64), rec_src_xy=np.ascontiguousarray(pair.rec_src_xy, np.float64),
                  rec_tgt_xy=np.ascontiguousarray(pair.rec_tgt_xy, np.float64))
    cp = AL._Pair(pair.num_images, 0, len(pair.rec_image), None if "src_cameras" in null else C.cast(sc, C.c_void_p),
                  C.cast(tc, C.c_void_p), *[ptr(k, v) for k, v in arrays.items()])
    L, h = AL.lib(), C.c_void_p()
    rc = L.align_reproj_create(C.byref(cp), C.c_int32(0), C.byref(h))
    msg = L.align_last_error().decode() if rc else ""
    if h:
        L.align_destroy(h)
    return rc, msg


def case_validation():
    src, tgt = build_pair([5, 6, 7], seed=4)
    pair = AL.flatten_pair(src, tgt)
    assert _raw_pair(pair)[0] == 0
    for field in ("rec_image", "rec_tgt_xy", "src_poses", "tgt_num_points2D", "src_cameras"):
        rc, msg = _raw_pair(pair, **{field: True})
        assert rc != 0 and "null" in msg, field
    with pytest.raises(AL.AlignmentError, match="same length"):  # a short array
        AL.ReprojScorer(types.SimpleNamespace(**{**pair.__dict__, "num_images": pair.num_images, "rec_src_xy": pair.rec_src_xy[:-1]}))
    bad = AL.flatten_pair(src, tgt)
    bad.tgt_num_points2D = bad.tgt_num_points2D + np.array([0, 1, 0], np.int32)
    with pytest.raises(AL.AlignmentError, match="NumPoints2D"):
        AL.ReprojScorer(bad)
    bad = AL.flatten_pair(src, tgt)
    bad.src_cameras = [(99, 100, 100, [1.0, 2.0, 3.0])] + list(bad.src_cameras[1:])
    with pytest.raises(AL.AlignmentError, match="unknown camera model"):
        AL.ReprojScorer(bad)
    bad = AL.flatten_pair(src, tgt)
    bad.rec_image = bad.rec_image.copy()
    bad.rec_image[-1] = 3
    with pytest.raises(AL.AlignmentError, match="out of range"):
        AL.ReprojScorer(bad)
    with AL.ReprojScorer(pair) as scorer:
        with pytest.raises(AL.AlignmentError, match="negative"):
            scorer.score([TRUE_SIM], -1.0)
        with pytest.raises(AL.AlignmentError, match="negative"):
            scorer.estimate(0.3, -8.0)
        with pytest.raises(AL.AlignmentError, match="scale 0"):
            scorer.score([np.array([0.0, 1, 0, 0, 0, 0, 0, 0])], MAX_REPROJ)
        with pytest.raises(AL.AlignmentError, match="min_inlier_observations"):
            scorer.estimate(1.5, MAX_REPROJ)
    with pytest.raises(AL.AlignmentError, match="same number"):
        AL.PositionScorer(np.zeros((4, 3)), np.zeros((3, 3)))
    with AL.PositionScorer(np.zeros((4, 3)), np.ones((4, 3))) as scorer:
        with pytest.raises(AL.AlignmentError, match="negative"):
            scorer.score([TRUE_SIM], -0.5)
        with pytest.raises(AL.AlignmentError, match="positive"):
            scorer.estimate(AL.RANSACOptions(max_error=0.0))
    L, h = AL.lib(), C.c_void_p()
    assert L.align_positions_create(None, None, C.c_int64(5), C.c_int32(0), C.byref(h)) != 0 and not h
    assert "null" in L.align_last_error().decode()
    assert L.align_transform_points(None, C.c_int64(5), TRUE_SIM.ctypes.data_as(C.c_void_p), C.c_int32(0)) != 0


def case_empty_inputs():
    empty = AL.flatten_pair(scene.Reconstruction(), scene.Reconstruction())
    with AL.ReprojScorer(empty) as scorer:
        inliers, common = scorer.score([TRUE_SIM, TRUE_SIM], MAX_REPROJ)
        assert inliers.shape == (2, 0) and common.shape == (0,)
        assert scorer.score(np.zeros((0, 8)), MAX_REPROJ)[0].shape == (0, 0)
        rep = scorer.estimate()
        assert not rep.success and rep.num_trials == 0
    src, tgt = build_pair([0, 0, 0, 0], seed=6)  # images without a common point: every residual is 1
    with AL.ReprojScorer(AL.flatten_pair(src, tgt)) as scorer:
        inliers, common = scorer.score([TRUE_SIM], MAX_REPROJ)
        assert not inliers.any() and not common.any()
        assert not scorer.estimate(0.3, MAX_REPROJ, search_options(max_num_trials=20)).success
    with AL.PositionScorer(np.zeros((0, 3)), np.zeros((0, 3))) as scorer:
        n, s = scorer.score([TRUE_SIM], 1.0)
        assert n[0] == 0 and s[0] == 0.0
        assert not scorer.estimate(AL.RANSACOptions(max_error=1.0)).success
    assert AL.transform_points(np.zeros((0, 3)), AL.Sim3d()).shape == (0, 3)


# ----------------------------------------------------------------------------------------------------------------------
# the tests
# ----------------------------------------------------------------------------------------------------------------------

def batch_sizes():
    return [1, 2, 15, 16, 17]  # 1, 2 and ALIGN_HYPOTHESIS_TILE - 1, + 0, + 1 (checked in case_tile_size)


def case_tile_size():
    assert batch_sizes()[2:] == [AL.hypothesis_tile() + d for d in (-1, 0, 1)]


pytestmark = pytest.mark.gpu


def test_tile_size():
    case_tile_size()


def test_pair_has_the_shapes():
    case_pair_shape()


@pytest.mark.parametrize("B", batch_sizes())
def test_reproj_score_matches_checker(edge_scorer, B):
    case_reproj_score(edge_scorer, B)


def test_reproj_batch_invariance(edge_scorer):
    case_reproj_batch_invariance(edge_scorer)


@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("N", [3, 64, 65, 1000])
def test_position_score_matches_checker(N, B):
    case_position_score(N, B)


def test_position_batch_invariance():
    case_position_batch_invariance()


@pytest.mark.parametrize("B", [1, 7, 64])
def test_search_matches_checker(B):
    case_search_matches_checker(B)


@pytest.mark.parametrize("name", ["min_num_trials", "max_num_trials", "dynamic_stop"])
def test_search_edges(name):
    case_search_edges(name)


def test_search_too_few_images():
    case_search_too_few_images()


def test_public_functions():
    case_public_functions()


@pytest.mark.parametrize("N", [1, 257, 1000])
def test_transform_matches_host(N):
    case_transform(N)


def test_validation():
    case_validation()


def test_empty_inputs():
    case_empty_inputs()
