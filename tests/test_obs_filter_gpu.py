"""Observation / point filtering on the GPU (include/colmap_amd_obs.h) against the sequential checker
tests/obs_reference.py. The case functions are shared with tests/test_obs_filter_emul.py, which runs them through the
CPU stand-in build of the same source (tests/hip_emul/build_obs.sh).

Comparison rule: keep bytes, point statuses and filtered counts equal the checker's EXACTLY; per-point errors agree
within the bar of the camera models in fp64, 1e-6 px (tests/test_undistort_gpu.py case_points) -- for NORMALIZED divided
by the largest focal length of the case, for ANGULAR (degrees) by the largest pixels-per-degree, i.e. the SMALLEST bar any
camera of the case would give. Exact decisions only mean something away from the thresholds: the generator places every
observation error, every decisive triangulation angle and every depth at least 1 % from its threshold, and each case
asserts that first, on the checker's values. Nothing is excluded from the comparison.

The model "edges" holds every camera model at 8 x its distortion and the observations at which a model has no projection
or no inverse (edges_model, case_edges_shape)."""
import numpy as np
import pytest

import obs_reference as Q
import test_undistort_gpu as G
from colmap_amd import observation_manager as OM
from colmap_amd import scene

EQUI = scene.Camera(0, scene.EQUIRECTANGULAR, 1000, 500, np.array([1000.0, 500.0]))
ALL_MODELS = G.PERSPECTIVE_MODELS + [scene.EQUIRECTANGULAR]
assert len(ALL_MODELS) == 18
# thresholds per error type: 4 px, and its size in normalized units / degrees for focal lengths around 1000 px
THRESHOLD = {Q.PIXEL: 4.0, Q.NORMALIZED: 0.004, Q.ANGULAR: 0.25}
MIN_TRI_ANGLE = 1.5
INLIER_PX, OUTLIER_PX = 0.3, 60.0
# track lengths: 0 .. 3; the lane-group edges 16 | 17 and 64 | 65 of obs_plan.h with their neighbours; one long track
# whose pair loop takes several steps of a whole wave; more of each class so that every class has more than one
# workgroup (256 lanes = 256 / 16 / 4 points) and none is a multiple of it
EDGE_LENGTHS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 200, 70, 100, 129, 66] + [17 + 2 * k for k in range(19)]
NUM_NORMAL_IMAGES = 204


def _camera(model, camera_id):
    if model == scene.EQUIRECTANGULAR:
        return scene.Camera(camera_id, model, EQUI.width, EQUI.height, EQUI.params.copy())
    c = G.ba_camera(model)
    return scene.Camera(camera_id, model, c.width, c.height, np.array(c.params, np.float64))


def _look_at_origin(center, away=False):
    view = -center / np.linalg.norm(center)
    if away:
        view = -view
    q = scene.quat_from_two_vectors(view, np.array([0.0, 0.0, 1.0]))
    return np.concatenate([q, scene.quat_to_rot(q) @ (-center)])


class Builder:
    def __init__(self, models, seed):
        self.rng = np.random.default_rng(seed)
        self.rec = scene.Reconstruction()
        for k, m in enumerate(models):
            self.rec.cameras[k + 1] = _camera(m, k + 1)
        self.ncam = len(models)
        self.normal, self.back, self.direction = [], [], {}

    def add_image(self, pose, camera_id=None):
        iid = len(self.rec.images) + 1
        cid = camera_id or (iid - 1) % self.ncam + 1
        self.rec.images[iid] = scene.Image(iid, cid, np.asarray(pose, np.float64))
        return iid

    def add_point(self, xyz, image_ids, outliers=()):
        """A point observed in image_ids; the measured pixel is the projection moved by INLIER_PX (OUTLIER_PX for the
        track positions in `outliers`) in a random direction, a random pixel where there is no projection."""
        pid = len(self.rec.points3D) + 1
        pt = scene.Point3D(np.asarray(xyz, np.float64))
        for k, iid in enumerate(image_ids):
            img = self.rec.images[iid]
            cam = self.rec.cameras[img.camera_id]
            proj = Q.img_from_cam(cam, Q.point_in_cam(img, pt.xyz))
            if proj is None or not np.isfinite(proj).all():
                xy = np.array([self.rng.uniform(0, cam.width), self.rng.uniform(0, cam.height)])
            else:
                ang = self.rng.uniform(0, 2 * np.pi)
                xy = proj + (OUTLIER_PX if k in outliers else INLIER_PX) * np.array([np.cos(ang), np.sin(ang)])
            img.points2D.append(scene.Point2D(xy, pid))
            pt.track.append((iid, len(img.points2D) - 1))
        self.rec.points3D[pid] = pt
        return pid


def build_model(models, seed, lengths=EDGE_LENGTHS, num_short=330):
    b = Builder(models, seed)
    rng = b.rng
    for _ in range(NUM_NORMAL_IMAGES):
        v = rng.uniform(-1, 1, 3)
        b.normal.append(b.add_image(_look_at_origin(5.0 * v / np.linalg.norm(v))))
        b.direction[b.normal[-1]] = v / np.linalg.norm(v)
    for _ in range(2 * b.ncam if b.ncam > 1 else 6):  # images that look away: everything near the origin is behind them
        v = rng.uniform(-1, 1, 3)
        b.back.append(b.add_image(_look_at_origin(5.0 * v / np.linalg.norm(v), away=True)))

    def near():
        return rng.uniform(-0.6, 0.6, 3)

    def pick(n):
        return [int(i) for i in rng.choice(b.normal, n, replace=False)]

    for L in lengths:                                       # the edge lengths, mostly clean
        out = set(int(k) for k in rng.choice(L, L // 10, replace=False)) if L >= 10 else set()
        b.add_point(near(), pick(L), out)
    for k in range(num_short):                              # short tracks of every kind
        L = int(rng.integers(2, 13))
        kind = k % 6
        if kind == 0:                                       # low parallax: 2000 units away, angles around 0.3 degrees,
            v = rng.uniform(-1, 1, 3)                           # seen by the L images that face it most directly
            v /= np.linalg.norm(v)
            facing = sorted(b.normal, key=lambda i: float(b.direction[i] @ v))[:L]
            b.add_point(2000.0 * v, [facing[i] for i in rng.permutation(L)])
        elif kind == 1:                                     # some outliers, the point survives
            b.add_point(near(), pick(L + 2), set(range(L // 3)))
        elif kind == 2:                                     # all but one (or all) observations are outliers
            b.add_point(near(), pick(L), set(range(L - int(rng.integers(0, 2)))))
        else:
            b.add_point(near(), pick(L))
    for L in (2, 3, 4):                                     # negative depth: k of L observations behind their camera
        for k in range(1, L + 1):
            for rep in range(2):
                ids = [int(i) for i in rng.choice(b.back, k, replace=False)] + pick(L - k)
                b.add_point(near(), [ids[i] for i in rng.permutation(L)])
    # a point ON a projection centre: identity rotation and integer translation make cam_from_world * X exactly zero
    centre_img = b.add_image([0, 0, 0, 1, -1.0, -2.0, -3.0], camera_id=1)
    b.add_point([1.0, 2.0, 3.0], [centre_img] + pick(3))
    if b.ncam > 1:
        centre_sph = b.add_image([0, 0, 0, 1, 2.0, -1.0, 0.5], camera_id=b.ncam)  # the spherical camera is the last one
        b.add_point([-2.0, 1.0, -0.5], [centre_sph] + pick(3))
    # "errors, then angles": three images 1e-3 apart and one far image; the far one is the only partner with a large
    # angle, and its observation is an outlier -- the error rule removes it, the angle rule then finds no pair
    c = np.array([0.0, 0.0, -5.0])
    cluster = [b.add_image(_look_at_origin(c + d), camera_id=1) for d in ([0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0])]
    for far in pick(3):
        b.add_point(near() * 0.2, cluster + [far], outliers={3})
        b.add_point(near() * 0.2, cluster + [far])          # the same without the outlier: kept
    return b.rec


def seam_model(seed=5):
    """EQUIRECTANGULAR only, points all around the cameras, measured pixels on either side of the +-pi seam."""
    b = Builder([scene.EQUIRECTANGULAR], seed)
    rng = b.rng
    imgs = [b.add_image(np.concatenate([scene.quat_from_two_vectors(np.array([0.0, 0.0, 1.0]), rng.uniform(-1, 1, 3)),
                                        rng.uniform(-0.5, 0.5, 3)])) for _ in range(24)]
    for k in range(150):
        v = rng.uniform(-1, 1, 3)
        L = int(rng.integers(2, 9))
        ids = [int(i) for i in rng.choice(imgs, L, replace=False)]
        pid = b.add_point(3.0 * v / np.linalg.norm(v), ids, {0} if k % 5 == 0 else ())
        for (im, idx) in b.rec.points3D[pid].track:          # the same bearing, written one image width further
            p2 = b.rec.images[im].points2D[idx]
            if p2.xy[0] < 40.0 or k % 7 == 0:
                p2.xy = p2.xy + np.array([1000.0, 0.0])
            elif p2.xy[0] > 960.0:
                p2.xy = p2.xy - np.array([1000.0, 0.0])
    # the reference's own seam case (observation_manager_test.cc:215-269): the back direction seen at x = 0
    a = b.add_image([0, 0, 0, 1, 0, 0, 0])
    c = b.add_image([0, 0, 0, 1, 0, 0, 0])
    pid = b.add_point([0.0, 0.0, -2.0], [a, c])
    for (im, idx) in b.rec.points3D[pid].track:
        b.rec.images[im].points2D[idx].xy = np.array([0.0, 250.0])
    return b.rec


EDGE_FEATURES = ("no_inverse_not_converged", "no_inverse_outside_eucm", "tiny_positive_depth", "behind_division_projects",
                 "behind_opencv_does_not", "disc_sq_negative", "eucm_den_small", "fisheye_theta_beyond_half_pi")
_EDGE_POINTS = {}


def edges_model(seed=21):
    """Every camera model at 8 x its distortion (tests/camera_edge_cases.py), EQUIRECTANGULAR, and the two cameras whose
    forward domain ends at a finite angle for points in FRONT of them (DIVISION with k = +0.2, EUCM with alpha = 1.2,
    beta = -0.3: at 8 x the suite's parameters neither rule can fire for w > 0). Each camera has two images, a point is
    seen by the two images of one camera, and EDGE_FEATURES names the observations the model exists for (their point
    ids are kept in _EDGE_POINTS; case_edges_shape restates each from the checker)."""
    import camera_edge_cases as E
    import undistort_reference as R
    b = Builder([], seed)
    rng = b.rng
    cams = []
    for m in G.PERSPECTIVE_MODELS:
        c = G.strong(G.ba_camera(m), 8.0)
        cams.append((m, c.width, c.height, c.params))
    cams.append((scene.EQUIRECTANGULAR, EQUI.width, EQUI.height, EQUI.params))
    for name in ("forward-DIVISION-k0.2", "forward-EUCM-1.2--0.3"):
        c = E.case(name).cam
        cams.append((c.model_id, c.width, c.height, c.params))
    for k, (m, w, h, p) in enumerate(cams):
        b.rec.cameras[k + 1] = scene.Camera(k + 1, m, w, h, np.array(p, np.float64))
    b.ncam = len(cams)
    # identity rotations: a point's camera coordinates in the first image are its world coordinates
    pair = {cid: [b.add_image([0, 0, 0, 1, 0.0, 0.0, 0.0], cid), b.add_image([0, 0, 0, 1, 0.3, -0.2, 0.1], cid)]
            for cid in b.rec.cameras}
    first = {}
    for cid, c in b.rec.cameras.items():
        first.setdefault(c.model_id, cid)
    for cid in b.rec.cameras:
        for k in range(36):                                  # a 6 x 6 fan of bearings out to |u| = 1, |v| = 0.8
            u = (k % 6 - 2.5) * 0.4 + rng.uniform(-0.05, 0.05)
            v = (k // 6 - 2.5) * 0.32 + rng.uniform(-0.05, 0.05)
            z = rng.uniform(3.0, 5.0)
            b.add_point([u * z, v * z, z], pair[cid], {0} if k % 9 == 4 else ())
        for _ in range(2):                                   # low parallax: 0.37 / 400 rad
            b.add_point([rng.uniform(-20, 20), rng.uniform(-20, 20), 400.0], pair[cid])

    def special(feature, model, xyz, pixel=None, camera_id=None):
        cid = camera_id or first[model]
        pid = b.add_point(xyz, pair[cid])
        if pixel is not None:
            im, idx = b.rec.points3D[pid].track[0]
            b.rec.images[im].points2D[idx].xy = np.array(pixel, np.float64)
        _EDGE_POINTS[feature] = pid

    full = b.rec.cameras[first[scene.FULL_OPENCV]]
    lost = np.isnan(R.cam_from_img(R.Camera(full.model_id, full.width, full.height, full.params), E.ITERATIVE_GRID)[:, 0])
    special("no_inverse_not_converged", scene.FULL_OPENCV, [0.4, 0.4, 4.0], E.ITERATIVE_GRID[np.nonzero(lost)[0][0]])
    special("no_inverse_outside_eucm", scene.EUCM, [0.4, -0.4, 4.0], [-4000.0, 384.0])
    special("tiny_positive_depth", scene.SIMPLE_RADIAL, [0.3, 0.2, 1e-17])
    special("behind_division_projects", scene.DIVISION, [0.4, -0.3, -2.0])
    special("behind_opencv_does_not", scene.OPENCV, [0.4, -0.3, -2.0])
    special("disc_sq_negative", scene.DIVISION, [6.0, 2.0, 4.0], camera_id=b.ncam - 1)
    special("eucm_den_small", scene.EUCM, [1.81 * 4.0, 0.0, 4.0], camera_id=b.ncam)
    fish = b.rec.cameras[first[scene.FISHEYE]]
    special("fisheye_theta_beyond_half_pi", scene.FISHEYE, [0.5, 0.1, 4.0],
            [fish.params[2] + 1.7 * fish.params[0] * np.cos(0.4), fish.params[3] + 1.7 * fish.params[1] * np.sin(0.4)])
    return b.rec


_MODELS = {}


def model(name):
    """Built once and never changed: every case works on copies."""
    if name not in _MODELS:
        _MODELS[name] = {"mixed": lambda: build_model(ALL_MODELS, 11), "single": lambda: build_model([scene.SIMPLE_RADIAL], 12),
                         "seam": seam_model, "edges": edges_model, "empty": scene.Reconstruction}[name]()
    return _MODELS[name]


_WANT = {}


def checker(name, entry, error_type=Q.PIXEL, rules=3):
    """(filtered reconstruction, trace, count) of the sequential checker, computed once per (model, call)."""
    key = (name, entry, error_type, rules)
    if key not in _WANT:
        rec, tr = model(name).copy(), Q.Trace()
        ids = list(rec.points3D)
        if entry == "filter_all_points3D":
            n = 0
            if rules & 1:
                n += Q.FilterPoints3DWithLargeReprojectionError(rec, THRESHOLD[error_type], ids, error_type, tr)
            if rules & 2:
                n += Q.FilterPoints3DWithSmallTriangulationAngle(rec, MIN_TRI_ANGLE, ids, tr)
        elif entry == "filter_short_tracks":
            n = Q.FilterPoints3DWithShortTracks(rec, 4, tr)
        elif entry == "filter_negative_depth":
            n = Q.FilterObservationsWithNegativeDepth(rec, tr)
        else:
            Q.UpdatePoint3DErrors(rec)
            n = 0
        _WANT[key] = (rec, tr, n)
    return _WANT[key]


def assert_margins(tr, error_type):
    """Every value a decision was taken on is at least 1 % from its threshold (on the checker's values)."""
    thr = THRESHOLD[error_type]
    e = np.array(tr.errors)
    if len(e):
        assert not np.isnan(e).any()
        assert (np.abs(e - thr) >= 0.01 * thr).all(), f"an observation error within 1 % of {thr}: {e[np.abs(e - thr) < 0.01 * thr]}"
    a = np.array(tr.angles)
    if len(a):
        t = np.deg2rad(MIN_TRI_ANGLE)
        assert (np.abs(a - t) >= 0.01 * t).all(), "a decisive triangulation angle within 1 % of the threshold"
    d = np.array(tr.depths)
    if len(d):
        assert (np.abs(d - Q.EPS) >= 0.01 * Q.EPS).all(), "a depth within 1 % of DBL_EPSILON"


def error_bar(rec, error_type):
    focal = max([float(max(c.params[:2])) if c.model_id != scene.EQUIRECTANGULAR else c.width / (2 * np.pi)
                 for c in rec.cameras.values()] or [1.0])
    return {Q.PIXEL: 1e-6, Q.NORMALIZED: 1e-6 / focal, Q.ANGULAR: 1e-6 / (focal * np.pi / 180.0)}[error_type]


def compare(name, entry, error_type=Q.PIXEL, rules=3):
    src = model(name)
    want_rec, tr, want_n = checker(name, entry, error_type, rules)
    assert_margins(tr, error_type)
    m, ids = OM.flatten(src)
    kw = dict(max_reproj_error=THRESHOLD[error_type], min_tri_angle=MIN_TRI_ANGLE, min_track_len=4, error_type=error_type,
              rules=rules)
    got = OM.run_flat(entry, m, **kw)
    again = OM.run_flat(entry, m, **kw)
    for f in ("obs_keep", "point_status", "point_error", "point_count"):
        assert getattr(got, f).tobytes() == getattr(again, f).tobytes(), f"{f} differs between two runs"
    assert got.num_filtered == again.num_filtered
    # the checker's decisions in the flat order
    status = np.array([tr.status.get(pid, Q.KEPT) for pid in ids], np.uint8)
    count = np.array([tr.count.get(pid, 0) for pid in ids], np.uint32)
    keep = np.zeros(len(m.obs_image), np.uint8)
    for k, pid in enumerate(ids):
        if pid in want_rec.points3D:
            left = set(want_rec.points3D[pid].track)
            keep[m.obs_offsets[k]:m.obs_offsets[k + 1]] = [el in left for el in src.points3D[pid].track]
    assert np.array_equal(got.point_status, status), np.nonzero(got.point_status != status)[0][:10]
    assert np.array_equal(got.obs_keep, keep), np.nonzero(got.obs_keep != keep)[0][:10]
    assert np.array_equal(got.point_count, count), np.nonzero(got.point_count != count)[0][:10]
    assert got.num_filtered == want_n == int(count.sum())
    sets_error = entry == "point_errors" or (entry == "filter_all_points3D" and rules & 1)
    worst = 0.0
    for k, pid in enumerate(ids):
        if status[k] != Q.KEPT or not sets_error:
            assert got.point_error[k] == -1.0
            continue
        w, g = want_rec.points3D[pid].error, got.point_error[k]
        worst = max(worst, 0.0 if g == w else abs(g - w))
    bar = error_bar(src, error_type)
    print(f"{name} {entry} type {error_type} rules {rules}: {len(ids)} points, {len(keep)} observations, filtered {want_n}, "
          f"statuses {np.bincount(status, minlength=5).tolist()}, max |error - checker| {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar
    return got, status


def case_model_shape():
    """What the generated model must contain for the cases to mean anything."""
    rec = model("mixed")
    lengths = np.array([len(p.track) for p in rec.points3D.values()])
    for L in (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 200):
        assert (lengths == L).any(), L
    assert {c.model_id for c in rec.cameras.values()} == set(ALL_MODELS)
    used = {rec.cameras[rec.images[im].camera_id].model_id for p in rec.points3D.values() for (im, _) in p.track}
    assert used == set(ALL_MODELS)
    assert 2000 <= lengths.sum() <= 8000 and len(lengths) % 256 != 0
    for lo, hi, per_block in ((0, 16, 256), (17, 64, 16), (65, 10 ** 9, 4)):
        n = int(((lengths >= lo) & (lengths <= hi)).sum())
        assert n > per_block and n % per_block != 0, (lo, hi, n)


def case_edges_shape():
    """What the "edges" model must contain, restated from the checker and the model alone."""
    import undistort_reference as R
    rec = model("edges")
    assert {c.model_id for c in rec.cameras.values()} == set(ALL_MODELS) and len(rec.cameras) == 20
    assert all(len(p.track) == 2 for p in rec.points3D.values())
    per_camera = np.bincount([rec.images[p.track[0][0]].camera_id for p in rec.points3D.values()], minlength=21)[1:]
    assert (per_camera >= 38).all() and (per_camera <= 42).all()
    assert set(_EDGE_POINTS) == set(EDGE_FEATURES)

    def first_observation(feature):
        pt = rec.points3D[_EDGE_POINTS[feature]]
        im, idx = pt.track[0]
        img = rec.images[im]
        cam = rec.cameras[img.camera_id]
        return cam, Q.point_in_cam(img, pt.xyz), img.points2D[idx].xy

    def inverse(cam, xy):
        return R.cam_from_img(R.Camera(cam.model_id, cam.width, cam.height, cam.params), xy[None])[0]

    for feature in ("no_inverse_not_converged", "no_inverse_outside_eucm"):
        cam, _, xy = first_observation(feature)
        assert np.isnan(inverse(cam, xy)).all(), feature
    cam, pc, _ = first_observation("tiny_positive_depth")
    assert 0.0 < pc[2] < Q.EPS and Q.img_from_cam(cam, pc) is None
    cam, pc, _ = first_observation("behind_division_projects")
    assert cam.model_id == scene.DIVISION and pc[2] < 0 and np.isfinite(Q.img_from_cam(cam, pc)).all()
    cam, pc, _ = first_observation("behind_opencv_does_not")
    assert cam.model_id == scene.OPENCV and pc[2] < 0 and Q.img_from_cam(cam, pc) is None
    cam, pc, _ = first_observation("disc_sq_negative")
    assert pc[2] > Q.EPS and pc[2] ** 2 - 4.0 * (pc[0] ** 2 + pc[1] ** 2) * cam.params[4] < -1.0 and Q.img_from_cam(cam, pc) is None
    cam, pc, _ = first_observation("eucm_den_small")
    rho2 = cam.params[5] * (pc[0] ** 2 + pc[1] ** 2) + pc[2] ** 2
    assert pc[2] > Q.EPS and rho2 > 0.01 and cam.params[4] * np.sqrt(rho2) + (1.0 - cam.params[4]) * pc[2] < -0.01
    assert Q.img_from_cam(cam, pc) is None
    cam, _, xy = first_observation("fisheye_theta_beyond_half_pi")
    theta = np.hypot((xy[0] - cam.params[2]) / cam.params[0], (xy[1] - cam.params[3]) / cam.params[1])
    assert theta > np.pi / 2 + 0.1 and np.isfinite(inverse(cam, xy)).all()


def case_filter_all(name, error_type):
    got, status = compare(name, "filter_all_points3D", error_type)
    if name != "seam":
        assert (status == Q.DELETED_ERROR).any() and (status == Q.DELETED_ANGLE).any() and (status == Q.KEPT).any()


def case_order_errors_then_angles():
    """The points whose only large-angle pair holds an outlier go by ANGLE under both rules, and stay under the angle
    rule alone; their twins without the outlier stay."""
    src = model("single")
    both, st_both = compare("single", "filter_all_points3D", Q.PIXEL, 3)
    angle, st_angle = compare("single", "filter_all_points3D", Q.PIXEL, 2)
    compare("single", "filter_all_points3D", Q.PIXEL, 1)
    ids = list(src.points3D)
    pairs = ids[-6:]
    for k in range(0, 6, 2):
        i, j = ids.index(pairs[k]), ids.index(pairs[k + 1])
        assert st_both[i] == Q.DELETED_ANGLE and both.point_count[i] == 4      # 1 by error + 3 by angle
        assert st_angle[i] == Q.KEPT and st_both[j] == Q.KEPT and st_angle[j] == Q.KEPT


def case_negative_depth(name):
    got, status = compare(name, "filter_negative_depth")
    assert (status == Q.DELETED_DEPTH).any()
    src = model(name)
    # the count rule on the constructed tracks: L observations, k of them behind their (non-spherical) camera
    seen = set()
    for k, (pid, pt) in enumerate(src.points3D.items()):
        L = len(pt.track)
        neg = sum(1 for (im, idx) in pt.track
                  if src.cameras[src.images[im].camera_id].model_id != scene.EQUIRECTANGULAR
                  and Q.point_in_cam(src.images[im], pt.xyz)[2] < Q.EPS)
        if 2 <= L <= 4 and neg:
            seen.add((L, neg))
            assert got.point_count[k] == min(neg, L - 1) and (status[k] == Q.DELETED_DEPTH) == (neg >= L - 1)
    assert {(2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3), (4, 4)} <= seen or name != "single"


def case_short_tracks(name):
    got, status = compare(name, "filter_short_tracks")
    assert (status == Q.DELETED_SHORT).any() and (status == Q.KEPT).any()


def case_point_errors(name):
    compare(name, "point_errors")


def case_empty_model():
    for entry in ("filter_all_points3D", "filter_short_tracks", "filter_negative_depth", "point_errors"):
        got = OM.run_flat(entry, OM.flatten(scene.Reconstruction())[0])
        assert got.num_filtered == 0 and len(got.obs_keep) == 0 and len(got.point_status) == 0
    rec = scene.Reconstruction()
    om = OM.ObservationManager(rec)
    assert om.FilterAllPoints3D(4.0, 1.5) == 0 and om.FilterPoints3DWithShortTracks(2) == 0
    assert om.FilterObservationsWithNegativeDepth() == 0
    # images and cameras, points without observations
    rec = model("single").copy()
    for pid in list(rec.points3D):
        rec.DeletePoint3D(pid)
    rec.points3D[1] = scene.Point3D(np.zeros(3))
    assert OM.ObservationManager(rec).FilterObservationsWithNegativeDepth() == 0 and 1 in rec.points3D
    assert OM.ObservationManager(rec).FilterAllPoints3D(4.0, 1.5) == 0 and not rec.points3D


def case_input_validation():
    m, _ = OM.flatten(model("single"))
    import copy

    def bad(**kw):
        b = copy.copy(m)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    off = m.obs_offsets.copy()
    off[0] = 1
    dec = m.obs_offsets.copy()
    dec[5] = dec[4] - 1
    img = m.obs_image.copy()
    img[3] = len(m.image_poses)
    cam = m.image_camera.copy()
    cam[0] = -1
    for b, what in ((bad(obs_offsets=off), "start at 0"), (bad(obs_offsets=dec), "decreases"), (bad(obs_image=img), "image index"),
                    (bad(image_camera=cam), "camera index"), (bad(cameras=[(99, 10, 10, [1.0, 2.0])]), "unknown camera model"),
                    (bad(cameras=[(scene.SIMPLE_RADIAL, 10, 10, [1.0, 2.0, 3.0])]), "takes 4 parameters")):
        with pytest.raises(OM.ObservationFilterError, match=what):
            OM.run_flat("filter_all_points3D", b)
    with pytest.raises(OM.ObservationFilterError, match="error_type"):
        OM.run_flat("filter_all_points3D", m, error_type=7)
    with pytest.raises(OM.ObservationFilterError, match="gpu_index"):
        OM.run_flat("filter_all_points3D", m, gpu_index=1000)


def case_manager_applies_deletions():
    """The class surface: the filtered Reconstruction equals the checker's -- points, tracks, point3D_ids, errors."""
    for name in ("mixed", "seam"):
        got, want = model(name).copy(), model(name).copy()
        n_got = OM.ObservationManager(got).FilterAllPoints3D(4.0, MIN_TRI_ANGLE) + \
            OM.ObservationManager(got).FilterPoints3DWithShortTracks(3)
        n_want = Q.FilterAllPoints3D(want, 4.0, MIN_TRI_ANGLE) + Q.FilterPoints3DWithShortTracks(want, 3)
        assert n_got == n_want
        assert_same_model(got, want)
        got.UpdatePoint3DErrors()
        Q.UpdatePoint3DErrors(want)
        assert max(abs(got.points3D[p].error - want.points3D[p].error) for p in want.points3D) <= 1e-6
        assert got.ComputeNumObservations() == sum(len(p.track) for p in want.points3D.values())
        assert abs(got.ComputeMeanTrackLength() - got.ComputeNumObservations() / len(got.points3D)) < 1e-12
        assert abs(got.ComputeMeanReprojectionError() - np.mean([p.error for p in want.points3D.values()])) <= 1e-6


def assert_same_model(got, want):
    assert sorted(got.points3D) == sorted(want.points3D)
    for pid in want.points3D:
        assert got.points3D[pid].track == want.points3D[pid].track
    for iid in want.images:
        assert [p.point3D_id for p in got.images[iid].points2D] == [p.point3D_id for p in want.images[iid].points2D]


def case_known_answers(manager):
    """The reference's own expectations (sfm/observation_manager_test.cc) through a manager class."""
    import test_obs_filter as T
    T.known_answers(manager)


def case_subsets_and_single_rules():
    """FilterPoints3D on a subset, FilterPoints3DInImages, and the two rules alone, on the class surface."""
    src = model("single")
    ids = list(src.points3D)[::3]
    for call in (lambda om: om.FilterPoints3D(4.0, MIN_TRI_ANGLE, ids + [10 ** 6]),
                 lambda om: om.FilterPoints3DInImages(4.0, MIN_TRI_ANGLE, [1, 2, 3]),
                 lambda om: om.FilterPoints3DWithLargeReprojectionError(0.004, ids, Q.NORMALIZED),
                 lambda om: om.FilterPoints3DWithSmallTriangulationAngle(MIN_TRI_ANGLE, ids),
                 lambda om: om.FilterObservationsWithNegativeDepth()):
        got, want = src.copy(), src.copy()
        assert call(OM.ObservationManager(got)) == call(Q.Manager(want))
        assert_same_model(got, want)


# ---- the GPU runs of the cases ---------------------------------------------------------------------------------------

pytestmark = pytest.mark.gpu


def test_generated_model_has_the_shapes():
    case_model_shape()


def test_edges_model_has_the_observations_it_is_named_for():
    case_edges_shape()


@pytest.mark.parametrize("error_type", [Q.PIXEL, Q.NORMALIZED, Q.ANGULAR], ids=["pixel", "normalized", "angular"])
@pytest.mark.parametrize("name", ["mixed", "single", "seam", "edges"])
def test_filter_all_points3D_matches_checker(name, error_type):
    case_filter_all(name, error_type)


def test_errors_then_angles():
    case_order_errors_then_angles()


@pytest.mark.parametrize("name", ["mixed", "single", "edges"])
def test_negative_depth_matches_checker(name):
    case_negative_depth(name)


@pytest.mark.parametrize("name", ["mixed", "seam"])
def test_short_tracks_match_checker(name):
    case_short_tracks(name)


@pytest.mark.parametrize("name", ["mixed", "single", "seam", "edges"])
def test_point_errors_match_checker(name):
    case_point_errors(name)


def test_empty_model():
    case_empty_model()


def test_input_validation():
    case_input_validation()


def test_manager_applies_deletions():
    case_manager_applies_deletions()


def test_known_answers_of_the_reference():
    case_known_answers(OM.ObservationManager)


def test_subsets_and_single_rules():
    case_subsets_and_single_rules()


def test_point_filtering_command_end_to_end(tmp_path):
    """SynthesizeDataset + SynthesizeNoise with injected outliers and low-parallax points -> `point_filtering` -> the
    output model equals the checker's: same points, tracks and point3D_ids."""
    import test_obs_filter as T
    T.command_round_trip(tmp_path, manager=None)
