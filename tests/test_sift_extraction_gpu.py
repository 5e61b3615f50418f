"""SIFT extraction on the GPU (colmap_amd/csrc/sift.hip behind colmap_amd/feature_extraction.py) against the numpy checker
tests/sift_reference.py and against what VLFeat itself gave (tests/golden/sift_vlfeat.npz): every pyramid and DoG level,
the refined detections, the orientation lists, the float descriptors and the final keypoints and descriptors, bit for
bit and row for row; independence of the handle's history and of the candidate capacity; and a database written by
`feature_extractor` that the matcher and the verifier accept. The case functions are shared with
tests/test_sift_extraction_emul.py, which runs them through the CPU build of the unmodified source.

The device keeps the reference's summation order (one accumulator per histogram bin, raster order of the window), so
the checker has one order and condition 3 of the design (device order against reference order) has nothing to record."""
import functools
import os
import sqlite3

import numpy as np
import pytest

import sift_cases as SC
import sift_reference as R
from colmap_amd import database as DB
from colmap_amd import feature_extraction as FE

CASES = SC.case_names()


def options_of(case) -> FE.SiftExtractionOptions:
    return FE.SiftExtractionOptions(**case["options"])


@functools.lru_cache(maxsize=None)
def checker(name):
    """The checker's result of a case, computed once and shared."""
    c = SC.fixture()[name]
    return R.extract(c["image"], c["options"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} against {b.shape}"
    assert a.dtype == b.dtype, f"{what}: dtype {a.dtype} against {b.dtype}"
    if not np.array_equal(bits(a), bits(b)):
        bad = np.argwhere(bits(a) != bits(b))
        raise AssertionError(f"{what}: {len(bad)} of {a.size} entries differ, first at {bad[0].tolist()}: "
                             f"{a[tuple(bad[0])]!r} against {b[tuple(bad[0])]!r}")


def device_detections(ex, k):
    d = ex.detections(k)
    return (np.stack([d["o"], d["ix"], d["iy"], d["is"]], 1).astype(np.int32).reshape(-1, 4),
            np.stack([d["x"], d["y"], d["s"], d["sigma"]], 1).astype(np.float32).reshape(-1, 4))


def extract(name, ex=None):
    c = SC.fixture()[name]
    own = ex is None
    ex = ex or FE.SiftFeatureExtractor(options_of(c))
    kp, desc = ex.extract(c["image"], options_of(c))
    out = dict(keypoints=kp, descriptors=desc, float_desc=ex.float_descriptors())
    if own:
        ex.close()
    return out


# ---- case functions -------------------------------------------------------------------------------------------------
def case_sizes():
    assert FE.conv_tile(0) == (64, 32) and FE.conv_tile(1) == (128, 8)
    assert FE.halo_limit() == 32
    assert FE.candidate_capacity(320, 240, 3) == 3600 and FE.candidate_capacity(16, 11, 3) == 1024
    assert FE.grown_capacity(1025) == 2048 and FE.grown_capacity(5) == 1024
    d = FE.default_options()
    assert (d.max_num_features, d.first_octave, d.num_octaves, d.octave_resolution) == (8192, -1, 4, 3)
    assert d.peak_threshold == 0.02 / 3.0 and d.edge_threshold == 10.0 and d.max_num_orientations == 2
    assert not d.upright and d.normalization == FE.L1_ROOT


def case_device_equals_checker(name):
    """Condition 2: device == checker at every stage."""
    device_equals(name, SC.fixture()[name], checker(name))


LAST_ROW = os.path.join(os.path.dirname(SC.GOLDEN), "sift_last_row.npz")


def case_descriptor_early_return():
    """Where vl_sift_calc_keypoint_descriptor returns early -- a keypoint whose rounded row is the last row of its octave
    -- the reference keeps the descriptor of the row before; device and checker both give the row a zero descriptor
    (DESIGN.md 2.4g). Two small images that have such a keypoint (tests/golden/sift_last_row.npz: blobs on the bottom
    edge, from tests/sift_cases.py: blob_image), one in octave -1 with two orientations, one in octave 1."""
    z = np.load(LAST_ROW)
    for key, octave in (("octave_m1", 0), ("octave_1", 2)):
        c = dict(image=z[key], options=dict(SC.DEFAULTS))
        want = R.extract(c["image"], c["options"])
        oc = want["octaves"][octave]
        rows = (oc["float_desc"] == 0).all(axis=1)
        last = oc["det_f"][:, 1].astype(np.float64) / 2.0 ** oc["o"] + 0.5 >= oc["h"] - 1   # yi = (int)(y + 0.5) == h - 1
        assert rows.any() and last.any(), f"{key}: the image no longer has a keypoint on the last row"
        assert (want["descriptors"][(want["float_desc"] == 0).all(axis=1)] == 0).all()
        device_equals(key, c, want)


def device_equals(name, c, want):
    S = c["options"]["octave_resolution"]
    with FE.SiftFeatureExtractor(options_of(c)) as ex:
        kp, desc = ex.extract(c["image"])
        fd = ex.float_descriptors()
        assert ex.num_octaves() == len(want["octaves"])
        for k, oc in enumerate(want["octaves"]):
            assert ex.octave_info(k) == (oc["w"], oc["h"], oc["o"])
            for lv in range(S + 3):
                same(ex.level(k, lv), oc["levels"][lv], f"{name}: octave {k} level {lv}")
            for lv in range(S + 2):
                same(ex.dog(k, lv), oc["dog"][lv], f"{name}: octave {k} DoG level {lv}")
            assert ex.num_candidates(k) == oc["num_candidates"]
            di, df = device_detections(ex, k)
            same(di, oc["det_i"], f"{name}: octave {k} detections (o, ix, iy, is)")
            same(df, oc["det_f"], f"{name}: octave {k} detections (x, y, s, sigma)")
            counts, angles = ex.orientations(k)
            same(counts, oc["counts"], f"{name}: octave {k} orientation counts")
            same(angles, oc["angles"], f"{name}: octave {k} angles")
            if len(di):
                for p in range(S):
                    g = ex.gradient(k, p)
                    same(g[..., 0], oc["gradient"][p][0], f"{name}: octave {k} gradient modulus {p}")
                    same(g[..., 1], oc["gradient"][p][1], f"{name}: octave {k} gradient angle {p}")
    lo, hi = want["skip"], want["skip"] + want["num_out"]
    same(kp, want["keypoints"][lo:hi], f"{name}: keypoints")
    same(fd, want["float_desc"][lo:hi], f"{name}: float descriptors")
    same(desc, want["descriptors"][lo:hi], f"{name}: descriptors")


def case_device_equals_fixture(name):
    """The device against VLFeat's own results, directly."""
    c = SC.fixture()[name]
    with FE.SiftFeatureExtractor(options_of(c)) as ex:
        kp, desc = ex.extract(c["image"])
        fd = ex.float_descriptors()
        assert ex.num_octaves() == len(c["octaves"])
        for k, oc in enumerate(c["octaves"]):
            di, df = device_detections(ex, k)
            same(di, oc["det_i"], f"{name}: octave {k} detections (o, ix, iy, is)")
            same(df, oc["det_f"], f"{name}: octave {k} detections (x, y, s, sigma)")
            counts, angles = ex.orientations(k)
            same(counts, oc["counts"], f"{name}: octave {k} orientation counts")
            same(angles, oc["angles"], f"{name}: octave {k} angles")
    lo, hi = c["skip"], c["skip"] + c["num_out"]
    all_fd = np.concatenate([oc["float_desc"] for oc in c["octaves"]]).reshape(-1, 128)
    same(kp, c["keypoints"][lo:hi], f"{name}: keypoints")
    same(fd, all_fd[lo:hi], f"{name}: float descriptors")
    same(desc, c["descriptors"][lo:hi], f"{name}: descriptors")


def case_independence():
    """Condition 4: the same bytes alone, after a larger and after a smaller image on the same handle, and with a
    candidate capacity so small that the detection of every octave with candidates reruns."""
    alone = extract("blobs96")
    c = SC.fixture()["blobs96"]
    with FE.SiftFeatureExtractor(options_of(c)) as ex:
        extract("blobs160", ex)
        after_larger = extract("blobs96", ex)
        extract("odd67", ex)
        extract("res2", ex)   # other options on the same handle
        after_smaller = extract("blobs96", ex)
        assert ex.num_reruns() == 0
        ex.set_candidate_capacity(4)
        small_capacity = extract("blobs96", ex)
        assert ex.num_reruns() >= 3, "the overflow path did not run"
        ex.set_candidate_capacity(0)
    for other, what in ((after_larger, "after a larger image"), (after_smaller, "after a smaller image"),
                        (small_capacity, "with a candidate capacity of 4")):
        for key in ("keypoints", "descriptors", "float_desc"):
            same(other[key], alone[key], f"blobs96 {what}: {key}")


def case_validation():
    img = SC.fixture()["odd67"]["image"]
    with pytest.raises(FE.FeatureExtractionError, match="octave_resolution"):
        FE.SiftFeatureExtractor(FE.SiftExtractionOptions(octave_resolution=0))
    with pytest.raises(FE.FeatureExtractionError, match="first_octave"):
        FE.SiftFeatureExtractor(FE.SiftExtractionOptions(first_octave=-2))
    with FE.SiftFeatureExtractor() as ex:
        with pytest.raises(FE.FeatureExtractionError, match="grey uint8"):
            ex.extract(img.astype(np.float32))
        with pytest.raises(FE.FeatureExtractionError, match="half-width"):   # sigma 5.5: 23 taps a side fit; resolution 1 needs 45
            ex.extract(img, FE.SiftExtractionOptions(octave_resolution=1))
        kp, desc = ex.extract(img)   # the handle still works after a refusal
        assert len(kp) == SC.fixture()["odd67"]["num_out"]
        kp, desc = ex.extract(np.zeros((1, 1), np.uint8))   # no octave of at least 2 x 2 after the first
        assert kp.shape == (0, 4) and desc.shape == (0, 128)


# ---- the database round trip: feature_extractor -> exhaustive_matcher -> geometric_verifier ------------------------------
HOMOGRAPHY = np.array([[1.02 * np.cos(0.06), -1.02 * np.sin(0.06), 6.0], [1.02 * np.sin(0.06), 1.02 * np.cos(0.06), -4.0],
                       [2e-5, -1e-5, 1.0]])
VIEW_W, VIEW_H = 224, 168


def two_views():
    """Two views of one blob scene: view 2 shows at H p what view 1 shows at p (pixel centres at +0.5)."""
    rng = np.random.RandomState(11)
    n = 260
    cx, cy = rng.uniform(-20, VIEW_W + 20, n), rng.uniform(-20, VIEW_H + 20, n)
    s = rng.uniform(1.2, 4.0, n)
    a = rng.uniform(0.1, 0.35, n) * rng.choice([-1.0, 1.0], n)

    def scene(x, y):
        v = np.zeros_like(x)
        for i in range(n):
            v += a[i] * np.exp(-((x - cx[i]) ** 2 + (y - cy[i]) ** 2) / (2 * s[i] * s[i]))
        return np.clip(np.floor((0.5 + v) * 255 + 0.5), 0, 255).astype(np.uint8)

    yy, xx = np.mgrid[0:VIEW_H, 0:VIEW_W].astype(np.float64)
    xx, yy = xx + 0.5, yy + 0.5
    Hi = np.linalg.inv(HOMOGRAPHY)
    d = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
    x1, y1 = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / d, (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / d
    return scene(xx, yy), scene(x1, y1)


def case_database_round_trip(tmp_path, main):
    """main(argv) runs `python -m colmap_amd` in-process and returns (exit code, stderr)."""
    from PIL import Image as PILImage
    images = tmp_path / "images"
    images.mkdir()
    v1, v2 = two_views()
    PILImage.fromarray(v1).save(str(images / "a.png"))
    PILImage.fromarray(v2).save(str(images / "b.png"))
    db_path = str(tmp_path / "database.db")
    rc, err = main(["feature_extractor", "--database_path", db_path, "--image_path", str(images)])
    assert rc == 0, err
    with DB.Database(db_path) as db:
        names = db.read_image_names()
        assert sorted(names.values()) == ["a.png", "b.png"]
        cams = db.read_cameras()
        assert len(cams) == 2
        for c in cams.values():   # SIMPLE_RADIAL, f = 1.2 max(w, h), principal point at the centre, no prior
            assert c["model"] == 2 and (c["width"], c["height"]) == (VIEW_W, VIEW_H) and not c["prior_focal_length"]
            assert c["params"].tolist() == [1.2 * VIEW_W, VIEW_W / 2.0, VIEW_H / 2.0, 0.0]
        ids = {n: i for i, n in names.items()}
        kp = {n: db.read_keypoints(i) for n, i in ids.items()}
        for n, i in ids.items():
            assert kp[n].shape[1] == 6 and len(kp[n]) >= 60
            assert db.read_descriptors(i).shape == (len(kp[n]), 128)
        # the rows are the extractor's own
        with FE.SiftFeatureExtractor() as ex:
            k4, d = ex.extract(v1)
        same(kp["a.png"], FE.keypoints_to_affine(k4), "database keypoints of a.png")
        same(db.read_descriptors(ids["a.png"]), d, "database descriptors of a.png")
    rc, err = main(["exhaustive_matcher", "--database_path", db_path])
    assert rc == 0, err
    max_error = 4.0
    rc, err = main(["geometric_verifier", "--database_path", db_path, "--TwoViewGeometry.max_error", str(max_error),
                    "--TwoViewGeometry.random_seed", "0"])
    assert rc == 0, err
    con = sqlite3.connect(db_path)
    rows = con.execute("SELECT pair_id, rows, cols, data, config FROM two_view_geometries").fetchall()
    con.close()
    assert len(rows) == 1
    pid, nrows, ncols, data, config = rows[0]
    assert nrows >= 15 and ncols == 2 and config != 0
    i1, i2 = DB.pair_id_to_image_pair(pid)
    inl = np.frombuffer(data, np.uint32).reshape(nrows, 2)
    by_id = {i: kp[n] for n, i in ids.items()}
    p1, p2 = by_id[i1][inl[:, 0], :2].astype(np.float64), by_id[i2][inl[:, 1], :2].astype(np.float64)
    Hm = HOMOGRAPHY if names[i1] == "a.png" else np.linalg.inv(HOMOGRAPHY)
    q = (Hm @ np.column_stack([p1, np.ones(len(p1))]).T).T
    q = q[:, :2] / q[:, 2:]
    err_px = np.linalg.norm(q - p2, axis=1)
    assert err_px.max() <= max_error, f"an inlier is {err_px.max():.2f} px from the homography"
    # a second run skips both images and leaves the rows alone
    rc, err = main(["feature_extractor", "--database_path", db_path, "--image_path", str(images)])
    assert rc == 0, err
    with DB.Database(db_path) as db:
        assert len(db.read_image_names()) == 2 and len(db.read_cameras()) == 2
        same(db.read_keypoints(ids["a.png"]), kp["a.png"], "keypoints after the second run")


def case_scale_back(tmp_path):
    """--FeatureExtraction.max_image_size: the keypoints of the scaled-down image are scaled back (ScaleKeypoints)."""
    from PIL import Image as PILImage
    from colmap_amd import feature_extractor as FX
    from colmap_amd import pipeline
    images = tmp_path / "images"
    images.mkdir()
    big = SC.fixture()["blobs160"]["image"]
    PILImage.fromarray(big).save(str(images / "big.png"))
    db_path = str(tmp_path / "database.db")
    stats = pipeline.extract_features(db_path, str(images), max_image_size=80)
    assert stats["extracted"] == 1 and stats["skipped"] == 0
    small = FX.thumbnail(big, 80)
    assert small.shape == (60, 80)
    with FE.SiftFeatureExtractor() as ex:
        k4, d = ex.extract(small)
    want = FE.rescale_keypoints(FE.keypoints_to_affine(k4), np.float32(160) / np.float32(80), np.float32(120) / np.float32(60))
    with DB.Database(db_path) as db:
        same(db.read_keypoints(1), want, "scaled-back keypoints")
        same(db.read_descriptors(1), d, "descriptors of the scaled-down image")
        cam = db.read_cameras()[1]
        assert (cam["width"], cam["height"]) == (160, 120)   # the camera keeps the size of the file
    assert stats["features"] == len(want) > 0
    assert pipeline.extract_features(db_path, str(images), max_image_size=80) == {"extracted": 0, "skipped": 1, "features": 0}


def run_main(argv):
    import contextlib
    import io
    from colmap_amd import __main__ as M
    err = io.StringIO()
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        rc = M.main(argv)
    return rc, err.getvalue()


# ---- the GPU tests --------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


def test_sizes_and_defaults():
    case_sizes()


@pytest.mark.parametrize("name", CASES)
def test_device_equals_checker(name):
    case_device_equals_checker(name)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_vlfeat_fixture(name):
    case_device_equals_fixture(name)


def test_independence_of_history_and_capacity():
    case_independence()


def test_validation():
    case_validation()


def test_descriptor_early_return():
    case_descriptor_early_return()


def test_database_round_trip(tmp_path):
    case_database_round_trip(tmp_path, run_main)


def test_scale_back_and_skip(tmp_path):
    case_scale_back(tmp_path)
