"""The host side of geometric verification without a GPU: the database methods on old and new schemas, the row layout of
`two_view_geometries`, the command's options and refusals, the Python mirror of the C structures, and the numpy checker
itself -- its answers on the scenes of tests/test_two_view_geometry_gpu.py are the ones those cases expect."""
import ctypes as C
import os
import re
import sqlite3

import numpy as np
import pytest

import test_two_view_geometry_gpu as G
import two_view_reference as R
from colmap_amd import __main__ as M
from colmap_amd import database as DB
from colmap_amd import geometric_verifier as GV
from colmap_amd import two_view_geometry as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_confirms_the_scenes():
    for name, (cams, pts, truth, o, config) in G.scenes().items():
        got, mask = G.checker_answer(name)
        assert got == config, name
        if name.endswith("_outliers"):
            assert (mask >= truth).all(), name
        else:
            assert (mask == truth).all(), name


def test_checker_sample_draw_and_budget():
    for kind in G.KINDS:
        seen = set()
        for t in range(200):
            s = R.draw_sample(-1, 5, kind, t, 9)
            assert (s == R.draw_sample(0, 5, kind, t, 9)).all() and len(set(s.tolist())) == R.MIN_SAMPLES[kind]
            seen |= set(s.tolist())
        assert seen == set(range(9))
    assert R.compute_num_trials(25000, 100000, 0.999, 3.0, 1) == 73
    assert R.compute_num_trials(100, 100, 0.999, 3.0, 7) == 1
    assert R.compute_num_trials(0, 100, 0.999, 3.0, 7) == R.NO_LIMIT


def test_checker_solvers_fit_their_samples():
    for kind in (R.KIND_F, R.KIND_H):
        for p in G.solver_samples(kind)[:6]:
            for m in R.solve_minimal(kind, p):
                assert R.residuals(kind, m, p).max() < 1e-12
    pts, truth = G.scene("general", 40, 0, 3)
    F = R.estimate_f8(pts)
    assert R.residuals(R.KIND_F, F, pts).max() < 1e-16 and abs(np.linalg.det(F.reshape(3, 3))) < 1e-18
    pts, _ = G.scene("plane", 40, 0, 3)
    assert R.residuals(R.KIND_H, R.estimate_h_dlt(pts), pts).max() < 1e-12


def test_structures_match_the_header():
    """Field order and count of the ctypes mirrors against include/colmap_amd_tvg.h."""
    text = open(os.path.join(ROOT, "include", "colmap_amd_tvg.h")).read()
    for name, cls in (("tvg_camera", TV._Camera), ("tvg_ransac_options", TV._Ransac), ("tvg_options", TV._Options),
                      ("tvg_report", TV._Report)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r"\[.*\]|\*", "", f).split()[-1] for f in decl.split(",")]
        assert fields == [f[0] for f in cls._fields_], name
    assert C.sizeof(TV._Options) == C.sizeof(TV._Ransac) + 6 * 4 + 5 * 8
    values = dict(re.findall(r"TVG_CONFIG_(\w+) = (-?\d+)", text))
    assert int(values["UNCALIBRATED"]) == TV.UNCALIBRATED == 3 and int(values["PLANAR_OR_PANORAMIC"]) == TV.PLANAR_OR_PANORAMIC == 6
    assert int(values["WATERMARK"]) == TV.WATERMARK == 7 and int(values["MULTIPLE"]) == TV.MULTIPLE == 8
    assert int(values["DEGENERATE"]) == TV.DEGENERATE == 1 and int(values["NOT_BUILT"]) == TV.NOT_BUILT


def test_database_methods(tmp_path):
    path = str(tmp_path / "d.db")
    with DB.Database(path, create=True) as db:
        db.create_verification_tables()
        db.con.execute("INSERT INTO cameras VALUES (7, 2, 640, 480, ?, 1)", (np.array([500.0, 320, 240, 0.1]).tobytes(),))
        db.write_image("a.jpg", 7, 1)
        db.write_image("b.jpg", 7, 2)
        kp = np.arange(30, dtype=np.float32).reshape(5, 6)
        db.con.execute("INSERT INTO keypoints VALUES (1, 5, 6, ?)", (kp.tobytes(),))
        db.con.execute("INSERT INTO keypoints VALUES (2, 0, 4, NULL)")
        cams = db.read_cameras()
        assert list(cams) == [7] and cams[7]["model"] == 2 and cams[7]["prior_focal_length"] is True
        assert cams[7]["params"].tolist() == [500.0, 320, 240, 0.1] and (cams[7]["width"], cams[7]["height"]) == (640, 480)
        assert db.read_image_camera_ids() == {1: 7, 2: 7}
        assert (db.read_keypoints(1) == kp).all() and db.read_keypoints(2).shape == (0, 2) and db.read_keypoints(3).shape == (0, 2)
        assert db.read_matched_pair_ids() == [] and not db.exists_inlier_matches(1, 2)
        db.delete_two_view_geometry(1, 2)                      # no table yet: nothing to do
        db.write_matches(2, 1, [[0, 1]])
        assert db.read_matched_pair_ids() == [DB.image_pair_to_pair_id(1, 2)]
        F, H = np.arange(9.0).reshape(3, 3), np.arange(9.0)[::-1]
        db.write_two_view_geometry(1, 2, [[3, 4], [5, 6]], TV.UNCALIBRATED, F, H)
        assert db.exists_inlier_matches(2, 1) and db.exists_two_view_geometry(1, 2)
        with pytest.raises(sqlite3.IntegrityError):
            db.write_two_view_geometry(1, 2, [[3, 4]], TV.UNCALIBRATED)
        with pytest.raises(DB.DatabaseError, match="order of the pair id"):
            db.write_two_view_geometry(2, 1, [[3, 4]], TV.UNCALIBRATED, F)
    con = sqlite3.connect(path)
    cols = [r[1] for r in con.execute("PRAGMA table_info(two_view_geometries)")]
    assert cols == ["pair_id", "rows", "cols", "data", "config", "F", "E", "H", "qvec", "tvec", "camera1", "camera2"]
    row = con.execute("SELECT * FROM two_view_geometries").fetchone()
    assert row[:3] == (DB.image_pair_to_pair_id(1, 2), 2, 2) and row[4] == 3
    assert np.frombuffer(row[3], np.uint32).tolist() == [3, 4, 5, 6]
    assert np.frombuffer(row[5], np.float64).tolist() == list(range(9)) and np.frombuffer(row[7], np.float64).tolist() == list(range(9))[::-1]
    assert row[6] is None and row[8:] == (None, None, None, None)
    con.close()
    with DB.Database(path) as db:
        db.delete_two_view_geometry(2, 1)
        assert not db.exists_two_view_geometry(1, 2)
        db.write_two_view_geometry(2, 1, [[9, 8]], TV.UNDEFINED)   # swapped: stored in pair-id order
        db.write_two_view_geometry(1, 3, np.zeros((0, 2)), TV.UNDEFINED)
        assert not db.exists_inlier_matches(1, 3) and db.exists_two_view_geometry(1, 3)
    con = sqlite3.connect(path)
    rows = con.execute("SELECT rows, cols, data, config, F, H FROM two_view_geometries ORDER BY pair_id").fetchall()
    assert np.frombuffer(rows[0][2], np.uint32).tolist() == [8, 9] and rows[0][3:] == (0, None, None)
    assert rows[1] == (0, 2, None, 0, None, None)
    con.close()


def test_older_schema(tmp_path):
    """A two_view_geometries table from before qvec / tvec / camera1 / camera2: only its columns are written."""
    path = str(tmp_path / "old.db")
    with DB.Database(path, create=True) as db:
        db.con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY NOT NULL, rows INTEGER NOT NULL, "
                       "cols INTEGER NOT NULL, data BLOB, config INTEGER NOT NULL, F BLOB, E BLOB, H BLOB)")
        db.write_two_view_geometry(1, 2, [[1, 2]], TV.PLANAR_OR_PANORAMIC, None, np.eye(3))
        assert db.exists_inlier_matches(1, 2)
        assert db._columns("two_view_geometries") == ["pair_id", "rows", "cols", "data", "config", "F", "E", "H"]
        row = db.con.execute("SELECT config, F, E, H FROM two_view_geometries").fetchone()
        assert row[0] == 6 and row[1] is None and row[2] is None and np.frombuffer(row[3], np.float64).tolist() == np.eye(3).ravel().tolist()
    bad = str(tmp_path / "bad.db")
    with DB.Database(bad, create=True) as db:
        db.create_verification_tables()
        db.con.execute("INSERT INTO keypoints VALUES (1, 2, 3, ?)", (np.zeros(6, np.float32).tobytes(),))
        db.con.execute("INSERT INTO keypoints VALUES (2, 2, 4, ?)", (np.zeros(6, np.float32).tobytes(),))
        with pytest.raises(DB.DatabaseError, match="3 columns"):
            db.read_keypoints(1)
        with pytest.raises(DB.DatabaseError, match="blob"):
            db.read_keypoints(2)


def test_option_parsing():
    a = GV.build_parser().parse_args(["--database_path", "x"])
    o = GV.geometry_options(a)
    assert o == TV.TwoViewGeometryOptions() and GV.refusal(a) == ""
    assert (o.ransac_options.max_error, o.ransac_options.confidence, o.ransac_options.max_num_trials,
            o.ransac_options.min_inlier_ratio, o.ransac_options.min_num_trials, o.min_num_inliers) == (4.0, 0.999, 10000, 0.25, 100, 15)
    a = GV.build_parser().parse_args(["--database_path", "x", "--TwoViewGeometry.max_error", "2.5", "--TwoViewGeometry.multiple_models",
                                      "1", "--TwoViewGeometry.max_num_trials", "50", "--TwoViewGeometry.detect_watermark", "0",
                                      "--TwoViewGeometry.filter_stationary_matches", "1", "--TwoViewGeometry.random_seed", "9",
                                      "--num_threads", "4", "--batch_size", "3"])
    o = GV.geometry_options(a)
    assert o.ransac_options.max_error == 2.5 and o.multiple_models and not o.detect_watermark and o.filter_stationary_matches
    assert o.ransac_options.max_num_trials == 50 and o.ransac_options.min_num_trials == 50 and o.ransac_options.random_seed == 9
    assert a.batch_size == 3 and a.num_threads == 4
    c = o.c()
    assert c.ransac.max_error == 2.5 and c.multiple_models == 1 and c.detect_watermark == 0 and c.ransac.random_seed == 9
    for flag, word in (("--TwoViewGeometry.use_degensac", "use_degensac"), ("--TwoViewGeometry.compute_relative_pose", "compute_relative_pose"),
                       ("--FeatureMatching.rig_verification", "rig_verification"), ("--FeatureMatching.guided_matching", "guided_matching")):
        why = GV.refusal(GV.build_parser().parse_args(["--database_path", "x", flag, "1"]))
        assert word in why and "not built" in why
    assert "geometric_verifier" in M.COMMANDS


def test_command_refuses_before_it_opens_anything(tmp_path, capsys):
    assert M.main(["geometric_verifier", "--database_path", str(tmp_path / "none.db"), "--TwoViewGeometry.use_degensac", "1"]) == 1
    assert "use_degensac is not built" in capsys.readouterr().err
    assert M.main(["geometric_verifier", "--database_path", str(tmp_path / "none.db")]) == 1
    assert "does not exist" in capsys.readouterr().err


def test_camera_classification():
    pinhole = [m for m in range(18) if TV.CameraInfo(m, 1, 1).is_perspective_pinhole()]
    fisheye = [m for m in range(18) if TV.CameraInfo(m, 1, 1).is_perspective_fisheye()]
    spherical = [m for m in range(18) if TV.CameraInfo(m, 1, 1).is_spherical()]
    assert fisheye == [5, 8, 9, 10, 11, 14, 15] and spherical == [17]
    assert sorted(pinhole + fisheye + spherical) == list(range(18))
