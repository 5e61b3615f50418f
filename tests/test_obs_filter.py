"""Observation / point filtering without a GPU: the sequential checker tests/obs_reference.py against the reference's own
expectations (sfm/observation_manager_test.cc, restated as known answers), the closed forms of the kernels' header comment
against the checker on small tracks, and the `point_filtering` command -- error paths and a file round trip -- with the
library call replaced by the checker. The same known answers and round trip run against the library in
tests/test_obs_filter_gpu.py and, through the CPU stand-in, in tests/test_obs_filter_emul.py."""
import os

import numpy as np
import pytest

import obs_reference as Q
from colmap_amd import __main__ as cli_main
from colmap_amd import bundle_adjuster as BA
from colmap_amd import point_filtering as PF
from colmap_amd import scene
from colmap_amd import workspace as W


def generate_reconstruction(num_images, camera=None):
    """GenerateReconstruction (observation_manager_test.cc:42-71): PINHOLE f = 1 on a 1 x 1 image, identity poses, ten
    observations at (0, 0) per image."""
    rec = scene.Reconstruction()
    rec.cameras[1] = camera or scene.Camera(1, scene.PINHOLE, 1, 1, np.array([1.0, 1.0, 0.5, 0.5]))
    for image_id in range(1, num_images + 1):
        img = scene.Image(image_id, 1, np.array([0.0, 0, 0, 1, 0, 0, 0]))
        img.points2D = [scene.Point2D(np.zeros(2)) for _ in range(10)]
        rec.images[image_id] = img
    return rec


def add_point(rec, xyz, track=()):
    pid = max(list(rec.points3D) + [getattr(rec, "_last_id", 0)]) + 1
    rec._last_id = pid
    rec.points3D[pid] = scene.Point3D(np.array(xyz, np.float64))
    for (im, idx) in track:
        add_observation(rec, pid, im, idx)
    return pid


def add_observation(rec, pid, im, idx):
    rec.points3D[pid].track.append((im, idx))
    rec.images[im].points2D[idx].point3D_id = pid


def known_answers(manager):
    """observation_manager_test.cc:85-410 with `manager(reconstruction)` as the ObservationManager."""
    rnd = np.random.default_rng(0).uniform(-1, 1, (8, 3))  # RandomEigenVectord<3>

    for filt in ("FilterPoints3D", "FilterPoints3DInImages", "FilterAllPoints3D"):  # :85, :271, :322
        rec = generate_reconstruction(2)
        om = manager(rec)

        def call(e, a, point_ids, image_ids=(1,)):
            if filt == "FilterPoints3D":
                return om.FilterPoints3D(e, a, point_ids)
            if filt == "FilterPoints3DInImages":
                return om.FilterPoints3DInImages(e, a, image_ids)
            return om.FilterAllPoints3D(e, a)
        p1 = add_point(rec, rnd[0], [(1, 0), (2, 0)])
        assert rec.NumPoints3D() == 1
        if filt != "FilterAllPoints3D":
            assert call(0.0, 0.0, [], []) == 0 and rec.NumPoints3D() == 1
        if filt == "FilterPoints3D":
            assert call(0.0, 0.0, [p1 + 1]) == 0 and rec.NumPoints3D() == 1
        assert call(0.0, 0.0, [p1]) == 2 and rec.NumPoints3D() == 0
        if filt == "FilterPoints3DInImages":
            p2 = add_point(rec, [-0.4, -0.5, 1], [(1, 0)])
            assert call(0.0, 0.0, None, [2]) == 0 and rec.NumPoints3D() == 1
        else:
            p2 = add_point(rec, rnd[1], [(1, 0)])
        assert call(0.0, 0.0, [p2]) == 1 and rec.NumPoints3D() == 0
        p3 = add_point(rec, [-0.5, -0.5, 1], [(1, 0), (2, 0)])
        assert call(0.0, 0.0, [p3]) == 0 and rec.NumPoints3D() == 1
        assert call(0.0, 1e-3, [p3]) == 2 and rec.NumPoints3D() == 0
        p4 = add_point(rec, [-0.6, -0.5, 1], [(1, 0), (2, 0)])
        assert call(0.1, 0.0, [p4]) == 0 and rec.NumPoints3D() == 1
        assert call(0.09, 0.0, [p4]) == 2 and rec.NumPoints3D() == 0
        assert all(not p.HasPoint3D() for img in rec.images.values() for p in img.points2D)

    # FilterPoints3DWithLargeReprojectionErrorTypes (:137): PINHOLE f = 100, 100 x 100; (0.02, 0, 2) is 1 px, 0.01
    # normalized units, 0.57 degrees off the principal point
    rec = generate_reconstruction(2, scene.Camera(1, scene.PINHOLE, 100, 100, np.array([100.0, 100.0, 50.0, 50.0])))
    for img in rec.images.values():
        img.points2D = [scene.Point2D(np.array([50.0, 50.0]))]
    om = manager(rec)
    for error_type, passes, filters in ((Q.PIXEL, 1.0, 0.9), (Q.NORMALIZED, 0.01, 0.009), (Q.ANGULAR, 0.6, 0.5)):
        pid = add_point(rec, [0.02, 0, 2], [(1, 0), (2, 0)])
        assert om.FilterPoints3DWithLargeReprojectionError(passes, [pid], error_type) == 0
        assert om.FilterPoints3DWithLargeReprojectionError(filters, [pid], error_type) == 2
        assert pid not in rec.points3D

    # FilterPoints3DSphericalSeam (:215): the back direction, seen at the x = 0 side of the seam
    rec = generate_reconstruction(2, scene.Camera(1, scene.EQUIRECTANGULAR, 1000, 500, np.array([1000.0, 500.0])))
    for img in rec.images.values():
        img.points2D = [scene.Point2D(np.array([0.0, 250.0]))]
    pid = add_point(rec, [0, 0, -2], [(1, 0), (2, 0)])
    assert manager(rec).FilterPoints3DWithLargeReprojectionError(1.0, [pid], Q.PIXEL) == 0 and pid in rec.points3D

    # FilterPoints3DWithShortTracks (:356)
    rec = generate_reconstruction(4)
    om = manager(rec)
    add_point(rec, rnd[2], [(1, 0)])
    add_point(rec, rnd[3], [(1, 1), (2, 1)])
    add_point(rec, rnd[4], [(1, 2), (2, 2), (3, 2)])
    assert rec.NumPoints3D() == 3
    assert om.FilterPoints3DWithShortTracks(2) == 1 and rec.NumPoints3D() == 2
    assert om.FilterPoints3DWithShortTracks(3) == 2 and rec.NumPoints3D() == 1
    assert om.FilterPoints3DWithShortTracks(4) == 3 and rec.NumPoints3D() == 0

    # FilterObservationsWithNegativeDepth (:388)
    rec = generate_reconstruction(2)
    om = manager(rec)
    pid = add_point(rec, [0, 0, 1])
    for z in (1.0, 0.001, 0.0):
        rec.points3D[pid].xyz[2] = z
        assert om.FilterObservationsWithNegativeDepth() == 0 and rec.NumPoints3D() == 1
    add_observation(rec, pid, 1, 0)
    rec.points3D[pid].xyz[2] = 0.001
    assert om.FilterObservationsWithNegativeDepth() == 0 and rec.NumPoints3D() == 1
    rec.points3D[pid].xyz[2] = 0.0
    assert om.FilterObservationsWithNegativeDepth() == 1 and rec.NumPoints3D() == 0


def synthetic_model_with_outliers(seed=3):
    """SynthesizeDataset + SynthesizeNoise, then outlier observations and a few low-parallax points."""
    rec = scene.SynthesizeDataset(scene.SyntheticDatasetOptions(num_rigs=3, num_frames_per_rig=4, num_points3D=120), seed=seed)
    scene.SynthesizeNoise(scene.SyntheticNoiseOptions(point2D_stddev=0.4), rec, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    for pid in sorted(rec.points3D):
        tr = rec.points3D[pid].track
        if pid % 4 == 0:      # a few outliers per track
            hit = tr[: max(1, len(tr) // 4)]
        elif pid % 11 == 0:   # nearly all of them
            hit = tr[: len(tr) - int(pid % 2)]
        elif pid % 7 == 0:    # all but two: what is left is a short track
            hit = tr[: len(tr) - 2]
        else:
            hit = []
        for (im, idx) in hit:
            p2 = rec.images[im].points2D[idx]
            ang = rng.uniform(0, 2 * np.pi)
            p2.xy = p2.xy + 50.0 * np.array([np.cos(ang), np.sin(ang)])
    centers = {im: rec.ProjectionCenter(im) for im in rec.images}
    for k in range(6):        # 3000 units away, seen by the three images that face them: angles of 0.2 degrees
        v = rng.uniform(-1, 1, 3)
        v /= np.linalg.norm(v)
        pid = max(rec.points3D) + 1
        pt = scene.Point3D(3000.0 * v)
        for im in sorted(rec.images, key=lambda i: float(centers[i] @ v))[:3]:
            img = rec.images[im]
            cam = rec.cameras[img.camera_id]
            img.points2D.append(scene.Point2D(Q.img_from_cam(cam, Q.point_in_cam(img, pt.xyz)) + 0.3, pid))
            pt.track.append((im, len(img.points2D) - 1))
        rec.points3D[pid] = pt
    return rec


def command_round_trip(tmp_path, manager):
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    W.write_model_binary(BA.sparse_model_from_reconstruction(synthetic_model_with_outliers()), str(inp))
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert PF.main(["--input_path", str(inp), "--output_path", str(out), "--min_track_len", "3"], manager=manager) == 0
    want = BA.reconstruction_from_sparse_model(W.read_sparse_model(str(inp)))
    before = len(want.points3D)
    tr = Q.Trace()
    n = Q.FilterAllPoints3D(want, 4.0, 1.5, trace=tr) + Q.FilterPoints3DWithShortTracks(want, 3, tr)
    e, a = np.array(tr.errors), np.array(tr.angles)
    assert (np.abs(e - 4.0) >= 0.04).all() and (np.abs(a - np.deg2rad(1.5)) >= 0.01 * np.deg2rad(1.5)).all()
    statuses = set(tr.status.values())
    assert {Q.DELETED_ERROR, Q.DELETED_ANGLE, Q.DELETED_SHORT} <= statuses and 0 < len(want.points3D) < before
    assert f"Filtered observations: {n}" in buf.getvalue()
    got = W.read_sparse_model(str(out))
    assert sorted(got.points3D) == sorted(want.points3D)
    for pid, pt in want.points3D.items():
        assert [tuple(int(v) for v in el) for el in got.points3D[pid].track] == pt.track
        assert abs(got.points3D[pid].error - pt.error) <= 1e-6
    for iid, img in want.images.items():
        assert [int(v) for v in got.images[iid].point3D_ids] == [p.point3D_id for p in img.points2D]
        np.testing.assert_array_equal(got.images[iid].xys, np.array([p.xy for p in img.points2D]).reshape(-1, 2))


def test_checker_reproduces_the_reference_tests():
    known_answers(Q.Manager)


def test_closed_forms_agree_with_the_sequential_checker():
    """The per-point forms stated in colmap_amd/csrc/obs_filter.hip, evaluated here in Python on every mask of marked /
    negative observations of tracks up to length 6, against the deleting loops."""
    for L in range(0, 7):
        for mask in range(1 << L):
            bad = [(mask >> j) & 1 for j in range(L)]
            k = sum(bad)
            # negative depth: camera 1 looks down +z from the origin, camera 2 is the same pose turned around
            rec = generate_reconstruction(0)
            for j in range(L):
                pose = np.array([0.0, 1.0, 0, 0, 0, 0, 0]) if bad[j] else np.array([0.0, 0, 0, 1, 0, 0, 0])
                rec.images[j + 1] = scene.Image(j + 1, 1, pose, [scene.Point2D(np.zeros(2))])
            pid = add_point(rec, [0.1, 0.2, 3.0], [(j + 1, 0) for j in range(L)])
            n = Q.FilterObservationsWithNegativeDepth(rec)
            limit = max(L - 1, 1)
            assert n == min(k, limit) and (pid not in rec.points3D) == (k >= limit)
            if pid in rec.points3D:
                assert rec.points3D[pid].track == [(j + 1, 0) for j in range(L) if not bad[j]]
            # large error: the observation of a marked image sits 10 px from the projection
            rec = generate_reconstruction(0, scene.Camera(1, scene.PINHOLE, 100, 100, np.array([100.0, 100.0, 50.0, 50.0])))
            for j in range(L):
                xy = np.array([50.0 + 100.0 * 0.1 / 3.0 + (10.0 if bad[j] else 0.5 * j), 50.0 + 100.0 * 0.2 / 3.0])
                rec.images[j + 1] = scene.Image(j + 1, 1, np.array([0.0, 0, 0, 1, 0, 0, 0]), [scene.Point2D(xy)])
            pid = add_point(rec, [0.1, 0.2, 3.0], [(j + 1, 0) for j in range(L)])
            n = Q.FilterPoints3DWithLargeReprojectionError(rec, 4.0, [pid])
            if L < 2 or k >= L - 1:
                assert n == L and pid not in rec.points3D
            else:
                assert n == k and rec.points3D[pid].track == [(j + 1, 0) for j in range(L) if not bad[j]]
                assert abs(rec.points3D[pid].error - sum(0.5 * j for j in range(L) if not bad[j]) / (L - k)) < 1e-9


def test_command_error_paths(tmp_path, capsys):
    assert PF.main(["--input_path", str(tmp_path / "missing"), "--output_path", str(tmp_path)]) == 1
    assert "`input_path` is not a directory" in capsys.readouterr().err
    assert PF.main(["--input_path", str(tmp_path), "--output_path", str(tmp_path / "missing")]) == 1
    assert "`output_path` is not a directory" in capsys.readouterr().err
    assert PF.main(["--input_path", str(tmp_path), "--output_path", str(tmp_path), "--min_track_len", "-1"]) == 1
    with pytest.raises(SystemExit):
        PF.main(["--output_path", str(tmp_path)])
    capsys.readouterr()
    assert "point_filtering" in cli_main.COMMANDS
    assert cli_main.main(["point_filtering", "--input_path", str(tmp_path / "missing"), "--output_path", str(tmp_path)]) == 1


def test_command_file_round_trip_with_the_checker(tmp_path):
    command_round_trip(tmp_path, manager=Q.Manager)


def test_library_call_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from colmap_amd import observation_manager as OM
    rec = generate_reconstruction(2)
    add_point(rec, [0, 0, 1], [(1, 0), (2, 0)])
    with pytest.raises(OM.ObservationFilterError, match="no HIP device available"):
        OM.ObservationManager(rec).FilterAllPoints3D(4.0, 1.5)
    assert os.path.exists(os.path.join(os.path.dirname(PF.__file__), "csrc", "obs_filter.hip"))
