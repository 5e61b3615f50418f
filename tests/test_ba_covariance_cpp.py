"""The C++ covariance surface (include/colmap_amd/ba_covariance.hpp) end to end: tests/cpp/test_ba_cov_host.cc, compiled
like tests/test_cpp_host.py compiles its host programs, solves the reference's covariance problem
(covariance_test.cc:41-326) through CreateDefaultBundleAdjuster and EstimateBACovariance, and writes every result. They
are compared with the independent restatement of tests/ba_cov_reference.py within the reference's 1e-8 absolute, and the
solve itself with the Python mirror (same flattening, same C ABI)."""
import os
import subprocess

import numpy as np
import pytest

import ba_cov_reference as R
import test_ba_covariance_gpu as G
import test_cpp_host
from colmap_amd import estimators as est


@pytest.fixture(scope="session")
def cov_host(tmp_path_factory):
    return test_cpp_host._compile("test_ba_cov_host", tmp_path_factory)


def test_cov_host_api(cov_host):
    r = subprocess.run([cov_host, "api"], capture_output=True, text=True)
    assert r.returncode == 0 and "api OK" in r.stdout, r.stderr


def _read(path):
    out = {}
    for ln in open(path).read().splitlines():
        t = ln.split()
        if t[0] == "none":
            return None
        key = tuple([t[0]] + [int(v) for v in t[1:3 if t[0] in ("cross", "rel") else 2]])
        k = len(key)
        rows, cols = int(t[k]), int(t[k + 1])
        out[key] = np.array(t[k + 2:], float).reshape(rows, cols)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("params,fixed_points,fixed_poses,fixed_intrinsics", G.REFERENCE_CASES)
def test_cpp_estimate_matches_restatement(cov_host, tmp_path, params, fixed_points, fixed_poses, fixed_intrinsics):
    rec, ba = G._reference_problem(fixed_points, fixed_poses, fixed_intrinsics)  # the Python mirror's solve
    rec0, ba0 = _unsolved_reference_problem(fixed_points, fixed_poses, fixed_intrinsics)
    spec, out = str(tmp_path / "spec.txt"), str(tmp_path / "cov.txt")
    test_cpp_host._write_ba_spec(spec, rec0, ba0.config_, ba0.options_)
    r = subprocess.run([cov_host, "run", spec, str(int(params)), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = _read(out)
    assert got is not None
    fp = ba.problem_
    J, lay = R.jacobian(fp)
    want = R.SchurCovariance(J, lay, G.MODES[params])
    slot = {iid: s for iid, (s, _) in fp.image_slots.items()}
    n = 0
    for iid in rec.images:
        w = want.block(R.POSE, slot[iid]) if (params != G.P.POINTS and iid in slot) else None
        g = got.get(("pose", iid))
        assert (w is None) == (g is None), iid
        if w is not None:
            np.testing.assert_allclose(g, w, atol=1e-8, rtol=0)
            n += 1
        for jid in rec.images:
            g = got.get(("cross", iid, jid))
            w = (want.block(R.POSE, slot[iid], R.POSE, slot[jid])
                 if (params != G.P.POINTS and iid in slot and jid in slot) else None)
            assert (w is None) == (g is None), (iid, jid)
            if w is not None:
                np.testing.assert_allclose(g, w, atol=1e-8, rtol=0)
    for j, pid in enumerate(fp.point_ids):
        w, g = want.point(j), got.get(("point", pid))
        assert (w is None) == (g is None), pid
        if w is not None:
            np.testing.assert_allclose(g, w, atol=1e-8, rtol=0)
            n += 1
    for k, cid in enumerate(fp.cam_ids):
        w, g = want.block(R.CAMERA, k), got.get(("camera", cid))
        assert (w is None) == (g is None), cid
        if w is not None:
            np.testing.assert_allclose(g, w, atol=1e-8, rtol=0)
    ids = sorted(rec.images)
    if ("rel", ids[0], ids[1]) in got:
        cov = est.EstimateBACovariance(est.BACovarianceOptions(params=params), rec, ba)
        np.testing.assert_allclose(got[("rel", ids[0], ids[1])],
                                   cov.GetCam2CovFromCam1(ids[0], rec.images[ids[0]].cam_from_world, ids[1],
                                                          rec.images[ids[1]].cam_from_world), atol=1e-8, rtol=0)
    assert n > 0


def _unsolved_reference_problem(fixed_points, fixed_poses, fixed_intrinsics):
    """The same reconstruction, config and options as G._reference_problem, before its solve."""
    from colmap_amd import scene
    rec = scene.SynthesizeDataset(scene.SyntheticDatasetOptions(num_rigs=1, num_cameras_per_rig=1, num_frames_per_rig=7,
                                                               num_points3D=200), seed=0)
    scene.SynthesizeNoise(scene.SyntheticNoiseOptions(point2D_stddev=0.01), rec)
    config = est.BundleAdjustmentConfig()
    for image_id, img in rec.images.items():
        config.AddImage(image_id)
        if fixed_poses:
            config.SetConstantRigFromWorldPose(img.frame_id)
        if fixed_intrinsics:
            config.SetConstantCamIntrinsics(img.camera_id)
    for k, pid in enumerate(rec.points3D):
        if k < 3 or fixed_points:
            config.AddConstantPoint(pid)
    return rec, est.BundleAdjuster(est.BundleAdjustmentOptions(gpu_index="0"), config, rec.copy())
