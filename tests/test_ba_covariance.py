"""Host side of the bundle-adjustment covariance (no GPU): the independent restatement of tests/ba_cov_reference.py
against finite differences, Rigid3d covariance propagation (reference geometry/rigid3_test.cc:184-248), option and enum
plumbing, and the adapter's refusal of images that are not the reference sensor of their frame."""
import numpy as np
import pytest

import ba_cov_reference as R
import ba_oracle
from colmap_amd import estimators as est
from colmap_amd import pipeline, scene


def _random_pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.concatenate([q, rng.normal(size=3)])


def _inverse(p):
    q = np.array([-p[0], -p[1], -p[2], p[3]])
    return np.concatenate([q, -scene.quat_to_rot(q) @ p[4:]])


def test_quaternion_plus_jacobian_matches_finite_differences():
    rng = np.random.default_rng(0)
    for _ in range(5):
        q = _random_pose(rng)[:4]
        h = 1e-7
        fd = np.stack([(ba_oracle.quat_plus(q, h * e) - ba_oracle.quat_plus(q, -h * e)) / (2 * h) for e in np.eye(3)], 1)
        np.testing.assert_allclose(R.quat_plus_jacobian(q), fd, atol=1e-8)


def test_tangent_jacobian_matches_finite_differences():
    """Every column of the assembled Jacobian (poses with a held translation coordinate, intrinsics masks, points,
    Cauchy loss correction excluded: trivial loss) against central differences of the checker's residuals through
    the manifold's Plus."""
    d = scene.synthesize_flat(4, 12, 3, seed=3)
    fp = est.FlatProblem.from_arrays(d)
    est.fix_gauge_two_cams(fp)
    J, lay = R.jacobian(fp)
    J = J.toarray()

    def residuals(f):
        out = []
        for o in lay.active:
            pi, ci, xi = int(f.obs_pose[o]), int(f.obs_cam[o]), int(f.obs_point[o])
            m = int(f.cam_model[ci])
            r, *_ = ba_oracle.reproj_error(m, f.points[xi], f.poses[pi], f.cams[ci][:ba_oracle.NUM_PARAMS[m]],
                                           f.obs_xy[o], want_jac=False)
            out.append(r)
        return np.concatenate(out)

    def plus(f, col, h):
        g = f.copy()
        for i, (off, sel) in lay.pose.items():
            if off <= col < off + len(sel):
                t = np.zeros(6)
                t[sel[col - off]] = h
                g.poses[i, :4] = ba_oracle.quat_plus(g.poses[i, :4], t[:3])
                g.poses[i, 4:] += t[3:]
                return g
        for k, (off, sel) in lay.cam.items():
            if off <= col < off + len(sel):
                g.cams[k, sel[col - off]] += h
                return g
        for j, (off, _) in lay.point.items():
            if off <= col < off + 3:
                g.points[j, col - off] += h
                return g
        raise AssertionError(col)

    h = 1e-6
    assert any(len(sel) == 5 for _, sel in lay.pose.values())  # the held coordinate of the second gauge camera
    for col in range(lay.n):
        fd = (residuals(plus(fp, col, h)) - residuals(plus(fp, col, -h))) / (2 * h)
        np.testing.assert_allclose(J[:, col], fd, atol=1e-4 * max(1.0, np.abs(fd).max()), err_msg=str(col))


def test_schur_restatement_equals_the_dense_inverse():
    """With ALL, the blocks of S^-1 are blocks of (J^T J)^-1 (ceres::Covariance semantics), up to the damping."""
    d = scene.synthesize_flat(5, 30, 4, seed=1)
    fp = est.FlatProblem.from_arrays(d)
    est.fix_gauge_three_points(fp)
    J, lay = R.jacobian(fp)
    full = R.dense_covariance(J)
    sc = R.SchurCovariance(J, lay, R.ALL, damping=0.0)
    assert sc.estimable
    na = lay.n_a
    np.testing.assert_allclose(sc.cov, full[:na, :na], rtol=1e-6, atol=1e-12)
    sc_p = R.SchurCovariance(J, lay, R.POSES, damping=0.0)
    npd = lay.n_pose
    np.testing.assert_allclose(np.linalg.inv(sc_p.S), full[:npd, :npd], rtol=1e-6, atol=1e-12)


def test_relative_pose_covariance_perfect_correlation():
    rng = np.random.default_rng(1)
    world_from_a, world_from_b = _random_pose(rng), _random_pose(rng)
    A = rng.normal(size=(6, 6))
    sub = A @ A.T
    cov_w = np.block([[sub, sub], [sub, sub]])
    J0 = np.zeros((12, 12))
    J0[:6, :6] = -scene.rigid3d_adjoint_inverse(world_from_a)
    J0[6:, 6:] = -scene.rigid3d_adjoint_inverse(world_from_b)
    cov_c = J0 @ cov_w @ J0.T
    rel = scene.GetCovarianceForRelativeRigid3d(_inverse(world_from_a), _inverse(world_from_b), cov_c)
    assert np.linalg.norm(rel) < 1e-6


def test_relative_pose_covariance_left_right_consistency():
    rng = np.random.default_rng(2)
    a_from_world, b_from_world = _random_pose(rng), _random_pose(rng)
    A = rng.normal(size=(12, 12))
    covar = A @ A.T
    ours = scene.GetCovarianceForRelativeRigid3d(a_from_world, b_from_world, covar)
    J0 = np.zeros((12, 12))
    J0[:6, :6] = -scene.rigid3d_adjoint_inverse(a_from_world)
    J0[6:, 6:] = np.eye(6)
    right = J0 @ covar @ J0.T
    Jr = np.zeros((6, 12))
    Jr[:, :6] = scene.rigid3d_adjoint(b_from_world)
    Jr[:, 6:] = np.eye(6)
    np.testing.assert_allclose(ours, Jr @ right @ Jr.T, atol=1e-6)
    np.testing.assert_allclose(scene.rigid3d_adjoint(a_from_world) @ scene.rigid3d_adjoint_inverse(a_from_world),
                               np.eye(6), atol=1e-12)
    with pytest.raises(ValueError):
        scene.GetCovarianceForRelativeRigid3d(a_from_world, b_from_world, np.eye(6))


def test_options_and_enums():
    o = est.BACovarianceOptions()
    assert o.params == est.BACovarianceOptions.Params.ALL and o.damping == 1e-8
    assert [int(p) for p in est.BACovarianceParams] == [0, 1, 2, 3]  # BA_COV_POSES .. BA_COV_ALL
    assert [p.name for p in est.BACovarianceParams] == ["POSES", "POINTS", "POSES_AND_POINTS", "ALL"]
    c = est.ba_covariance_options(int(o.params), o.damping)
    assert C_sizeof(c) == 16
    assert C_sizeof(est.ba_covariance_pair()) == 16
    assert est.COV_SLOT == 256
    assert callable(pipeline.estimate_ba_covariance)


def C_sizeof(x):
    import ctypes
    return ctypes.sizeof(x)


def test_header_constants_match_the_binding():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "colmap_amd_ba_covariance.h")).read()
    for name, want in (("BA_COV_POSES", 0), ("BA_COV_POINTS", 1), ("BA_COV_POSES_AND_POINTS", 2), ("BA_COV_ALL", 3),
                       ("BA_COV_OK", est.COV_OK), ("BA_COV_ERROR", est.COV_ERROR),
                       ("BA_COV_NOT_ESTIMABLE", est.COV_NOT_ESTIMABLE), ("BA_COV_NO_RESULT", est.COV_NO_RESULT),
                       ("BA_COV_KIND_POSE", est.COV_KIND_POSE), ("BA_COV_KIND_CAMERA", est.COV_KIND_CAMERA),
                       ("BA_COV_KIND_SENSOR", est.COV_KIND_SENSOR)):
        assert re.search(rf"\b{name} = {want}\b", hdr), name
    assert re.search(r"#define BA_COV_SLOT 256\b", hdr)
    assert '#include "colmap_amd_ba.h"' in hdr


def test_non_reference_sensor_images_raise():
    """covariance.cc GetPoseParams: THROW_CHECK(image.IsRefInFrame())."""
    rec = scene.SynthesizeDataset(scene.SyntheticDatasetOptions(num_rigs=1, num_cameras_per_rig=2, num_frames_per_rig=2,
                                                               num_points3D=20))
    config = est.BundleAdjustmentConfig()
    for image_id in rec.images:
        config.AddImage(image_id)
    ba = est.BundleAdjuster(est.BundleAdjustmentOptions(), config, rec)
    assert not all(rec.IsRefInFrame(i) for i in rec.images)
    with pytest.raises(ValueError, match="reference sensor"):
        est.EstimateBACovariance(est.BACovarianceOptions(), rec, ba)
    with pytest.raises(ValueError, match="reference sensor"):
        pipeline.estimate_ba_covariance(est.BACovarianceOptions(), rec, ba)
