"""Bundle-adjustment covariance on the GPU (include/colmap_amd_ba_covariance.h) against the independent restatement of
tests/ba_cov_reference.py (checker Jacobians, numpy / scipy Schur complements).

The reference's seven parameterisations (covariance_test.cc:41-326: one rig, one camera, 7 frames, 200 points,
0.01 px noise, three constant points as the gauge) are compared entry by entry within 1e-8 absolute, the reference's own
tolerance. The case functions are shared with tests/test_ba_covariance_emul.py, which runs them through the CPU
stand-in build of the same sources."""
import numpy as np
import pytest

import ba_cov_reference as R
from colmap_amd import estimators as est
from colmap_amd import scene

P = est.BACovarianceOptions.Params
MODES = {P.ALL: R.ALL, P.POSES: R.POSES, P.POINTS: R.POINTS, P.POSES_AND_POINTS: R.POSES_AND_POINTS}
# (params, fixed_points, fixed_poses, fixed_intrinsics): covariance_test.cc:291-326
REFERENCE_CASES = [
    (P.ALL, False, False, False),
    (P.ALL, True, False, False),
    (P.ALL, False, False, True),
    (P.ALL, False, True, False),
    (P.POINTS, False, False, False),
    (P.POSES, False, False, False),
    (P.POSES_AND_POINTS, False, False, False),
]


def _reference_problem(fixed_points=False, fixed_poses=False, fixed_intrinsics=False, seed=0):
    rec = scene.SynthesizeDataset(scene.SyntheticDatasetOptions(num_rigs=1, num_cameras_per_rig=1, num_frames_per_rig=7,
                                                               num_points3D=200), seed=seed)
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
    ba = est.CreateDefaultBundleAdjuster(est.BundleAdjustmentOptions(gpu_index="0"), config, rec)
    assert ba.Solve().IsSolutionUsable()
    return rec, ba


def _check_flat(flat, want, fp, params, atol=1e-8, rtol=0.0):
    """Every pose pair, every other block and every point of the flat result against the restatement."""
    lay = want.lay
    n_checked = 0
    if params != P.POSES:
        for j in range(len(fp.points)):
            w, g = want.point(j), flat.point(j)
            assert (w is None) == (g is None), j
            if w is not None:
                np.testing.assert_allclose(g, w, atol=atol, rtol=rtol)
                n_checked += 1
    else:
        assert all(flat.point(j) is None for j in range(len(fp.points)))
    poses = sorted(lay.pose)
    pairs = [(R.POSE, a, R.POSE, b) for a in poses for b in poses]
    if params == P.ALL:
        pairs += [(R.CAMERA, k, R.CAMERA, k) for k in lay.cam] + [(R.SENSOR, s, R.SENSOR, s) for s in lay.sens]
        pairs += [(R.POSE, a, R.CAMERA, k) for a in poses[:2] for k in lay.cam]
    got = flat.blocks(pairs)
    for pr, g in zip(pairs, got):
        w = want.block(*pr)
        if params == P.POINTS:
            w = None
        assert (w is None) == (g is None), pr
        if w is not None:
            np.testing.assert_allclose(g, w, atol=atol, rtol=rtol, err_msg=str(pr))
            n_checked += 1
    for k in range(len(fp.cams)):  # other blocks without ALL: no result
        if params != P.ALL:
            assert flat.block(R.CAMERA, k) is None
    return n_checked


def case_reference(params, fixed_points, fixed_poses, fixed_intrinsics):
    rec, ba = _reference_problem(fixed_points, fixed_poses, fixed_intrinsics)
    fp = ba.problem_
    J, lay = R.jacobian(fp)
    want = R.SchurCovariance(J, lay, MODES[params])
    assert len(lay.point) == (0 if fixed_points else 197)
    assert len(lay.pose) == (0 if fixed_poses else 7)
    cov = est.EstimateBACovariance(est.BACovarianceOptions(params=params), rec, ba)
    assert cov is not None
    assert _check_flat(cov.flat_, want, fp, params) > 0
    # the reconstruction-level queries
    for image_id, (slot, _) in fp.image_slots.items():
        g = cov.GetCamCovFromWorld(image_id)
        w = want.block(R.POSE, slot) if params != P.POINTS else None
        assert (g is None) == (w is None)
        if w is not None:
            np.testing.assert_allclose(g, w, atol=1e-8, rtol=0)
    for j, pid in enumerate(fp.point_ids):
        g = cov.GetPointCov(pid)
        w = want.point(j)
        assert (g is None) == (w is None)
        if w is not None:
            np.testing.assert_allclose(g, w, atol=1e-8, rtol=0)
    cam_id = fp.cam_ids[0]
    g = cov.GetOtherParamsCov(rec.cameras[cam_id].params)
    w = want.block(R.CAMERA, 0)
    assert (g is None) == (w is None)
    if w is not None:
        np.testing.assert_allclose(g, w, atol=1e-8, rtol=0)
    assert cov.GetOtherParamsCov(rec.cameras[cam_id].params.copy()) is None  # identity, not value
    # unknown ids
    assert cov.GetPointCov(10 ** 9) is None and cov.GetCamCovFromWorld(10 ** 9) is None
    assert cov.GetCamCrossCovFromWorld(10 ** 9, next(iter(rec.images))) is None
    if params in (P.ALL, P.POSES, P.POSES_AND_POINTS) and not fixed_poses:
        ids = sorted(fp.image_slots)
        a, b = ids[0], ids[1]
        c12 = cov.GetCam2CovFromCam1(a, rec.images[a].cam_from_world, b, rec.images[b].cam_from_world)
        full = np.zeros((12, 12))
        sa, sb = fp.image_slots[a][0], fp.image_slots[b][0]
        full[:6, :6], full[6:, 6:] = want.block(R.POSE, sa), want.block(R.POSE, sb)
        full[:6, 6:] = want.block(R.POSE, sa, R.POSE, sb)
        full[6:, :6] = full[:6, 6:].T
        np.testing.assert_allclose(c12, scene.GetCovarianceForRelativeRigid3d(rec.images[a].cam_from_world,
                                                                             rec.images[b].cam_from_world, full),
                                   atol=1e-8, rtol=0)
    cov.flat_.close()


def _gauge_free_problem():
    rec = scene.SynthesizeDataset(scene.SyntheticDatasetOptions(num_rigs=1, num_cameras_per_rig=1, num_frames_per_rig=5,
                                                               num_points3D=60), seed=2)
    scene.SynthesizeNoise(scene.SyntheticNoiseOptions(point2D_stddev=0.01), rec)
    config = est.BundleAdjustmentConfig()
    for image_id in rec.images:
        config.AddImage(image_id)
    return est.CreateDefaultBundleAdjuster(est.BundleAdjustmentOptions(gpu_index="0"), config, rec), rec


def case_not_estimable():
    """No gauge at all (seven-dimensional similarity ambiguity): "no result", with the column count and the rank."""
    ba, rec = _gauge_free_problem()
    for params in (P.ALL, P.POSES):
        assert est.EstimateBACovariance(est.BACovarianceOptions(params=params), rec, ba) is None
        assert "Number of columns" in est.last_covariance_message and "rank" in est.last_covariance_message
    # points alone are conditioned on the poses: still estimable
    cov = est.EstimateBACovariance(est.BACovarianceOptions(params=P.POINTS), rec, ba)
    assert cov is not None and cov.GetPointCov(next(iter(rec.points3D))) is not None


def _flat_problem(frames, points, track, seed, mixed=False, pp=False):
    d = scene.synthesize_flat(frames, points, track, seed=seed, mixed_models=mixed)
    fp = est.FlatProblem.from_arrays(d, refine_pp=pp)
    est.fix_gauge_three_points(fp)
    return fp


def case_flat(fp, params=P.ALL, loss=(0, 1.0), atol=None, rtol=0.0, so_kw=None):
    so = est.SolverOptions(loss_type=loss[0], loss_scale=loss[1], **(so_kw or {}))
    J, lay = R.jacobian(fp, loss[0], loss[1])
    want = R.SchurCovariance(J, lay, MODES[params])
    flat = est.estimate_covariance_flat(fp, est.BACovarianceOptions(params=params), so, gpu_index=0)
    assert flat is not None
    try:
        assert _check_flat(flat, want, fp, params, atol=1e-8 if atol is None else atol, rtol=rtol) > 0
        return flat.timing()
    finally:
        flat.close()


def case_crossing_panels():
    """n_c > 256 with an unaligned others block (48 intrinsics blocks of width 2: 96 other columns padded to 128): the
    pose part starts inside an outer panel of the factorisation and spans several 64-blocks."""
    fp = _flat_problem(48, 150, 8, seed=5, mixed=True)
    assert est.num_camera_parameters(fp) > 256
    est.solve_flat(fp, est.SolverOptions(linear_solver_type=est.SOLVER_DENSE_SCHUR), gpu_index=0)
    t = case_flat(fp, P.ALL, rtol=1e-9, atol=1e-9)
    assert t["n"] == 128 + 48 * 6 and t["n_inverted"] == t["n"]
    case_flat(fp, P.POSES, rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("params,fixed_points,fixed_poses,fixed_intrinsics", REFERENCE_CASES)
def test_reference_parameterisations(params, fixed_points, fixed_poses, fixed_intrinsics):
    case_reference(params, fixed_points, fixed_poses, fixed_intrinsics)


@pytest.mark.gpu
def test_not_estimable():
    case_not_estimable()


@pytest.mark.gpu
def test_crossing_panels():
    case_crossing_panels()


def _mixed_models_problem():
    fp = _flat_problem(120, 900, 6, seed=11, mixed=True)
    for k in range(1, len(fp.cams), 2):  # PINHOLE (f, f, cx, cy) -> OPENCV with zero distortion, refined
        assert fp.cam_model[k] == scene.PINHOLE
        fp.cam_model[k] = scene.OPENCV
        fp.cam_const[k, scene.MODEL_EXTRA_IDXS[scene.OPENCV]] = 0
    assert est.num_camera_parameters(fp) > 700
    return fp


def case_conditioned(fp, params):
    """Every pose pair (and every other block with ALL) against the restatement, within a bound derived from the
    conditioning of the matrix the device factors. The device forms the Jacobi-scaled S_s = D S D (D = diag(s),
    s = 1 / (1 + column norm), as the solver scales) in 64-bit fixed point (exact to 2^-60 per term, below fp64
    rounding), factors and inverts it in fp64, and returns D S_s^-1 D. A backward-stable Cholesky inverse carries a
    normwise error of at most c n eps cond(S_s) ||S_s^-1||; entry (a, b) of the unscaled result then differs by at most
    s_a s_b times that. c = 4 covers the factorisation, the triangular inverse and the product X^T X."""
    J, lay = R.jacobian(fp)
    want = R.SchurCovariance(J, lay, MODES[params])
    m = want.S.shape[0]
    s = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(axis=0)).ravel()[:m]))
    Ss = want.S * s[:, None] * s[None, :]
    cond = np.linalg.cond(Ss)
    assert cond < 1e9, cond  # the bound below is meaningful (well below 1 / eps)
    bound = 4.0 * m * np.finfo(float).eps * cond * np.linalg.norm(np.linalg.inv(Ss), 2)
    flat = est.estimate_covariance_flat(fp, est.BACovarianceOptions(params=params), gpu_index=0)
    assert flat is not None
    try:
        poses = sorted(lay.pose)
        pairs = [(R.POSE, a, R.POSE, b) for a in poses for b in poses]
        if params == P.ALL:
            pairs += [(R.CAMERA, k, R.CAMERA, k) for k in lay.cam]
        for pr, g in zip(pairs, flat.blocks(pairs)):
            (oa, sa), (ob, sb) = lay.block(pr[0], pr[1]), lay.block(pr[2], pr[3])
            tol = bound * np.outer(s[oa:oa + len(sa)], s[ob:ob + len(sb)])
            w = want.block(*pr)
            assert g is not None and g.shape == w.shape, pr
            assert np.all(np.abs(g - w) <= tol), (pr, float(np.max(np.abs(g - w) / tol)))
        return cond
    finally:
        flat.close()


@pytest.mark.gpu
def test_mixed_models_large():
    """OPENCV + SIMPLE_RADIAL, 120 images, > 700 camera-side columns, against the numpy Schur restatement, within the
    bound the conditioning of the factored matrix gives (case_conditioned); points within 1e-8 absolute."""
    fp = _mixed_models_problem()
    est.solve_flat(fp, est.SolverOptions(linear_solver_type=est.SOLVER_DENSE_SCHUR), gpu_index=0)
    case_conditioned(fp, P.ALL)
    case_conditioned(fp, P.POSES_AND_POINTS)
    J, lay = R.jacobian(fp)
    want = R.SchurCovariance(J, lay, R.POINTS)
    flat = est.estimate_covariance_flat(fp, est.BACovarianceOptions(params=P.POINTS), gpu_index=0)
    try:
        for j in lay.point:
            np.testing.assert_allclose(flat.point(j), want.point(j), atol=1e-8, rtol=0)
    finally:
        flat.close()


@pytest.mark.gpu
@pytest.mark.parametrize("loss", [(est.LossFunctionType.CAUCHY, 0.5), (est.LossFunctionType.HUBER, 1.0)])
def test_robust_loss(loss):
    fp = _flat_problem(8, 80, 4, seed=3)
    rng = np.random.default_rng(0)
    fp.obs_xy += rng.normal(0, 1.0, fp.obs_xy.shape)  # residuals beyond the loss scale: the correction matters
    case_flat(fp, P.ALL, loss=(int(loss[0]), loss[1]), atol=1e-8, rtol=1e-9)


def _prior_problem():
    fp = _flat_problem(8, 80, 4, seed=4)
    fp.point_const[:] = 0  # the priors own the gauge
    n = len(fp.poses)
    rng = np.random.default_rng(1)
    centres = np.array([-scene.quat_to_rot(p[:4]).T @ p[4:] for p in fp.poses])
    fp.prior_pose = np.arange(n, dtype=np.int32)
    fp.prior_sensor = np.full(n, -1, np.int32)
    fp.prior_position = np.ascontiguousarray(centres + rng.normal(0, 0.01, (n, 3)))
    fp.prior_sqrt_info = np.ascontiguousarray(np.tile(np.eye(3) / 0.05, (n, 1, 1)))
    fp.prior_loss_type, fp.prior_loss_scale = int(est.LossFunctionType.CAUCHY), 1.0
    return fp


@pytest.mark.gpu
def test_pose_priors():
    case_flat(_prior_problem(), P.ALL, atol=1e-8, rtol=1e-9)
    case_flat(_prior_problem(), P.POSES, atol=1e-8, rtol=1e-9)


def _sensor_problem():
    rec = scene.SynthesizeDataset(scene.SyntheticDatasetOptions(num_rigs=1, num_cameras_per_rig=2, num_frames_per_rig=4,
                                                               num_points3D=60), seed=6)
    scene.SynthesizeNoise(scene.SyntheticNoiseOptions(point2D_stddev=0.01), rec)
    config = est.BundleAdjustmentConfig()
    for image_id in rec.images:
        config.AddImage(image_id)
    for k, pid in enumerate(rec.points3D):
        if k < 3:
            config.AddConstantPoint(pid)
    ba = est.CreateDefaultBundleAdjuster(est.BundleAdjustmentOptions(gpu_index="0", refine_sensor_from_rig=True),
                                         config, rec)
    ba.Solve()
    return rec, ba


@pytest.mark.gpu
def test_variable_sensor_from_rig():
    rec, ba = _sensor_problem()
    fp = ba.problem_
    assert fp.sensor_const is not None and not fp.sensor_const.all()
    case_flat(fp, P.ALL, atol=1e-8, rtol=1e-9)
    case_flat(fp, P.POSES, atol=1e-8, rtol=1e-9)
    with pytest.raises(ValueError, match="reference sensor"):  # THROW_CHECK(image.IsRefInFrame())
        est.EstimateBACovariance(est.BACovarianceOptions(), rec, ba)


@pytest.mark.gpu
def test_bitwise_determinism_and_read_only():
    fp = _flat_problem(12, 120, 5, seed=8, mixed=True)
    before = {k: np.array(v, copy=True) for k, v in vars(fp).items() if isinstance(v, np.ndarray)}
    res = []
    for _ in range(2):
        flat = est.estimate_covariance_flat(fp, est.BACovarianceOptions(), gpu_index=0)
        pairs = [(R.POSE, a, R.POSE, b) for a in range(len(fp.poses)) for b in range(len(fp.poses))]
        res.append((flat.blocks(pairs), [flat.point(j) for j in range(len(fp.points))]))
        flat.close()
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert (a is None and b is None) or np.array_equal(a, b)
    for k, v in before.items():
        assert np.array_equal(v, getattr(fp, k)), k
