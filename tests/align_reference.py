"""The checker of model alignment: a sequential numpy restatement of the reference's estimators/alignment.cc:43-181,
371-398, optim/loransac.h:131-393, optim/ransac.h:167-210 and optim/support_measurement.cc:36-61 on
colmap_amd.scene.Reconstruction. One hypothesis at a time, one image after the other, one point2D_idx after the other;
none of the layouts, batches or reductions of colmap_amd/csrc/{align_plan.h,model_align.hip}. Projection goes through the
numpy camera checker of tests/obs_reference.py. The sample stream is the one documented for the product (64-bit LCG of
colmap_amd/estimators.py with rejection of repeats): the search is only comparable trial by trial on the same samples.

A similarity is 8 doubles: scale, qw qx qy qz, tx ty tz (Sim3d::ToFile)."""
import types

import numpy as np

import obs_reference as Q
from colmap_amd import estimators, scene

DBL_MAX = np.finfo(np.float64).max
SIZE_MAX = 2 ** 64 - 1
MIN_NUM_SAMPLES = 3


# ----------------------------------------------------------------------------------------------------------------------
# similarities
# ----------------------------------------------------------------------------------------------------------------------

def sim_rotation(sim):
    w, x, y, z = np.asarray(sim[1:5], np.float64) / np.linalg.norm(sim[1:5])
    return scene.quat_to_rot(np.array([x, y, z, w]))


def sim_apply(sim, x):
    """geometry/sim3.h:120-123: scale * (R x) + t."""
    return sim[0] * (sim_rotation(sim) @ np.asarray(x, np.float64)) + np.asarray(sim[5:8], np.float64)


def sim_inverse(sim):
    """geometry/sim3.h:98-105."""
    w, x, y, z = np.asarray(sim[1:5], np.float64) / np.linalg.norm(sim[1:5])
    inv = np.array([1.0 / sim[0], w, -x, -y, -z, 0.0, 0.0, 0.0])
    inv[5:8] = (sim_rotation(inv) @ np.asarray(sim[5:8], np.float64)) / -sim[0]
    return inv


def sim_from_srt(scale, R, t):
    q = scene.rot_to_quat(R)
    return np.array([scale, q[3], q[0], q[1], q[2], t[0], t[1], t[2]], np.float64)


def sim_distance(a, b):
    """Largest difference of the 3x4 matrices [sR | t], relative to the larger matrix (a quaternion and its negative are
    the same rotation)."""
    A = np.hstack([a[0] * sim_rotation(a), np.asarray(a[5:8]).reshape(3, 1)])
    B = np.hstack([b[0] * sim_rotation(b), np.asarray(b[5:8]).reshape(3, 1)])
    return float(np.abs(A - B).max() / max(np.abs(A).max(), np.abs(B).max()))


def horn(src, tgt):
    """Least-squares similarity tgt ~ s R src + t by Horn's closed form (the quaternion is the dominant eigenvector of
    the 4 x 4 matrix N of the cross-covariance), with the degeneracy rules of AlignToPositions
    (include/colmap_amd/bundle_adjustment.hpp). None where there is no answer."""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    n = len(src)
    if n < 3:
        return None
    ms, md = src.mean(0), tgt.mean(0)
    a, b = src - ms, tgt - md
    var = float((a * a).sum())
    if var < 1e-24:
        return None
    S = a.T @ b
    sv = np.linalg.svd(S, compute_uv=False)
    if sv[1] < 1e-12 * max(sv[0], 1e-150):
        return None
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    _, V = np.linalg.eigh(N)
    w, x, y, z = V[:, 3]
    R = scene.quat_to_rot(np.array([x, y, z, w]))
    scale = float((b * (a @ R.T)).sum() / var)
    if not (np.isfinite(scale) and scale > 0.0):
        return None
    sim = sim_from_srt(scale, R, md - scale * R @ ms)
    return sim if np.isfinite(sim).all() else None


# ----------------------------------------------------------------------------------------------------------------------
# residuals
# ----------------------------------------------------------------------------------------------------------------------

def common_image_ids(src, tgt):
    return [i for i in src.RegImageIds() if i in tgt.images]


def _moved(xyz, pose):
    """An image whose cam_from_world is `pose`, for obs_reference.squared_reprojection_error."""
    return types.SimpleNamespace(cam_from_world=np.asarray(pose, np.float64))


def observation_errors(src, tgt, sim):
    """Both CalculateSquaredReprojectionError terms of alignment.cc:141-161 for every common observation, whether the
    first passes or not: a list over the common images of arrays [n_i][2] (tgt term, src term)."""
    inv = sim_inverse(sim)
    out = []
    for i in common_image_ids(src, tgt):
        a, b = src.images[i], tgt.images[i]
        ca, cb = src.cameras[a.camera_id], tgt.cameras[b.camera_id]
        assert len(a.points2D) == len(b.points2D)
        rows = []
        for pa, pb in zip(a.points2D, b.points2D):
            if not pa.HasPoint3D() or not pb.HasPoint3D():
                continue
            e_tgt = Q.squared_reprojection_error(pb.xy, sim_apply(sim, src.points3D[pa.point3D_id].xyz), b, cb)
            e_src = Q.squared_reprojection_error(pa.xy, sim_apply(inv, tgt.points3D[pb.point3D_id].xyz), a, ca)
            rows.append((e_tgt, e_src))
        out.append(np.array(rows, np.float64).reshape(-1, 2))
    return out


def counts_from_errors(errors, max_reproj_error):
    """(inliers [I], common [I]) of alignment.cc:122-163."""
    m2 = max_reproj_error * max_reproj_error
    inliers = np.array([int((~(e[:, 0] > m2) & ~(e[:, 1] > m2)).sum()) for e in errors], np.int64)
    return inliers, np.array([len(e) for e in errors], np.int64)


def reproj_residuals(inliers, common):
    """alignment.cc:166-173."""
    r = np.ones(len(common), np.float64)
    for i, (n, c) in enumerate(zip(inliers, common)):
        if c > 0:
            neg = 1.0 - float(n) / float(c)
            r[i] = neg * neg
    return r


def position_residuals(src, tgt, sim):
    """SimilarityTransformEstimator::Residuals: |tgt - sim * src|^2."""
    d = np.asarray(tgt, np.float64) - (sim[0] * (np.asarray(src, np.float64) @ sim_rotation(sim).T) + np.asarray(sim[5:8]))
    return (d * d).sum(1)


def position_support(residuals, max_error):
    """(num_inliers, residual_sum in long double) of InlierSupportMeasurer::Evaluate."""
    inl = residuals <= max_error * max_error
    return int(inl.sum()), np.sum(residuals[inl].astype(np.longdouble)), inl


# ----------------------------------------------------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------------------------------------------------

def compute_num_trials(num_inliers, num_samples, confidence, multiplier):
    """RANSAC::ComputeNumTrials (optim/ransac.h:179-210); num_inliers - i wraps as size_t does."""
    prob_failure = 1 - confidence
    if prob_failure <= 0:
        return SIZE_MAX
    prob_inlier = 1.0
    for i in range(MIN_NUM_SAMPLES):
        prob_inlier *= float((num_inliers - i) % 2 ** 64) / float((num_samples - i) % 2 ** 64)
    prob_outlier = 1 - prob_inlier
    if prob_outlier <= 0:
        return 1
    if prob_outlier == 1.0:
        return SIZE_MAX
    return int(np.ceil(np.log(prob_failure) / np.log(prob_outlier) * multiplier))


class Samples:
    def __init__(self, seed):
        self.state = estimators._lcg(0x9E3779B97F4A7C15 ^ (seed & 0xFFFFFFFF))

    def draw(self, n):
        idx = []
        while len(idx) < MIN_NUM_SAMPLES:
            self.state = estimators._lcg(self.state)
            k = int((self.state >> 33) % n)
            if k not in idx:
                idx.append(k)
        return idx


def _evaluate(residuals, max_residual):
    n, s = 0, 0.0
    for r in residuals:
        if r <= max_residual:
            n += 1
            s += float(r)
    return n, s


def _better(left, right):
    return left[0] > right[0] or (left[0] == right[0] and left[1] < right[1])


def loransac(num_samples, estimate, residuals, max_residual, opt):
    """LORANSAC::Estimate (optim/loransac.h:131-393), serial. estimate(indices) -> model or None; residuals(model) ->
    array [num_samples]; opt has RANSACOptions' fields. Returns a dict like RANSAC::Report plus `trace`, the indices
    (0-based) of the trials that improved the best model."""
    rep = dict(success=False, num_trials=0, num_inliers=0, residual_sum=DBL_MAX, model=None, inlier_mask=None, trace=[])
    if num_samples < MIN_NUM_SAMPLES:
        return rep
    max_num_trials = min(opt.max_num_trials, compute_num_trials(int(opt.min_inlier_ratio * 100000), 100000, opt.confidence,
                                                                opt.dyn_num_trials_multiplier))
    best, best_model = (0, DBL_MAX), None
    samples = Samples(opt.random_seed)
    trial_counter, dyn_max = 0, max_num_trials
    while True:
        curr = trial_counter
        trial_counter += 1
        if curr >= max_num_trials:
            break
        model = estimate(samples.draw(num_samples))
        if model is None:
            continue
        r = residuals(model)
        support = _evaluate(r, max_residual)
        if _better(support, best):
            local_best, local_model = support, model
            if support[0] > MIN_NUM_SAMPLES:
                for _ in range(10):
                    refit = estimate([i for i in range(num_samples) if r[i] <= max_residual])
                    improved = False
                    if refit is not None:
                        r2 = residuals(refit)
                        s2 = _evaluate(r2, max_residual)
                        if _better(s2, local_best):
                            local_best, local_model, improved, r = s2, refit, True, r2
                    if not improved:
                        break
            if _better(local_best, best):
                best, best_model = local_best, local_model
                rep["trace"].append(curr)
                dyn_max = compute_num_trials(best[0], num_samples, opt.confidence, opt.dyn_num_trials_multiplier)
        if curr >= dyn_max and curr >= opt.min_num_trials:
            break
    rep["num_trials"] = trial_counter
    if best_model is None:
        return rep
    rep["num_inliers"], rep["residual_sum"], rep["model"] = best[0], best[1], best_model
    if best[0] < MIN_NUM_SAMPLES:
        return rep
    rep["success"] = True
    rep["inlier_mask"] = np.asarray(residuals(best_model)) <= max_residual
    return rep


def align_via_reprojections(src, tgt, min_inlier_observations, max_reproj_error, opt):
    """AlignReconstructionsViaReprojections (alignment.cc:301-342) with the caller's RANSACOptions (the reference sets
    min_inlier_ratio = 0.2); max_error is overwritten by 1 - min_inlier_observations as there."""
    ids = common_image_ids(src, tgt)
    a = np.array([src.ProjectionCenter(i) for i in ids]).reshape(-1, 3)
    b = np.array([tgt.ProjectionCenter(i) for i in ids]).reshape(-1, 3)

    def residuals(model):
        return reproj_residuals(*counts_from_errors(observation_errors(src, tgt, model), max_reproj_error))

    max_error = 1.0 - min_inlier_observations
    return loransac(len(ids), lambda idx: horn(a[idx], b[idx]), residuals, max_error * max_error, opt)


def estimate_sim3_robust(src, tgt, opt):
    """EstimateSim3dRobust on two point sets."""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    return loransac(len(src), lambda idx: horn(src[idx], tgt[idx]), lambda m: position_residuals(src, tgt, m),
                    opt.max_error * opt.max_error, opt)


# ----------------------------------------------------------------------------------------------------------------------
# ComputeImageAlignmentError
# ----------------------------------------------------------------------------------------------------------------------

def image_alignment_errors(src, tgt, sim):
    """alignment.cc:371-398 with rotation matrices: [(rotation error in degrees, projection-centre distance)] over the
    common images. The angle of R_a^T R_b is 2 asin(|R_a - R_b|_F / (2 sqrt 2)), well conditioned near 0."""
    out = []
    R, s, t = sim_rotation(sim), sim[0], np.asarray(sim[5:8], np.float64)
    for i in common_image_ids(src, tgt):
        pa, pb = src.images[i].cam_from_world, tgt.images[i].cam_from_world
        Ra = scene.quat_to_rot(pa[:4]) @ R.T          # TransformCameraWorld
        ta = s * pa[4:] - Ra @ t
        Rb, tb = scene.quat_to_rot(pb[:4]), pb[4:]
        angle = 2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra.T - Rb.T) / (2.0 * np.sqrt(2.0))))
        out.append((float(np.rad2deg(angle)), float(np.linalg.norm(-Ra.T @ ta + Rb.T @ tb))))
    return out
