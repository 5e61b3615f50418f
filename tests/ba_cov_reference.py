"""Independent restatement of the bundle-adjustment covariance (reference estimators/covariance.cc) for the tests.

TEST INFRASTRUCTURE ONLY. The tangent-space Jacobian of a flat problem is assembled from the checker's per-observation
Jacobians (oracle/ba_oracle.py: reproj_error, rig_reproj_error*, position_prior, loss), mapped through the quaternion
manifold's PlusJacobian, the SubsetManifold masks (pose_fixed_t, cam_const) and Ceres' loss correction -- the Jacobian
ceres::Problem::Evaluate returns. From it:
  * points: (E_p^T E_p + damping I)^-1;
  * poses / others: S = H_aa - H_ap H_pp^-1 H_pa (damped point blocks), inverted (ALL) or with the others eliminated
    first (S_cc - S_co (S_oo + damping I)^-1 S_oc), in numpy / scipy.sparse.
`dense_covariance` is (J^T J)^-1 itself: the ceres::Covariance semantics the reference's test compares against.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import ba_oracle

POSE, CAMERA, SENSOR = 0, 1, 2
POSES, POINTS, POSES_AND_POINTS, ALL = 0, 1, 2, 3


def quat_plus_jacobian(q: np.ndarray) -> np.ndarray:
    """d Plus(q, delta) / d delta at delta = 0 (4 x 3) of ceres::EigenQuaternionManifold, xyzw storage:
    Plus(q, d) = [sin(|d|) d/|d|, cos(|d|)] (x) q (left multiplication; Ceres does not halve the angle)."""
    x, y, z, w = q
    return np.array([[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]])


def pose_manifold_jacobian(q: np.ndarray) -> np.ndarray:
    """7 x 6: Rigid3d params (quaternion, translation) per tangent [rotation, translation]."""
    M = np.zeros((7, 6))
    M[:4, :3] = quat_plus_jacobian(q)
    M[4:, 3:] = np.eye(3)
    return M


def pose_tangent_columns(pf: int) -> list:
    """Tangent coordinates of a pose block that the SubsetManifold keeps (ba_problem.pose_fixed_t)."""
    cols = [] if pf >= 4 else [0, 1, 2]
    held = (pf & 3) if pf >= 0 else 3
    return cols + [3 + k for k in range(3) if k != held]


def _correct(r, J, loss_type, scale, use=None):
    """ceres::internal::Corrector on a residual block."""
    if loss_type == 0:
        return J
    s = float(r @ r)
    rho = ba_oracle.loss(loss_type, scale, s, use=use)
    sqrt_rho1 = np.sqrt(rho[1])
    if s == 0.0 or rho[2] <= 0.0:
        return sqrt_rho1 * J
    alpha = 1.0 - np.sqrt(1.0 + 2.0 * s * rho[2] / rho[1])
    return sqrt_rho1 * (J - (alpha / s) * np.outer(r, r @ J))


def _correct_residual(r, loss_type, scale, use=None):
    """ceres::internal::Corrector::CorrectResiduals."""
    if loss_type == 0:
        return r
    s = float(r @ r)
    rho = ba_oracle.loss(loss_type, scale, s, use=use)
    sqrt_rho1 = np.sqrt(rho[1])
    if s == 0.0 or rho[2] <= 0.0:
        return sqrt_rho1 * r
    alpha = 1.0 - np.sqrt(1.0 + 2.0 * s * rho[2] / rho[1])
    return (sqrt_rho1 / (1.0 - alpha)) * r


class Layout:
    """Columns of the variable blocks: poses, cameras, sensors (the camera side, `n_a` columns), then points."""

    def __init__(self, fp):
        n_obs = len(fp.obs_pose)
        P = len(fp.poses)
        pose_const = np.asarray(fp.pose_const) != 0
        cam_var = [np.flatnonzero(np.asarray(fp.cam_const[k])[: ba_oracle.NUM_PARAMS[int(fp.cam_model[k])]] == 0)
                   for k in range(len(fp.cams))]
        pt_const = np.asarray(fp.point_const) != 0
        has_s = fp.sensors is not None and fp.obs_sensor is not None
        sens_var = (np.zeros(0, bool) if not has_s else
                    (np.zeros(len(fp.sensors), bool) if fp.sensor_const is None else np.asarray(fp.sensor_const) == 0))
        self.active = []
        used_p, used_c, used_x, used_s = set(), set(), set(), set()
        for o in range(n_obs):
            pi, ci, xi = int(fp.obs_pose[o]), int(fp.obs_cam[o]), int(fp.obs_point[o])
            si = int(fp.obs_sensor[o]) if has_s else -1
            sv = si >= 0 and sens_var[si]
            if pose_const[pi] and len(cam_var[ci]) == 0 and pt_const[xi] and not sv:
                continue
            self.active.append(o)
            used_p.add(pi); used_c.add(ci); used_x.add(xi)
            if sv:
                used_s.add(si)
        self.cam_var = cam_var
        self.sens_var = sens_var
        self.pose = {}
        self.cam = {}
        self.sens = {}
        self.point = {}
        off = 0
        for i in range(P):
            if not pose_const[i] and i in used_p:
                cols = pose_tangent_columns(int(fp.pose_fixed_t[i]))
                self.pose[i] = (off, cols)
                off += len(cols)
        self.n_pose = off
        for k in range(len(fp.cams)):
            if len(cam_var[k]) and k in used_c:
                self.cam[k] = (off, cam_var[k])
                off += len(cam_var[k])
        for s in range(len(sens_var)):
            if sens_var[s] and s in used_s:
                self.sens[s] = (off, list(range(6)))
                off += 6
        self.n_a = off
        for j in range(len(fp.points)):
            if not pt_const[j] and j in used_x:
                self.point[j] = (off, [0, 1, 2])
                off += 3
        self.n = off

    def block(self, kind, index):
        d = {POSE: self.pose, CAMERA: self.cam, SENSOR: self.sens}[kind]
        return d.get(index)


def jacobian(fp, loss_type=0, loss_scale=1.0, use=None, residuals=False):
    """Sparse tangent-space Jacobian (rows: active observations x 2, then priors x 3) and its Layout. `use`: the checker
    build that evaluates the observations (ba_oracle.lib() by default, ba_oracle.lib_fast() for a noise floor);
    `residuals`: also return the loss-corrected residual vector of the same rows and, per residual block (observations,
    then priors), the squared norm of its uncorrected residual (what the loss is evaluated at)."""
    lay = Layout(fp)
    rows, cols, vals = [], [], []
    res, sq = [], []   # corrected residuals; squared norm of every block's uncorrected (weighted) residual
    row = 0

    for o in lay.active:
        pi, ci, xi = int(fp.obs_pose[o]), int(fp.obs_cam[o]), int(fp.obs_point[o])
        si = int(fp.obs_sensor[o]) if fp.obs_sensor is not None else -1
        m = int(fp.cam_model[ci])
        P = ba_oracle.NUM_PARAMS[m]
        prm = fp.cams[ci][:P]
        Js = None
        if si >= 0 and lay.sens_var[si]:
            r, Jpt, Jpose, Jpar, Js = ba_oracle.rig_reproj_error_sensor(m, fp.points[xi], fp.poses[pi], fp.sensors[si], prm,
                                                                        fp.obs_xy[o], use=use)
        elif si >= 0:
            r, Jpt, Jpose, Jpar = ba_oracle.rig_reproj_error(m, fp.points[xi], fp.poses[pi], fp.sensors[si], prm, fp.obs_xy[o], use=use)
        else:
            r, Jpt, Jpose, Jpar = ba_oracle.reproj_error(m, fp.points[xi], fp.poses[pi], prm, fp.obs_xy[o], use=use)
        blocks = []  # (first column, 2 x k tangent Jacobian)
        if pi in lay.pose:
            off, sel = lay.pose[pi]
            blocks.append((off, (Jpose @ pose_manifold_jacobian(fp.poses[pi][:4]))[:, sel]))
        if ci in lay.cam:
            off, sel = lay.cam[ci]
            blocks.append((off, Jpar[:, sel]))
        if Js is not None and si in lay.sens:
            blocks.append((lay.sens[si][0], Js @ pose_manifold_jacobian(fp.sensors[si][:4])))
        if xi in lay.point:
            blocks.append((lay.point[xi][0], Jpt))
        Jall = np.concatenate([b for _, b in blocks], axis=1)
        Jall = _correct(r, Jall, loss_type, loss_scale, use)
        res.append(_correct_residual(r, loss_type, loss_scale, use))
        sq.append(float(r @ r))
        c0 = 0
        for off, b in blocks:
            k = b.shape[1]
            for a in range(2):
                rows += [row + a] * k
                cols += list(range(off, off + k))
                vals += list(Jall[a, c0:c0 + k])
            c0 += k
        row += 2
    nq = 0 if fp.prior_pose is None else len(fp.prior_pose)
    for q in range(nq):
        pi = int(fp.prior_pose[q])
        si = int(fp.prior_sensor[q]) if fp.prior_sensor is not None else -1
        if pi not in lay.pose and si not in lay.sens:
            continue
        r, Jp, Js = ba_oracle.position_prior(fp.prior_position[q], fp.poses[pi], fp.sensors[si] if si >= 0 else None, use=use)
        A = np.asarray(fp.prior_sqrt_info[q])
        r = A @ r
        blocks = []
        if pi in lay.pose:
            off, sel = lay.pose[pi]
            blocks.append((off, (A @ Jp @ pose_manifold_jacobian(fp.poses[pi][:4]))[:, sel]))
        if si >= 0 and si in lay.sens:
            blocks.append((lay.sens[si][0], A @ Js @ pose_manifold_jacobian(fp.sensors[si][:4])))
        Jall = _correct(r, np.concatenate([b for _, b in blocks], axis=1), int(fp.prior_loss_type), float(fp.prior_loss_scale), use)
        res.append(_correct_residual(r, int(fp.prior_loss_type), float(fp.prior_loss_scale), use))
        sq.append(float(r @ r))
        c0 = 0
        for off, b in blocks:
            k = b.shape[1]
            for a in range(3):
                rows += [row + a] * k
                cols += list(range(off, off + k))
                vals += list(Jall[a, c0:c0 + k])
            c0 += k
        row += 3
    J = sp.csr_matrix((vals, (rows, cols)), shape=(row, lay.n))
    if residuals:
        return J, lay, (np.concatenate(res) if res else np.zeros(0)), np.array(sq)
    return J, lay


class SchurCovariance:
    """covariance.cc restated: point covariances and the pose / other covariances of a tangent Jacobian."""

    def __init__(self, J, lay: Layout, params=ALL, damping=1e-8):
        self.lay = lay
        self.params = params
        H = (J.T @ J).tocsr()
        na = lay.n_a
        self.points = {}
        npt = lay.n - na
        Hpp = H[na:, na:].toarray() if npt <= 3 else None
        blocks = []
        for j, (off, _) in lay.point.items():
            b = (H[off:off + 3, off:off + 3].toarray() if Hpp is None else Hpp[off - na:off - na + 3, off - na:off - na + 3])
            inv = np.linalg.inv(b + damping * np.eye(3))
            blocks.append((off - na, inv))
            if params != POSES:
                self.points[j] = inv
        self.S = None
        self.estimable = True
        if params == POINTS:
            return
        Haa = H[:na, :na].toarray()
        if npt > 0:
            Hpp_inv = sp.block_diag([b for _, b in sorted(blocks, key=lambda t: t[0])], format="csr")
            Hap = H[:na, na:]
            Haa = Haa - (Hap @ Hpp_inv @ Hap.T).toarray()
        npd = lay.n_pose
        if params == ALL:
            S = Haa
        else:
            Soo = Haa[npd:, npd:] + damping * np.eye(na - npd)
            S = Haa[:npd, :npd] - Haa[:npd, npd:] @ np.linalg.solve(Soo, Haa[npd:, :npd])
        self.S = S
        d = _ldl_pivots(S)
        self.rank = int(np.count_nonzero(np.abs(d) > 1e-6))
        self.cols = S.shape[0]
        self.estimable = self.rank == self.cols
        self.cov = np.linalg.inv(S) if self.estimable and S.size else np.zeros_like(S)

    def point(self, j):
        return self.points.get(j)

    def block(self, ka, ia, kb=None, ib=None):
        if kb is None:
            kb, ib = ka, ia
        if self.S is None or not self.estimable:
            return None
        if self.params != ALL and (ka != POSE or kb != POSE):
            return None
        a, b = self.lay.block(ka, ia), self.lay.block(kb, ib)
        if a is None or b is None:
            return None
        return self.cov[a[0]:a[0] + len(a[1]), b[0]:b[0] + len(b[1])]


def _ldl_pivots(S):
    """Pivots of an unpivoted LDL^T (the Cholesky factor's squared diagonal)."""
    A = np.array(S, dtype=np.float64, copy=True)
    n = A.shape[0]
    d = np.zeros(n)
    for k in range(n):
        d[k] = A[k, k]
        if not d[k] > 0.0:  # not positive definite: the rest is not factored
            d[k:] = 0.0
            break
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:]) / d[k]
    return d


def dense_covariance(J):
    """(J^T J)^-1 over every variable block (ceres::Covariance of the whole problem)."""
    H = (J.T @ J).toarray()
    return np.linalg.inv(H)
