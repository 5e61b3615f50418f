"""The iterative tier of colmap_amd/csrc/ba_kernels.hip one step at a time: the step probe (colmap_amd/csrc/ba_probe.h)
stops the solver after every named step of its first LM iteration and returns what the step computed in the caller's
indexing; the cases below compare each result with an independent value.

The case functions are shared: tests/test_ba_steps_gpu.py runs them on the hipcc build, tests/test_ba_emul.py the small
ones on the CPU stand-in build of the same source. A case takes the loaded library (a ctypes.CDLL).

Three layers, so that no bar comes from the code under test:
 (A) the linearisation (residuals, Jacobian blocks) against the checker (tests/ba_cov_reference.jacobian over
     oracle/ba_oracle.py), entry by entry. Both sides are fp64 evaluations of the same formulas; the bar of a case is
     FLOOR_MARGIN (tests/ba_compare.py) x the largest entrywise difference between the checker and its contracted
     build (ba_oracle.lib_fast()) on that case's inputs, relative to max(|entry|, the row's largest entry x 2^-40).
 (B) every later step against np.longdouble arithmetic on the device's OWN residuals and Jacobian. Bars are
     componentwise forward bounds gamma_K x (the same expression with every factor replaced by its absolute value),
     K = the number of roundings on the longest chain into an entry; the small inverses take the normwise bound
     c_n u kappa ||X|| with the condition number computed in longdouble.
 (C) the PCG recurrence restated on the device's own Minv and rhs and the dense longdouble S.
u = 2^-53, gamma_k = k u / (1 - k u) (ba_explicit_cases.gamma)."""
import ctypes as C
import functools

import numpy as np

import ba_compare
import ba_cov_reference as R
import ba_oracle
from ba_explicit_cases import EPS, LD, gamma
from colmap_amd import estimators as est
from colmap_amd import scene
from switches import switches

U32 = 2.0 ** -24
JCOLS, POSE_COL, CAM_COL, SENS_COL, PT_COL = 31, 0, 6, 22, 28
TIER_NARROW, TIER_MAX, TIER_WIDE = 0, 1, 2


# ------------------------------------------------------------------------------------------------
# ctypes mirror of ba_probe.h (field order and types as declared there; natural alignment)
# ------------------------------------------------------------------------------------------------

_P = C.c_void_p


class ba_probe_io(C.Structure):
    _fields_ = ([("radius", C.c_double), ("num_vectors", C.c_int32), ("vec_stride", C.c_int32), ("block_cap", C.c_int32),
                 ("reserved_", C.c_int32), ("x_in", _P)] +
                [(n, _P) for n in ("pose_off", "pose_dim", "pose_moff", "cam_off", "cam_dim", "cam_moff", "sens_off",
                                   "sens_dim", "sens_moff", "pt_off", "obs_active")] +
                [("cost", C.c_double)] + [(n, _P) for n in ("res", "res_p", "J", "J32")] +
                [(n, _P) for n in ("gc", "diag_c", "scale_c", "Dc", "gp", "diag_p", "scale_p", "Dp")] +
                [(n, _P) for n in ("Craw", "Cinv", "M", "Minv", "rhs", "q_out", "x")] +
                [("pcg_iterations", C.c_int32), ("pcg_pipelined", C.c_int32), ("dp", _P), ("s_model", C.c_double),
                 ("s_newcost", C.c_double)] +
                [(n, _P) for n in ("cand_poses", "cand_cams", "cand_points", "cand_sensors")] +
                [(n, C.c_int32) for n in ("n_c", "n_p", "n_active", "moff_total", "width_tier", "kd", "bd", "plain_model",
                                          "split_linearize", "op32", "n_tiles", "n_chunks", "n_heavy", "pv_n",
                                          "rhs_pass_fused", "n_priors")] +
                [("n_paired", C.c_int64)])


assert C.sizeof(ba_probe_io) == 32 + 11 * 8 + 8 + 4 * 8 + 8 * 8 + 7 * 8 + 8 + 8 + 16 + 4 * 8 + 16 * 4 + 8

FACTS = ("n_c", "n_p", "n_active", "moff_total", "width_tier", "kd", "bd", "plain_model", "split_linearize", "op32",
         "n_tiles", "n_chunks", "n_heavy", "pv_n", "rhs_pass_fused", "n_priors", "n_paired", "pcg_iterations",
         "pcg_pipelined", "cost", "s_model", "s_newcost")


class Probe:
    """What ba_probe_steps returned: the arrays by name (numpy, caller's indexing) and the path facts as attributes."""

    def arrays(self):
        return {k: v for k, v in self.__dict__.items() if isinstance(v, np.ndarray)}


def run_probe(lib, fp, so=None, xs=None, env=None):
    """One probe run. `xs`: (k, vec_stride) camera-side vectors or None; `env`: development switches for the run."""
    so = so or est.SolverOptions(jacobi_scaling=False)
    p = est.marshal_problem(fp)
    o = est.marshal_options(so)
    nP, nK, nX, nO = len(fp.poses), len(fp.cams), len(fp.points), len(fp.obs_pose)
    nS = 0 if fp.sensors is None else len(fp.sensors)
    stride = 6 * nP + 16 * nK + 6 * nS
    cap = 36 * nP + 256 * nK + 36 * nS
    k = 0 if xs is None else len(xs)
    out = Probe()
    io = ba_probe_io()
    io.radius, io.num_vectors, io.vec_stride, io.block_cap = float(so.initial_trust_region_radius), k, stride, cap
    if k:
        xs = np.ascontiguousarray(xs, np.float64)
        assert xs.shape == (k, stride)
        io.x_in = xs.ctypes.data

    def arr(name, shape, dtype=np.float64, fill=0):
        a = np.full(shape, fill, dtype)
        setattr(out, name, a)
        setattr(io, name, a.ctypes.data)

    for kind, n in (("pose", nP), ("cam", nK), ("sens", nS)):
        for f in ("off", "dim", "moff"):
            arr(f"{kind}_{f}", max(n, 1), np.int32, -1)
    arr("pt_off", nX, np.int32, -1)
    arr("obs_active", nO, np.uint8)
    arr("res", (nO, 2)); arr("res_p", (nO, 2)); arr("J", (nO, 2, JCOLS)); arr("J32", (nO, 2, JCOLS), np.float32)
    for n in ("gc", "diag_c", "scale_c", "Dc", "rhs", "x"):
        arr(n, stride)
    for n in ("gp", "diag_p", "scale_p", "Dp", "dp"):
        arr(n, (nX, 3))
    arr("Craw", (nX, 6)); arr("Cinv", (nX, 9)); arr("M", cap); arr("Minv", cap)
    arr("q_out", (2, max(k, 1), stride))
    arr("cand_poses", (nP, 7)); arr("cand_cams", (nK, est.CAM_STRIDE)); arr("cand_points", (nX, 3))
    arr("cand_sensors", (max(nS, 1), 7))
    lib.ba_last_error.restype = C.c_char_p
    with switches(lib, **(env or {})):
        rc = lib.ba_probe_steps(C.byref(p), C.byref(o), C.c_int32(0), C.byref(io))
    if rc != 0:
        raise RuntimeError(lib.ba_last_error().decode())
    for f in FACTS:
        setattr(out, f, getattr(io, f))
    out.stride = stride
    return out


# ------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------

MODEL_PARAMS = {
    scene.SIMPLE_PINHOLE: (1280.0, 512.0, 384.0),
    scene.PINHOLE: (1280.0, 1290.0, 512.0, 384.0),
    scene.SIMPLE_RADIAL: (1280.0, 512.0, 384.0, 0.05),
    scene.RADIAL: (1280.0, 512.0, 384.0, 0.05, -0.01),
    scene.OPENCV: (1280.0, 1290.0, 512.0, 384.0, 0.05, -0.01, 0.001, -0.002),
    scene.OPENCV_FISHEYE: (900.0, 910.0, 512.0, 384.0, 0.03, -0.004, 0.001, -0.0002),
    scene.FULL_OPENCV: (900.0, 910.0, 512.0, 384.0, -0.05, 0.02, -0.001, 0.001, 0.001, 0.02, -0.02, 0.001),
    scene.FOV: (900.0, 910.0, 512.0, 384.0, 0.6),
    scene.SIMPLE_RADIAL_FISHEYE: (900.0, 512.0, 384.0, 0.03),
    scene.RADIAL_FISHEYE: (900.0, 512.0, 384.0, 0.03, -0.004),
    scene.THIN_PRISM_FISHEYE: (900.0, 910.0, 512.0, 384.0, -0.05, 0.02, -0.001, 0.001, 0.001, 0.02, -0.02, 0.001),
    scene.RAD_TAN_THIN_PRISM_FISHEYE: (900.0, 910.0, 512.0, 384.0, -0.0232, 0.0924, -0.0591, 0.003, 0.0048, -0.0009,
                                       0.0002, 0.0005, -0.0009, -0.0001, 0.00007, -0.00017),
    scene.SIMPLE_DIVISION: (900.0, 512.0, 384.0, -0.05),
    scene.DIVISION: (900.0, 910.0, 512.0, 384.0, -0.05),
    scene.SIMPLE_FISHEYE: (900.0, 512.0, 384.0),
    scene.FISHEYE: (900.0, 910.0, 512.0, 384.0),
    scene.EUCM: (900.0, 910.0, 512.0, 384.0, 0.56, 0.87),
    scene.EQUIRECTANGULAR: (1024.0, 768.0),
}
TIER_MODELS = {"plain": [scene.SIMPLE_RADIAL], "narrow": [scene.SIMPLE_RADIAL, scene.PINHOLE, scene.RADIAL],
               "kd8": [scene.OPENCV, scene.OPENCV_FISHEYE], "kd12": [scene.FULL_OPENCV],
               "kd16": [scene.RAD_TAN_THIN_PRISM_FISHEYE]}
OTHER_MODELS = [m for m in MODEL_PARAMS if m not in (scene.SIMPLE_RADIAL, scene.OPENCV, scene.OPENCV_FISHEYE,
                                                     scene.FULL_OPENCV, scene.RAD_TAN_THIN_PRISM_FISHEYE)]
assert len(OTHER_MODELS) == 13


def _flat(frames, points, track, seed, models=None, obs_cam=None, n_cams=None, noise=(0.02, 0.01, 0.5), refine_pp=False):
    """scene.synthesize_flat without noise, the cameras replaced by `models` (camera k takes models[k % len]), the
    observations re-projected through the checker, then noise (translation, point, pixel standard deviations)."""
    d = scene.synthesize_flat(frames, points, track, seed=seed, noise=None)
    rng = np.random.default_rng(seed + 1000)
    if obs_cam is not None:
        d["obs_cam"] = np.ascontiguousarray(obs_cam(d["obs_pose"]), np.int32)
        d["cams"], d["cam_model"] = d["cams"][:n_cams].copy(), d["cam_model"][:n_cams].copy()
    if models is not None:
        for k in range(len(d["cams"])):
            m = models[k % len(models)]
            d["cam_model"][k] = m
            d["cams"][k] = 0.0
            d["cams"][k, :len(MODEL_PARAMS[m])] = MODEL_PARAMS[m]
        for o in range(len(d["obs_pose"])):
            k = int(d["obs_cam"][o])
            m = int(d["cam_model"][k])
            d["obs_xy"][o] = ba_oracle.reproj_error(m, d["points"][d["obs_point"][o]], d["poses"][d["obs_pose"][o]],
                                                    d["cams"][k, :ba_oracle.NUM_PARAMS[m]], np.zeros(2), want_jac=False)[0]
    d["poses"][:, 4:] += rng.normal(0, noise[0], (len(d["poses"]), 3))
    d["points"] += rng.normal(0, noise[1], d["points"].shape)
    d["obs_xy"] += rng.normal(0, noise[2], d["obs_xy"].shape)
    return est.FlatProblem.from_arrays(d, refine_pp=refine_pp)


@functools.lru_cache(maxsize=None)
def tier_problem(kind):
    """8 images x 60 points x tracks of 4 with every kind of block: a constant pose and a 5-wide one (the two-camera
    gauge), constant points, a camera with some parameters constant and one with all of them (dimension 0); the kd-8
    tier also refines a principal point (an 8-wide block = bd)."""
    fp = _flat(8, 60, 4, seed=31 + len(kind), models=TIER_MODELS[kind])
    assert est.fix_gauge_two_cams(fp)
    fp.point_const[::7] = 1
    fp.cam_const[2, 0] = 1
    fp.cam_const[3, :] = 1
    if kind == "kd8":
        fp.cam_const[4, :8] = 0
    return fp


DIVISION_FAMILY = (scene.SIMPLE_DIVISION, scene.DIVISION)


@functools.lru_cache(maxsize=None)
def model_problem(model):
    """One of the other camera models (layer A only): 4 images x 24 points x tracks of 3. `fp.behind` = an observation
    whose point was moved behind its camera (z < 0). The DIVISION models have no cheirality test and project it; for
    them `fp.outside` = an observation outside the model's domain (w^2 - 4 rho^2 k < 0 with k > 0). EUCM's domain test
    (a non-positive denominator) is what rejects its point behind the camera."""
    fp = _flat(4, 24, 3, seed=200 + model, models=[model])
    assert est.fix_gauge_two_cams(fp)
    var = np.flatnonzero(fp.pose_const[fp.obs_pose] == 0)
    o = int(var[0])
    pose = fp.poses[fp.obs_pose[o]]
    fp.points[fp.obs_point[o]] = scene.quat_to_rot(pose[:4]).T @ (np.array([0.1, 0.1, -1.0]) - pose[4:])
    fp.behind, fp.outside = o, None
    if model in DIVISION_FAMILY:
        o2 = int(var[fp.obs_point[var] != fp.obs_point[o]][0])
        pose, k = fp.poses[fp.obs_pose[o2]], int(fp.obs_cam[o2])
        fp.cams[k, 3 if model == scene.SIMPLE_DIVISION else 4] = 0.2
        fp.points[fp.obs_point[o2]] = scene.quat_to_rot(pose[:4]).T @ (np.array([3.0, 3.0, 1.0]) - pose[4:])
        fp.outside = o2
    return fp


@functools.lru_cache(maxsize=None)
def rig_problem(variable_sensors):
    """Two rigs of three cameras, three frames each: a frame's pose block is seen through three cameras, two of them
    through a sensor_from_rig -- constant, or (refine_sensor_from_rig) a 6-wide block of its own."""
    rec = scene.SynthesizeDataset(scene.SyntheticDatasetOptions(
        num_rigs=2, num_cameras_per_rig=3, num_frames_per_rig=3, num_points3D=40, num_points2D_without_point3D=0), seed=5)
    scene.SynthesizeNoise(scene.SyntheticNoiseOptions(0.02, 0.0, 0.02, 0.5), rec, seed=6)
    if variable_sensors:
        for rig in rec.rigs.values():
            for cid in rig.sensors:
                rig.sensors[cid] = rig.sensors[cid] + np.array([0, 0, 0, 0, 0.03, -0.02, 0.01])
        rec.UpdateCamFromWorld()
    cfg = est.BundleAdjustmentConfig()
    for i in rec.RegImageIds():
        cfg.AddImage(i)
    cfg.FixGauge(est.BundleAdjustmentGauge.TWO_CAMS_FROM_WORLD)
    fp = est.flatten(est.BundleAdjustmentOptions(refine_sensor_from_rig=bool(variable_sensors)), cfg, rec)
    fp.point_const[::11] = 1
    return fp


@functools.lru_cache(maxsize=None)
def prior_problem(loss):
    """A position prior on every pose instead of a gauge, covariance weighted, with the priors' own loss (and an outlier
    for the robust one)."""
    fp = _flat(8, 60, 4, seed=3, models=[scene.SIMPLE_RADIAL])
    rng = np.random.default_rng(3)
    centres = np.stack([-scene.quat_to_rot(q[:4]).T @ q[4:] for q in fp.poses])
    fp.prior_pose = np.arange(8, dtype=np.int32)
    fp.prior_position = np.ascontiguousarray(centres + 0.05 * rng.normal(size=centres.shape))
    L = np.linalg.cholesky(np.linalg.inv(np.diag([0.01, 0.02, 0.04]) + 0.002))
    fp.prior_sqrt_info = np.ascontiguousarray(np.repeat(L.T[None], 8, 0))
    fp.prior_loss_type, fp.prior_loss_scale = int(loss), 1.5
    if int(loss) != 0:
        fp.prior_position[2] += 3.0
    fp.point_const[::7] = 1
    return fp


@functools.lru_cache(maxsize=None)
def shared_problem():
    """Three cameras shared by twelve images: pairs of observations of one point inside one intrinsics block."""
    fp = _flat(12, 60, 5, seed=71, models=[scene.SIMPLE_RADIAL], obs_cam=lambda op: op % 3, n_cams=3)
    assert est.fix_gauge_two_cams(fp)
    fp.point_const[::9] = 1
    return fp


@functools.lru_cache(maxsize=None)
def heavy_problem():
    """One camera for all images: its block has many chunks of 64 (heavy with COLMAP_AMD_BA_HEAVY_CHUNKS=1)."""
    fp = _flat(8, 80, 5, seed=11, models=[scene.SIMPLE_RADIAL], obs_cam=lambda op: 0 * op, n_cams=1)
    assert est.fix_gauge_two_cams(fp)
    return fp


@functools.lru_cache(maxsize=None)
def chunk_edge_problem():
    """Pose blocks with 1, 63, 64, 65 and 129 observations (COLMAP_AMD_BA_CHUNK=64: odd counts under the pair-consuming
    Gram kernel, exactly one and two full chunks) beside two ordinary images that carry the gauge."""
    counts = [129, 129, 1, 63, 64, 65, 129]
    fp = _flat(7, 129, 2, seed=5, models=[scene.SIMPLE_RADIAL])
    keep = []
    seen = [0] * 7
    d_pose, d_pt = [], []
    for j in range(129):       # point j is seen by every image that still needs observations
        for i in range(7):
            if seen[i] < counts[i]:
                seen[i] += 1
                d_pose.append(i); d_pt.append(j)
    fp = _retopo(fp, np.array(d_pose, np.int32), np.array(d_pt, np.int32), seed=6)
    assert est.fix_gauge_two_cams(fp)
    assert np.bincount(fp.obs_pose).tolist() == counts
    return fp


def _retopo(fp, obs_pose, obs_point, seed):
    """The same cameras, poses and points with another observation list (re-projected by the checker + 0.5 px)."""
    rng = np.random.default_rng(seed)
    fp = fp.copy()
    fp.obs_pose, fp.obs_point = np.ascontiguousarray(obs_pose, np.int32), np.ascontiguousarray(obs_point, np.int32)
    fp.obs_cam = fp.obs_pose.copy()
    xy = np.zeros((len(obs_pose), 2))
    for o in range(len(obs_pose)):
        k = int(fp.obs_cam[o])
        m = int(fp.cam_model[k])
        xy[o] = ba_oracle.reproj_error(m, fp.points[obs_point[o]], fp.poses[obs_pose[o]],
                                       fp.cams[k, :ba_oracle.NUM_PARAMS[m]], np.zeros(2), want_jac=False)[0]
    fp.obs_xy = np.ascontiguousarray(xy + rng.normal(0, 0.5, xy.shape))
    return fp


@functools.lru_cache(maxsize=None)
def tile_problem(kind):
    """"pts": 300 points with tracks of 2 (a tile closes on TILE_PTS = 256); "obs511" / "obs512" / "obs513": points
    whose tracks sum to that many observations before a long one (the tile closes on TILE_OBS = 512, at, on and past
    its end); "track512" / "track513": one track of exactly 512 (tiled) / 513 observations (untiled kernels)."""
    if kind == "pts":
        fp = _flat(6, 300, 2, seed=3, models=[scene.SIMPLE_RADIAL])
    else:
        tracks = {"obs511": [255, 256, 40, 3], "obs512": [256, 256, 40, 3], "obs513": [256, 257, 40, 3],
                  "track512": [512, 3, 2], "track513": [513, 3, 2]}[kind]
        # (eight images: an image observes a long track's point many times -- valid input, and n_c stays small)
        base = _flat(8, len(tracks), 2, seed=17, models=[scene.SIMPLE_RADIAL], noise=(0.02, 0.01, 0.0))
        obs_pose = np.concatenate([np.arange(t) % 8 for t in tracks])
        obs_point = np.concatenate([np.full(t, j) for j, t in enumerate(tracks)])
        fp = _retopo(base, obs_pose, obs_point, seed=18)
    assert est.fix_gauge_two_cams(fp)
    return fp


@functools.lru_cache(maxsize=None)
def degenerate_problem(kind):
    fp = _flat(6, 40, 4, seed=13, models=[scene.SIMPLE_RADIAL])
    if kind == "points_only":
        fp.pose_const[:] = 1
        fp.cam_const[:] = 1
    else:
        assert est.fix_gauge_two_cams(fp)
        fp.point_const[:] = 1
    return fp


# ------------------------------------------------------------------------------------------------
# the device's linearisation as dense longdouble matrices (through the probe's maps only)
# ------------------------------------------------------------------------------------------------

class Dense:
    """J = [Jc | E] (scaled as stored) and r of the active observations in caller order, in longdouble; `rows_of_pt[j]`
    = the rows of point j. Also asserts what the probe's layout promises: unused columns are zero, the blocks of an
    inactive observation are zero, both copies of the residuals agree."""

    def __init__(self, fp, P):
        act = np.flatnonzero(P.obs_active)
        assert len(act) == P.n_active
        inactive = np.flatnonzero(P.obs_active == 0)
        assert not P.J[inactive].any() and not P.res[inactive].any()
        assert np.array_equal(P.res, P.res_p), "c-order and p-order residuals differ"
        self.act = act
        nr = 2 * len(act)
        self.Jc = np.zeros((nr, P.n_c), LD)
        self.E = np.zeros((nr, P.n_p), LD)
        self.r = P.res[act].reshape(-1).astype(LD)
        self.rows_of_pt = {}
        has_s = fp.obs_sensor is not None and fp.sensors is not None
        for row, o in enumerate(act):
            blk = P.J[o]
            used = np.zeros(JCOLS, bool)
            rr = slice(2 * row, 2 * row + 2)
            for kind, idx, col in (("pose", fp.obs_pose[o], POSE_COL), ("cam", fp.obs_cam[o], CAM_COL),
                                   ("sens", fp.obs_sensor[o] if has_s else -1, SENS_COL)):
                if idx < 0:
                    continue
                off, dim = int(getattr(P, kind + "_off")[idx]), int(getattr(P, kind + "_dim")[idx])
                if off >= 0:
                    self.Jc[rr, off:off + dim] = blk[:, col:col + dim]
                    used[col:col + dim] = True
            j = int(fp.obs_point[o])
            if P.pt_off[j] >= 0:
                self.E[rr, P.pt_off[j]:P.pt_off[j] + 3] = blk[:, PT_COL:PT_COL + 3]
                used[PT_COL:PT_COL + 3] = True
                self.rows_of_pt.setdefault(j, []).extend([2 * row, 2 * row + 1])
            assert not blk[:, ~used].any(), f"observation {o}: a column outside its blocks is not zero"


def _inverse_bar(A):
    """(X, bar, ||X||_F): the longdouble inverse of a small SPD block and the bound on |X_fp64 - X| of an fp64 inversion
    by elimination (cofactors for 3 x 3, Gauss-Jordan with partial pivoting): column j of the computed inverse solves
    (A + dA_j) x_j = e_j with ||dA_j|| <= gamma_{3n} || |L||U| || (Higham, Accuracy and Stability, Thm 9.4), and
    || |L||U| ||_F <= n ||A||_F for a positive definite A (no growth); so ||dx_j|| <= 3 n^2 u kappa ||x_j|| to first order and
    every entry of X_fp64 - X is below 3 n^2 u kappa_F(A) ||X||_F. kappa_F = ||A||_F ||X||_F >= kappa_2, in longdouble."""
    n = A.shape[0]
    X = np.linalg.inv(A.astype(np.float64)).astype(LD)
    for _ in range(4):                      # Newton-Schulz in longdouble from the fp64 inverse
        X = X + X @ (np.eye(n, dtype=LD) - A @ X)
    nA, nX = np.sqrt((A * A).sum()), np.sqrt((X * X).sum())
    return X, float(3 * n * n * EPS * nA * nX * nX), nX


class Reference:
    """Everything after the linearisation from the device's own r and J, in longdouble, with its bars."""

    def __init__(self, fp, P, so):
        D = self.D = Dense(fp, P)
        self.P = P
        n_c, nX = P.n_c, len(fp.points)
        # what the checker's rows (position priors) may differ by from the device's: FLOOR_MARGIN x the floor between
        # the two checker builds + 16 roundings of evaluating a prior's Jacobian; an expression with f such factors
        # carries f x that on top of its gamma_K
        self.prior_eps = 0.0
        if P.n_priors:
            c = checker(fp, so.loss_type, so.loss_scale)
            assert c.J.shape[0] - c.n_rows == 3 * P.n_priors
            self.prior_eps = ba_compare.FLOOR_MARGIN * c.floor_prior + 16 * EPS
            Jq = c.J[c.n_rows:, :n_c].astype(LD) * P.scale_c[:n_c].astype(LD)   # stored columns are column-scaled
            D.Jc = np.concatenate([D.Jc, Jq])
            D.E = np.concatenate([D.E, np.zeros((len(Jq), P.n_p), LD)])
            D.r = np.concatenate([D.r, c.r[c.n_rows:].astype(LD)])
        Jc, E, r = D.Jc, D.E, D.r
        pe2, pe4 = 2 * self.prior_eps, 4 * self.prior_eps
        aJc, aE, ar = np.abs(Jc), np.abs(E), np.abs(r)
        nnz_c = (Jc != 0).sum(0)
        # g = J^T r, column norms^2: k = the non-zero terms of the column
        self.gc, self.gc_bar = Jc.T @ r, (_g(nnz_c) + pe2) * (aJc.T @ ar)
        self.diag_c, self.diag_c_bar = (Jc * Jc).sum(0), (_g(nnz_c) + pe2) * (aJc * aJc).sum(0)
        lo, hi, rad = LD(so.min_lm_diagonal), LD(so.max_lm_diagonal), LD(so.initial_trust_region_radius)
        # ba_lm_diag_kernel: D = sqrt(min(max(diag, lo), hi) / radius) of the device's own diag: a division and a square
        # root, each correctly rounded -> 2 u relative (3 u asked)
        self.lm = lambda diag: np.sqrt(np.minimum(np.maximum(diag.astype(LD), lo), hi) / rad)
        self.Dc2 = P.Dc[:n_c].astype(LD) ** 2
        self.gp = np.zeros((nX, 3), LD); self.gp_bar = np.zeros((nX, 3))
        self.diag_p = np.zeros((nX, 3), LD); self.diag_p_bar = np.zeros((nX, 3))
        self.Craw = np.zeros((nX, 3, 3), LD); self.Craw_bar = np.zeros((nX, 3, 3))
        self.Cinv = np.zeros((nX, 3, 3), LD); self.Cinv_bar = np.zeros(nX)
        S = Jc.T @ Jc + np.diag(self.Dc2)
        Sabs = aJc.T @ aJc + np.diag(self.Dc2)       # |Jc|^T |Jc| + Dc^2
        S2abs = np.zeros((n_c, n_c), LD)             # sum_j |W_j| |Cinv_j| |W_j|^T, |W_j| = |Jc_j|^T |E_j|
        Serr = np.zeros((n_c, n_c), LD)              # sum_j |W_j| dCinv_j |W_j|^T: what the fp64 Cinv may differ by
        rhs, rhs_abs, rhs_err = self.gc.copy(), aJc.T @ ar, np.zeros(n_c, LD)
        self.W, self.Wabs = {}, {}
        self.max_track = 1
        ones = np.ones((3, 3), LD)
        for j, rows in D.rows_of_pt.items():
            off = int(P.pt_off[j])
            Ej, rj = E[rows, off:off + 3], r[rows]
            k = _g(len(rows))
            self.max_track = max(self.max_track, len(rows) // 2)
            self.gp[j], self.gp_bar[j] = Ej.T @ rj, k * (np.abs(Ej).T @ np.abs(rj))
            self.diag_p[j], self.diag_p_bar[j] = (Ej * Ej).sum(0), k * (Ej * Ej).sum(0)
            self.Craw[j], self.Craw_bar[j] = Ej.T @ Ej, k * (np.abs(Ej).T @ np.abs(Ej))
            C = self.Craw[j] + np.diag(P.Dp[j].astype(LD) ** 2)
            X, bar, nX = _inverse_bar(C)
            # + the device inverts ITS C, whose entries are fp64 sums of 2 t products plus Dp^2: |dC| <= gamma_{2t+2}
            # (|E|^T |E| + Dp^2) entrywise, and dX = -X dC X to first order: ||dX||_F <= ||X||_F^2 ||dC||_F
            dC = gamma(len(rows) + 2) * (np.abs(Ej).T @ np.abs(Ej) + np.diag(P.Dp[j].astype(LD) ** 2))
            bar += float(nX * nX * np.sqrt((dC * dC).sum()))
            self.Cinv[j], self.Cinv_bar[j] = X, bar
            W, Wa = Jc[rows].T @ Ej, aJc[rows].T @ np.abs(Ej)
            self.W[j], self.Wabs[j] = W, Wa
            S -= W @ X @ W.T
            S2abs += Wa @ np.abs(X) @ Wa.T
            Serr += bar * (Wa @ ones @ Wa.T)
            rhs -= W @ (X @ self.gp[j])
            rhs_abs += Wa @ (np.abs(X) @ (np.abs(Ej).T @ np.abs(rj)))
            rhs_err += bar * (Wa @ (ones @ (np.abs(Ej).T @ np.abs(rj))))
        self.S, self.Sabs, self.S2abs, self.Serr = S, Sabs, S2abs, Serr
        # roundings on the longest chain of an implicit product / the right-hand side: J_c x (<= 28 terms), E^T (2 t),
        # C^-1 (3), E u and the subtraction (4), J_c^T v (the column's terms), D^2 x and the final additions (4)
        self.K = int(28 + 2 * self.max_track + 3 + 4 + (nnz_c.max() if n_c else 0) + 4)
        self.GK = gamma(self.K) + pe4
        self.rhs, self.rhs_bar = rhs, self.GK * rhs_abs + rhs_err

    def product(self, x, fp32=False):
        """S x and its bar. fp32: the operator streams columns rounded to fp32 (relative error u32 = 2^-24 each, the
        accumulation stays fp64): the J_c^T J_c x term carries two such factors, the J_c^T E C^-1 E^T J_c x term four
        (C^-1 is formed from the fp64 columns), so the exact product may differ by ((1 + u32)^2 - 1) |J_c|^T |J_c| |x| +
        ((1 + u32)^4 - 1) sum_j |W_j| |C_j^-1| |W_j|^T |x| on top of the fp64 accumulation's gamma_K term."""
        x = x.astype(LD)
        ax = np.abs(x)
        A1, A2 = (self.Sabs - np.diag(self.Dc2)) @ ax, self.S2abs @ ax
        bar = self.GK * (self.Sabs @ ax + A2) + self.Serr @ ax
        if fp32:
            bar = bar + ((1 + U32) ** 2 - 1) * A1 + ((1 + U32) ** 4 - 1) * A2
        return self.S @ x, bar

    def implicit_product_fp64(self):
        """p -> S p evaluated in fp64 the way an implicit-Schur solver must: no S, the point blocks inverted in fp64."""
        import scipy.sparse as sp
        Jc, E = self.D.Jc.astype(np.float64), sp.csr_matrix(self.D.E.astype(np.float64))
        Dp2 = _pvec(self.P, self.P.Dp) ** 2
        C = (E.T @ E + sp.diags(Dp2)).toarray() if self.P.n_p else np.zeros((0, 0))
        inv = [np.linalg.inv(C[o:o + 3, o:o + 3]) for o in range(0, self.P.n_p, 3)]
        Ci = sp.block_diag(inv, format="csr") if inv else None
        Dc2 = self.Dc2.astype(np.float64)

        def apply(p):
            jx = Jc @ p
            v = jx - E @ (Ci @ (E.T @ jx)) if Ci is not None else jx
            return Jc.T @ v + Dc2 * p
        return apply

    def blocks(self, fp):
        """(moff, dim, M_b, bar_b) per camera-side block: the diagonal block of S - Dc^2, pair terms included."""
        P = self.P
        out = []
        for kind, n in (("pose", len(fp.poses)), ("cam", len(fp.cams)), ("sens", 0 if fp.sensors is None else len(fp.sensors))):
            for i in range(n):
                off, dim = int(getattr(P, kind + "_off")[i]), int(getattr(P, kind + "_dim")[i])
                if off < 0:
                    continue
                sl = slice(off, off + dim)
                nobs = int((self.D.Jc[:, sl] != 0).any(1).sum())
                pairs = max([int((self.D.Jc[rows][:, sl] != 0).any(1).sum()) // 2 for rows in self.D.rows_of_pt.values()] or [1])
                # G_o = E C^-1 E^T (3 + 3), J^T (I - G) J (2 + 2 + 1), the sum over the block's observations and, for a
                # point seen m times in the block, its m^2 cross terms
                K = 2 * nobs + 16 + pairs * pairs
                M = self.S[sl, sl] - np.diag(self.Dc2[sl])
                bar = (gamma(K) + 4 * self.prior_eps) * ((self.Sabs[sl, sl] - np.diag(self.Dc2[sl])) + self.S2abs[sl, sl]) + self.Serr[sl, sl]
                out.append((int(getattr(P, kind + "_moff")[i]), dim, off, M, bar))
        return out


def _g(k):
    return gamma(np.maximum(np.asarray(k, np.float64), 1.0))


RATIOS = {}   # step -> largest |error| / bar seen in this process (reported by the GPU test module)


def _check(step, got, want, bar, what=""):
    got, want, bar = np.asarray(got, LD), np.asarray(want, LD), np.asarray(bar, LD)
    err = np.abs(got - want)
    ok = err <= bar
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / np.where(bar > 0, bar, LD(1e-300)))
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[step] = max(RATIOS.get(step, 0.0), worst)
    assert ok.all(), f"{step} {what}: {int((~ok).sum())} of {ok.size} entries beyond their bar, worst error / bar = {worst:.3g}"


# ------------------------------------------------------------------------------------------------
# layer A
# ------------------------------------------------------------------------------------------------

def _rel_to_row(diff, ref):
    rowmax = np.abs(ref).max(axis=1, keepdims=True) if ref.ndim == 2 else np.abs(ref).max()
    return np.abs(diff) / np.maximum(np.maximum(np.abs(ref), rowmax * 2.0 ** -40), 1e-300)


class _Checked:
    pass


def robust_cost(fp, so, sq, n_obs_blocks, use=None):
    """1/2 sum rho(s) over the observation blocks (the solve's loss) and the prior blocks (the priors' own loss)."""
    total = LD(0)
    for i, v in enumerate(sq):
        lt, ls = (so.loss_type, so.loss_scale) if i < n_obs_blocks else (fp.prior_loss_type, fp.prior_loss_scale)
        total += LD(v) if int(lt) == 0 else LD(ba_oracle.loss(int(lt), float(ls), float(v), use=use)[0])
    return 0.5 * float(total)


@functools.lru_cache(maxsize=None)
def _checker(fp_key, loss_type, loss_scale):
    fp = _PROBLEMS[fp_key]
    so = est.SolverOptions(loss_type=loss_type, loss_scale=loss_scale)
    J, lay, r, sq = R.jacobian(fp, loss_type, loss_scale, residuals=True)
    Jf, _, rf, sqf = R.jacobian(fp, loss_type, loss_scale, use=ba_oracle.lib_fast(), residuals=True)
    J, Jf = J.toarray(), Jf.toarray()
    n_rows = 2 * len(lay.active)
    r2, rf2 = r[:n_rows].reshape(-1, 2), rf[:n_rows].reshape(-1, 2)
    c = _Checked()
    c.J, c.lay, c.r, c.sq, c.n_rows = J, lay, r, sq, n_rows
    c.floor_J = float(_rel_to_row(J[:n_rows] - Jf[:n_rows], J[:n_rows]).max())
    c.floor_r = float(_rel_to_row(r2 - rf2, r2).max())
    # the prior rows (3 per prior) of both builds: the floor of what the later steps take from the checker
    c.floor_prior = 0.0
    if J.shape[0] > n_rows:
        c.floor_prior = max(float(_rel_to_row(J[n_rows:] - Jf[n_rows:], J[n_rows:]).max()),
                            float(_rel_to_row((r[n_rows:] - rf[n_rows:]).reshape(-1, 3), r[n_rows:].reshape(-1, 3)).max()))
    c.cost = robust_cost(fp, so, sq, len(lay.active))
    c.cost_fast = robust_cost(fp, so, sqf, len(lay.active), use=ba_oracle.lib_fast())
    return c


_PROBLEMS = {}


def checker(fp, loss_type=0, loss_scale=1.0):
    """The checker's Jacobian, layout and residuals of a problem, and the floors of the comparison (cached per problem)."""
    _PROBLEMS[id(fp)] = fp
    return _checker(id(fp), int(loss_type), float(loss_scale))


def check_layout(fp, P, lay):
    """The probe's maps against the independent Layout of tests/ba_cov_reference.py."""
    assert np.flatnonzero(P.obs_active).tolist() == lay.active
    for kind, d, n in (("pose", lay.pose, len(fp.poses)), ("cam", lay.cam, len(fp.cams)),
                       ("sens", lay.sens, 0 if fp.sensors is None else len(fp.sensors))):
        for i in range(n):
            want = d.get(i)
            assert int(getattr(P, kind + "_off")[i]) == (want[0] if want else -1), (kind, i)
            assert int(getattr(P, kind + "_dim")[i]) == (len(want[1]) if want else -1), (kind, i)
    for j in range(len(fp.points)):
        assert int(P.pt_off[j]) == (lay.point[j][0] - lay.n_a if j in lay.point else -1)
    assert P.n_c == lay.n_a and P.n_p == lay.n - lay.n_a


def check_linearisation(fp, P, so, verbose=False):
    """(A): the maps, the residuals and the unscaled Jacobian blocks against the checker, entry by entry; the cost
    1/2 sum rho(s) (observations under the solve's loss, priors under their own) against the checker's."""
    c = checker(fp, so.loss_type, so.loss_scale)
    J, lay, r, n_rows = c.J, c.lay, c.r, c.n_rows
    check_layout(fp, P, lay)
    D = Dense(fp, P)
    scale = np.concatenate([P.scale_c[:P.n_c], _pvec(P, P.scale_p)])
    Jdev = (np.concatenate([D.Jc, D.E], axis=1) / scale.astype(LD)).astype(np.float64)
    dJ = _rel_to_row(Jdev - J[:n_rows], J[:n_rows])
    rdev = D.r.astype(np.float64).reshape(-1, 2)
    dr = _rel_to_row(rdev - r[:n_rows].reshape(-1, 2), r[:n_rows].reshape(-1, 2))
    bar_J, bar_r = ba_compare.FLOOR_MARGIN * c.floor_J, ba_compare.FLOOR_MARGIN * c.floor_r
    if verbose:
        print(f"layer A: J {float(dJ.max()):.3e} (bar {bar_J:.3e})  r {float(dr.max()):.3e} (bar {bar_r:.3e})")
    for step, d, bar in (("linearise J", dJ, bar_J), ("linearise r", dr, bar_r)):
        worst = float(d.max())
        RATIOS[step] = max(RATIOS.get(step, 0.0), worst / bar if bar > 0 else (0.0 if worst == 0 else np.inf))
        assert worst <= bar, f"{step}: {worst:.3e} beyond {ba_compare.FLOOR_MARGIN} x the checker's floor = {bar:.3e}"
    _check("cost", P.cost, c.cost, cost_bar(c, bar_r))
    return D


def cost_bar(c, bar_r):
    """|cost - 1/2 sum rho(s)|: rho is concave with rho' <= 1, so an error ds of s moves rho by at most ds; s = |r|^2
    carries twice the residuals' relative bar; the sum of n terms gamma_{n+2}; evaluating rho a few roundings (8 u asked);
    and the checker's own floor between its two builds."""
    half_s = 0.5 * float(np.sum(c.sq))
    return ((gamma(len(c.sq) + 2) + 2 * bar_r + 2 * ba_compare.FLOOR_MARGIN * c.floor_prior) * half_s + 8 * EPS * c.cost +
            ba_compare.FLOOR_MARGIN * abs(c.cost - c.cost_fast))


def _pvec(P, a):
    """A point-side array of the probe (per caller point) as the device's point-side vector."""
    out = np.zeros(P.n_p, a.dtype)
    for j in np.flatnonzero(P.pt_off >= 0):
        out[P.pt_off[j]:P.pt_off[j] + 3] = a[j]
    return out


# ------------------------------------------------------------------------------------------------
# layer B and C
# ------------------------------------------------------------------------------------------------

def probe_vectors(fp, k=2, seed=9):
    nS = 0 if fp.sensors is None else len(fp.sensors)
    stride = 6 * len(fp.poses) + 16 * len(fp.cams) + 6 * nS
    rng = np.random.default_rng(seed)
    xs = rng.normal(size=(k, stride))
    xs[0] = np.abs(xs[0])   # one vector without cancellation between its terms
    return xs


def pcg_restated(apply_S, Minv_blocks, rhs, max_iter, eta, dtype):
    """ba_pcg_update_kernel / ba_pcgp_*: x = 0, r = b, z = Minv r, rho = r.z (zero: no iteration); per iteration k:
    p = z (+ rho_k / rho_{k-1} p), q = S p, alpha = rho / p.q, x += alpha p, r -= alpha q, Q_k = sum -x (b + r) / 2,
    z = Minv r, rho' = r.z; it stops after iteration k when rho or p.q is not positive and finite, when
    zeta = k (Q_k - Q_{k-1}) / Q_k < eta, or at max_iter. `apply_S`: the product in `dtype`. Returns x, the count and the
    smallest |zeta - eta| / eta."""
    n = len(rhs)
    b = rhs.astype(dtype)

    def precond(r):
        z = np.zeros(n, dtype)
        for off, dim, Mi in Minv_blocks:
            z[off:off + dim] = Mi.astype(dtype) @ r[off:off + dim]
        return z

    x, r = np.zeros(n, dtype), b.copy()
    z = precond(r)
    rho = r @ z
    if rho == 0:
        return x, 0, np.inf
    p, Q0, margin, rho_last = None, dtype(0), np.inf, None
    for k in range(1, max_iter + 1):
        p = z.copy() if k == 1 else z + (rho / rho_last) * p
        q = apply_S(p)
        pq = p @ q
        alpha = rho / pq
        x, r = x + alpha * p, r - alpha * q
        Q1 = (-0.5 * x * (b + r)).sum()
        rho_last, z = rho, precond(r)
        if not (rho > 0 and np.isfinite(rho) and pq > 0 and np.isfinite(pq)):
            return x, k, margin
        zeta = k * (Q1 - Q0) / Q1
        margin = min(margin, abs(float(zeta) - eta) / eta)
        if zeta < eta:
            return x, k, margin
        Q0, rho = Q1, r @ z
    return x, max_iter, margin


def check_steps(fp, P, so, xs, expect_pipelined=True, verbose=False):
    """(B) and (C) on one probe result."""
    ref = Reference(fp, P, so)
    n_c = P.n_c
    # ---- gradient, column norms, LM diagonal
    if n_c:
        _check("gc", P.gc[:n_c], ref.gc, ref.gc_bar)
        _check("diag_c", P.diag_c[:n_c], ref.diag_c, ref.diag_c_bar)
        _check("Dc", P.Dc[:n_c], ref.lm(P.diag_c[:n_c]), 3 * EPS * ref.lm(P.diag_c[:n_c]))
    var = np.flatnonzero(P.pt_off >= 0)
    assert sorted(ref.D.rows_of_pt) == var.tolist()
    _check("gp", P.gp[var], ref.gp[var], ref.gp_bar[var])
    _check("diag_p", P.diag_p[var], ref.diag_p[var], ref.diag_p_bar[var])
    _check("Dp", P.Dp[var], ref.lm(P.diag_p[var]), 3 * EPS * ref.lm(P.diag_p[var]))
    iu = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])
    _check("Craw", P.Craw[var], ref.Craw[var][:, iu[0], iu[1]], ref.Craw_bar[var][:, iu[0], iu[1]])
    _check("Cinv", P.Cinv[var].reshape(-1, 3, 3), ref.Cinv[var], ref.Cinv_bar[var][:, None, None])
    x = P.x[:n_c].astype(LD)
    if n_c:
        # ---- Schur-Jacobi blocks
        minv_blocks = []
        for moff, dim, off, M, bar in ref.blocks(fp):
            got = P.M[moff:moff + dim * dim].reshape(dim, dim)
            _check("M", got, M, bar, f"block at {off} ({dim} wide)")
            Xi, ibar, _ = _inverse_bar(got.astype(LD) + np.diag(ref.Dc2[off:off + dim]))   # of the device's own M
            gi = P.Minv[moff:moff + dim * dim].reshape(dim, dim)
            _check("Minv", gi, Xi, ibar, f"block at {off} ({dim} wide)")
            minv_blocks.append((off, dim, gi))
        # ---- right-hand side, products
        _check("rhs", P.rhs[:n_c], ref.rhs, ref.rhs_bar)
        for i in range(len(xs)):
            want, bar = ref.product(xs[i][:n_c])
            _check("S x", P.q_out[0, i, :n_c], want, bar, f"vector {i}")
            if P.op32:
                want, bar = ref.product(xs[i][:n_c], fp32=True)
                _check("S x (fp32 operator)", P.q_out[1, i, :n_c], want, bar, f"vector {i}")
                assert not np.array_equal(P.q_out[1, i, :n_c], P.q_out[0, i, :n_c]), "the fp32 copies were not streamed"
            else:
                assert np.array_equal(P.q_out[1, i, :n_c], P.q_out[0, i, :n_c]), "inexact product differs without fp32 copies"
        # ---- (C) PCG: the recurrence on the device's Minv and rhs and the dense longdouble S
        assert P.pcg_pipelined == (1 if expect_pipelined else 0), "pcg() took the other loop"
        if not P.op32:
            # the longdouble run multiplies by the dense longdouble S; the fp64 run forms the product as an fp64 solver
            # has to, implicitly from the fp64 columns and fp64 inverses of the point blocks: q = J_c^T (J_c p - E C^-1 E^T
            # J_c p) + Dc^2 p. Their distance is what fp64 arithmetic costs this solve.
            x64, it64, m64 = pcg_restated(ref.implicit_product_fp64(), minv_blocks, P.rhs[:n_c],
                                          so.max_linear_solver_iterations, so.eta, np.float64)
            xld, itld, mld = pcg_restated(lambda v: ref.S @ v, minv_blocks, P.rhs[:n_c], so.max_linear_solver_iterations,
                                          so.eta, LD)
            assert it64 == itld and min(m64, mld) > 1e-3, ("the restatement's own count is a coin flip", it64, itld, m64, mld)
            floor = float(np.abs(x64 - xld).max())
            if verbose:
                print(f"pcg: {itld} iterations, zeta margin {min(m64, mld):.3g}, fp64 - longdouble floor {floor:.3e}")
            assert P.pcg_iterations == itld, (P.pcg_iterations, itld)
            _check("pcg x", P.x[:n_c], xld, 10 * floor)
    # ---- back-substitution dp = C^-1 (g_p - E^T J_c x) and the model change, from the device's own x
    jx = ref.D.Jc @ x if n_c else np.zeros(len(ref.D.r), LD)
    ajx = np.abs(ref.D.Jc) @ np.abs(x) if n_c else np.zeros(len(ref.D.r), LD)
    E = ref.D.E
    for j, rows in ref.D.rows_of_pt.items():
        off = int(P.pt_off[j])
        Ej = E[rows, off:off + 3]
        t, ta = ref.gp[j] - Ej.T @ jx[rows], np.abs(Ej).T @ (np.abs(ref.D.r[rows]) + ajx[rows])
        bar = ref.GK * (np.abs(ref.Cinv[j]) @ ta) + ref.Cinv_bar[j] * ta.sum()
        _check("dp", P.dp[j], ref.Cinv[j] @ t, bar, f"point {j}")
    dpv = _pvec(P, P.dp).astype(LD)
    w = jx + E @ dpv                                   # J s = -w
    wa = ajx + np.abs(E) @ np.abs(dpv)
    model = (w * (ref.D.r - w / 2)).sum()              # -(J s).(r + J s / 2)
    mbar = (gamma(len(w) + 40) + 4 * ref.prior_eps) * (wa * (np.abs(ref.D.r) + wa / 2)).sum()
    _check("model change", P.s_model, model, mbar)
    return ref


def check_candidate_cost(fp, P, so):
    """S_NEWCOST against the checker's cost at the candidate parameters (both checker builds give the floor; the
    residuals' bar is the floor of the candidate's own residuals)."""
    cand = fp.copy()
    cand.poses, cand.cams, cand.points = P.cand_poses.copy(), P.cand_cams.copy(), P.cand_points.copy()
    if fp.sensors is not None:
        cand.sensors = P.cand_sensors.copy()
    _KEEP.append(cand)
    c = checker(cand, so.loss_type, so.loss_scale)
    _check("candidate cost", P.s_newcost, c.cost, cost_bar(c, ba_compare.FLOOR_MARGIN * c.floor_r))
    # constant blocks are carried over bit for bit
    assert np.array_equal(P.cand_poses[fp.pose_const == 1], fp.poses[fp.pose_const == 1])
    assert np.array_equal(P.cand_points[fp.point_const == 1], fp.points[fp.point_const == 1])
    if fp.sensors is not None and fp.sensor_const is not None:
        assert np.array_equal(P.cand_sensors[fp.sensor_const == 1], fp.sensors[fp.sensor_const == 1])


_KEEP = []   # candidates stay alive while the checker's cache is keyed by their id


def assert_identical(P, Q):
    a, b = P.arrays(), Q.arrays()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k} differs between two runs"
    for f in FACTS:
        assert getattr(P, f) == getattr(Q, f), f


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------

def _so(**kw):
    kw.setdefault("jacobi_scaling", False)
    return est.SolverOptions(**kw)


def case_tier(lib, kind, split, plain=True, verbose=False):
    """A width tier, with every kind of block, through (A), (B) and (C); two runs are identical."""
    fp, so = tier_problem(kind), _so()
    xs = probe_vectors(fp)
    env = {"COLMAP_AMD_BA_SPLIT_LINEARIZE": int(split)}
    if not plain:
        env["COLMAP_AMD_BA_PLAIN_LINEARIZE"] = 0
    P = run_probe(lib, fp, so, xs, env)
    tier, kd, bd = {"plain": (TIER_NARROW, 4, 6), "narrow": (TIER_NARROW, 4, 6), "kd8": (TIER_MAX, 8, 8),
                    "kd12": (TIER_WIDE, 16, 16), "kd16": (TIER_WIDE, 16, 16)}[kind]
    assert (P.width_tier, P.kd, P.bd) == (tier, kd, bd)
    assert P.split_linearize == int(split)
    assert P.plain_model == (scene.SIMPLE_RADIAL if kind == "plain" and plain else -1)
    assert P.n_tiles > 0 and P.n_chunks > 0 and P.rhs_pass_fused == 1 and P.op32 == 0 and P.n_heavy == 0
    assert -1 in P.pose_dim and 5 in P.pose_dim and 6 in P.pose_dim and (P.pt_off < 0).any()
    assert P.cam_dim[3] == -1 and P.cam_dim[2] == int((fp.cam_const[2, :ba_oracle.NUM_PARAMS[int(fp.cam_model[2])]] == 0).sum()) >= 1
    if kind == "kd8":
        assert P.cam_dim.max() == 8
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)
    check_candidate_cost(fp, P, so)
    assert_identical(P, run_probe(lib, fp, so, xs, env))


def case_jacobi_scaling(lib, verbose=False):
    """jacobi_scaling = 1: scale = 1 / (1 + sqrt(diag)) of the unscaled columns, the stored blocks are scale x unscaled
    (check_linearisation divides them back), and every later step holds on the scaled system."""
    fp, so = tier_problem("narrow"), _so(jacobi_scaling=True)
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs)
    D = check_linearisation(fp, P, so, verbose)
    assert (P.scale_c[:P.n_c] < 1).all() and (P.scale_c[:P.n_c] > 0).all()
    # diag of the unscaled columns from the stored ones: (J s)^2 / s^2; s = 1 / (1 + sqrt(d)) has a square root, an
    # addition and a division (3 u), d itself gamma_k of its terms, and the stored product J s one rounding (2 u in d)
    sc = P.scale_c[:P.n_c].astype(LD)
    d0 = (D.Jc * D.Jc).sum(0) / sc ** 2
    k = (D.Jc != 0).sum(0)
    _check("scale_c", P.scale_c[:P.n_c], 1 / (1 + np.sqrt(d0)), (3 * EPS + 0.5 * (_g(k) + 4 * EPS)) / (1 + np.sqrt(d0)))
    Ep = _pvec(P, P.scale_p).astype(LD)
    d0p = (D.E * D.E).sum(0) / Ep ** 2
    kp = (D.E != 0).sum(0)
    assert (Ep < 1).all() and (Ep > 0).all()
    _check("scale_p", Ep, 1 / (1 + np.sqrt(d0p)), (3 * EPS + 0.5 * (_g(kp) + 4 * EPS)) / (1 + np.sqrt(d0p)))
    check_steps(fp, P, so, xs, verbose=verbose)


def case_model(lib, model, verbose=False):
    """One of the other 13 camera models through (A). The observation of the point behind its camera has a zero
    residual and a zero Jacobian block on the device and in the checker -- except for EQUIRECTANGULAR and the DIVISION
    models, which define a projection there: the checker's rows are not zero and (A) has compared them; the DIVISION
    models' observation outside their domain is zero on both sides."""
    fp, so = model_problem(model), _so()
    P = run_probe(lib, fp, so)
    check_linearisation(fp, P, so, verbose)
    c = checker(fp, 0, 1.0)

    def rows(o):
        row = c.lay.active.index(o)
        return c.J[2 * row:2 * row + 2], c.r[2 * row:2 * row + 2]

    rejected = [fp.behind] if model not in DIVISION_FAMILY + (scene.EQUIRECTANGULAR,) else [fp.outside]
    for o in rejected:
        if o is None:
            continue
        Jo, ro = rows(o)
        assert P.obs_active[o] and not P.res[o].any() and not P.J[o].any(), f"observation {o} is not rejected on the device"
        assert not Jo.any() and not ro.any(), f"observation {o} is not rejected by the checker"
    if model in DIVISION_FAMILY + (scene.EQUIRECTANGULAR,):
        Jo, ro = rows(fp.behind)
        assert Jo.any() and ro.any() and P.res[fp.behind].any() and P.J[fp.behind].any()
    if model in DIVISION_FAMILY:
        assert fp.outside is not None


def case_rig(lib, variable_sensors, verbose=False):
    """Rig frames with constant and with variable sensor_from_rig: the latter has Jsens, 6-wide sensor blocks in M / Minv
    and pairs of observations of one point inside one block through the rig (n_paired > 0)."""
    fp, so = rig_problem(bool(variable_sensors)), _so()
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs)
    assert fp.sensors is not None and (fp.obs_sensor >= 0).any()
    if variable_sensors:
        assert (P.sens_off >= 0).any() and (P.sens_dim[P.sens_off >= 0] == 6).all() and (P.sens_moff[P.sens_off >= 0] >= 0).all()
        assert P.n_paired > 0 and P.J[:, :, SENS_COL:SENS_COL + 6].any()
    else:
        assert (P.sens_off < 0).all() and not P.J[:, :, SENS_COL:SENS_COL + 6].any()
    assert P.plain_model == -1 and P.pcg_pipelined == 1
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)
    check_candidate_cost(fp, P, so)
    if variable_sensors:
        assert not np.array_equal(P.cand_sensors[P.sens_off >= 0], fp.sensors[P.sens_off >= 0])


def case_priors(lib, loss, verbose=False):
    """Position priors on every pose: ba_prior_* add their rows to the cost, gc, diag_c, M, the products and the model
    change, and pcg() takes the step-by-step loop. The reference takes the prior rows from the checker."""
    fp, so = prior_problem(int(loss)), _so()
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs)
    assert P.n_priors == 8 and (P.pose_off >= 0).all()
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, expect_pipelined=False, verbose=verbose)
    check_candidate_cost(fp, P, so)


def case_loss(lib, loss, scale, verbose=False):
    fp, so = tier_problem("narrow"), _so(loss_type=int(loss), loss_scale=scale)
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs)
    assert P.plain_model == -1
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)


def case_shared_intrinsics(lib, incidences, verbose=False):
    """Three cameras shared by twelve images: the pair terms of the Schur-Jacobi blocks per incidence
    (ba_pair_cross_kernel / ba_pair_finalize_kernel) or per observation (COLMAP_AMD_BA_PAIR_INCIDENCES=0), each held to
    the longdouble block diagonal of S."""
    fp, so = shared_problem(), _so()
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs, {"COLMAP_AMD_BA_PAIR_INCIDENCES": int(incidences)})
    assert P.n_paired > 0 and (P.pv_n > 0) == bool(incidences)
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)


def case_heavy_blocks(lib, verbose=False):
    fp, so = heavy_problem(), _so()
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs, {"COLMAP_AMD_BA_CHUNK": 64, "COLMAP_AMD_BA_HEAVY_CHUNKS": 1})
    assert P.n_heavy > 0 and P.n_paired > 0
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)


def case_chunk_edges(lib, verbose=False):
    fp, so = chunk_edge_problem(), _so()
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs, {"COLMAP_AMD_BA_CHUNK": 64})
    counts = np.bincount(fp.obs_pose)
    assert sorted(counts.tolist()) == [1, 63, 64, 65, 129, 129, 129]
    # one chunk list per camera block and per variable pose block, 64 observations per chunk
    assert P.n_chunks == sum(-(-int(c) // 64) for i, c in enumerate(counts) for blk in (P.cam_off[i], P.pose_off[i]) if blk >= 0)
    assert sorted(counts[P.pose_off >= 0].tolist()) == [1, 63, 64, 65, 129, 129]
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)


def case_tiles(lib, kind, operator_f32=False, verbose=False):
    fp = tile_problem(kind)
    so = _so(operator_precision=est.OPERATOR_F32 if operator_f32 else est.OPERATOR_F64)
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs)
    if kind == "track513":
        assert P.n_tiles == 0 and P.rhs_pass_fused == 0
    else:
        assert P.n_tiles == {"pts": 2, "obs511": 2, "obs512": 2, "obs513": 2, "track512": 2}[kind]
        assert P.rhs_pass_fused == 1
    assert P.op32 == int(operator_f32)
    if operator_f32:
        assert np.array_equal(P.J32, P.J.astype(np.float32)), "the fp32 copies are not float32(J)"
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)


def case_degenerate(lib, kind, verbose=False):
    fp, so = degenerate_problem(kind), _so()
    xs = probe_vectors(fp)
    P = run_probe(lib, fp, so, xs)
    assert (P.n_c == 0) == (kind == "points_only") and (P.n_p == 0) == (kind == "cameras_only")
    if kind == "points_only":
        assert P.pcg_pipelined == -1
    check_linearisation(fp, P, so, verbose)
    check_steps(fp, P, so, xs, verbose=verbose)
