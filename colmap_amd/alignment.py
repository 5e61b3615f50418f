"""Model alignment and comparison on MI355X (include/colmap_amd_align.h, colmap_amd/csrc/model_align.hip).

The functions of the reference's estimators/alignment.{h,cc} on colmap_amd.scene.Reconstruction, thin over the C ABI:
the pair of models (or of point sets) is flattened and uploaded once, batches of similarity hypotheses are scored on
the GPU, and the LORANSAC loop of colmap_amd/csrc/align_plan.h decides. ComputeImageAlignmentError, the association
step of AlignReconstructionsViaPoints and everything about poses stay on the host. There is no CPU fallback: without
the library or a device the calls raise.

A scene.Reconstruction carries no image names; the functions that match images by name (FindCommonRegImageIds,
AlignReconstructionToLocations) take `names` dicts image_id -> name and fall back to the image ids themselves.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import scene

MAX_BATCH = 1024  # ALIGN_MAX_BATCH


class _Camera(C.Structure):  # align_camera
    _fields_ = [("model_id", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("num_params", C.c_int32),
                ("params", C.c_double * 16)]


class _Pair(C.Structure):  # align_reproj_pair
    _fields_ = [("num_images", C.c_int32), ("reserved", C.c_int32), ("num_records", C.c_int64),
                ("src_cameras", C.c_void_p), ("tgt_cameras", C.c_void_p), ("src_poses", C.c_void_p),
                ("tgt_poses", C.c_void_p), ("src_num_points2D", C.c_void_p), ("tgt_num_points2D", C.c_void_p),
                ("rec_image", C.c_void_p), ("rec_src_xyz", C.c_void_p), ("rec_tgt_xyz", C.c_void_p),
                ("rec_src_xy", C.c_void_p), ("rec_tgt_xy", C.c_void_p)]


class _Options(C.Structure):  # align_options
    _fields_ = [("max_error", C.c_double), ("min_inlier_observations", C.c_double), ("min_inlier_ratio", C.c_double),
                ("confidence", C.c_double), ("dyn_num_trials_multiplier", C.c_double), ("min_num_trials", C.c_int32),
                ("max_num_trials", C.c_int32), ("random_seed", C.c_int32), ("batch_size", C.c_int32)]


class _Report(C.Structure):  # align_report
    _fields_ = [("success", C.c_int32), ("reserved", C.c_int32), ("num_trials", C.c_int64), ("num_inliers", C.c_int64),
                ("residual_sum", C.c_double), ("model", C.c_double * 8), ("inlier_mask", C.c_void_p),
                ("num_scored", C.c_int64), ("num_launches", C.c_int64)]


class AlignmentError(RuntimeError):
    pass


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "align_reproj_score"):
        raise _lib.LibraryMissingError("the loaded library has no align_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    L.align_last_error.restype = C.c_char_p
    L.align_destroy.restype = None
    L.align_destroy.argtypes = [C.c_void_p]
    return L


def _check(L, rc):
    if rc != 0:
        raise AlignmentError(L.align_last_error().decode())


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def hypothesis_tile() -> int:
    """Hypotheses one workgroup of a scoring kernel walks (ALIGN_HYPOTHESIS_TILE of the loaded library)."""
    return int(lib().align_hypothesis_tile())


def last_timing() -> Tuple[float, float]:
    """(kernel ms, total ms) of the last call of this thread."""
    k, t = C.c_double(), C.c_double()
    lib().align_last_timing(C.byref(k), C.byref(t))
    return k.value, t.value


# ----------------------------------------------------------------------------------------------------------------------
# Sim3d
# ----------------------------------------------------------------------------------------------------------------------

@dataclass
class Sim3d:
    """geometry/sim3.h: x -> scale * (R x) + translation; rotation is a unit quaternion w x y z."""
    scale: float = 1.0
    rotation: np.ndarray = field(default_factory=lambda: np.array([1.0, 0.0, 0.0, 0.0]))
    translation: np.ndarray = field(default_factory=lambda: np.zeros(3))

    def params(self) -> np.ndarray:
        """The 8 doubles of the C ABI and of ToFile: scale, qw qx qy qz, tx ty tz."""
        return np.concatenate([[self.scale], np.asarray(self.rotation, np.float64), np.asarray(self.translation, np.float64)])

    @staticmethod
    def from_params(p) -> "Sim3d":
        p = np.asarray(p, np.float64).ravel()
        if len(p) != 8:
            raise AlignmentError(f"a Sim3d has 8 parameters, got {len(p)}")
        return Sim3d(float(p[0]), p[1:5].copy(), p[5:8].copy())

    @staticmethod
    def from_srt(scale: float, rot: np.ndarray, trans: np.ndarray) -> "Sim3d":
        q = scene.rot_to_quat(np.asarray(rot, np.float64).reshape(3, 3))  # xyzw
        return Sim3d(float(scale), np.array([q[3], q[0], q[1], q[2]]), np.asarray(trans, np.float64).copy())

    def RotationMatrix(self) -> np.ndarray:
        w, x, y, z = np.asarray(self.rotation, np.float64) / np.linalg.norm(self.rotation)
        return scene.quat_to_rot(np.array([x, y, z, w]))

    def ToMatrix(self) -> np.ndarray:
        return np.hstack([self.scale * self.RotationMatrix(), np.asarray(self.translation, np.float64).reshape(3, 1)])

    def __mul__(self, x: np.ndarray) -> np.ndarray:
        """b_from_a * x_in_a for one point [3] or rows of points [N][3]."""
        x = np.asarray(x, np.float64)
        return self.scale * (x @ self.RotationMatrix().T) + np.asarray(self.translation, np.float64)

    def ToFile(self, path: str):
        """geometry/sim3.cc:39-48: one line, 17 significant digits: scale qw qx qy qz tx ty tz."""
        with open(path, "w") as f:
            f.write(" ".join(f"{float(v):.17g}" for v in self.params()) + "\n")

    @staticmethod
    def FromFile(path: str) -> "Sim3d":
        """geometry/sim3.cc:50-63."""
        with open(path) as f:
            vals = f.read().split()
        if len(vals) < 8:
            raise AlignmentError(f"{path}: a Sim3d file holds 8 numbers")
        return Sim3d.from_params([float(v) for v in vals[:8]])


def Inverse(b_from_a: Sim3d) -> Sim3d:
    """geometry/sim3.h:98-105."""
    w, x, y, z = np.asarray(b_from_a.rotation, np.float64) / np.linalg.norm(b_from_a.rotation)
    inv = Sim3d(1.0 / b_from_a.scale, np.array([w, -x, -y, -z]))
    inv.translation = (inv.RotationMatrix() @ np.asarray(b_from_a.translation, np.float64)) / -b_from_a.scale
    return inv


# ----------------------------------------------------------------------------------------------------------------------
# options and report
# ----------------------------------------------------------------------------------------------------------------------

@dataclass
class RANSACOptions:
    """colmap::RANSACOptions (optim/ransac.h:50-83). random_seed: the reference's -1 (nondeterministic) does not exist
    here, the sample stream is a fixed 64-bit LCG. batch_size: hypotheses per launch, 0 = the library's default; the
    report does not depend on it."""
    max_error: float = 0.0
    min_inlier_ratio: float = 0.1
    confidence: float = 0.99
    dyn_num_trials_multiplier: float = 3.0
    min_num_trials: int = 0
    max_num_trials: int = 2 ** 31 - 1
    random_seed: int = 0
    batch_size: int = 0


@dataclass
class Report:
    """RANSAC::Report."""
    success: bool
    num_trials: int
    num_inliers: int
    residual_sum: float
    model: Sim3d
    inlier_mask: np.ndarray
    num_scored: int = 0
    num_launches: int = 0
    kernel_ms: float = 0.0
    total_ms: float = 0.0


def _c_options(o: RANSACOptions, min_inlier_observations: float = 0.0) -> _Options:
    return _Options(float(o.max_error), float(min_inlier_observations), float(o.min_inlier_ratio), float(o.confidence),
                    float(o.dyn_num_trials_multiplier), int(o.min_num_trials), int(o.max_num_trials), int(o.random_seed),
                    int(o.batch_size))


def _sims(hypotheses) -> np.ndarray:
    if isinstance(hypotheses, Sim3d):
        hypotheses = [hypotheses]
    if len(hypotheses) and isinstance(hypotheses[0], Sim3d):
        hypotheses = [h.params() for h in hypotheses]
    return np.ascontiguousarray(hypotheses, np.float64).reshape(-1, 8)


class _Handle:
    def __init__(self):
        self._L = lib()
        self._h = C.c_void_p()

    def close(self):
        if self._h:
            self._L.align_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _estimate(self, entry, c_opt: _Options, num_samples: int) -> Report:
        mask = np.zeros(num_samples, np.uint8)
        rep = _Report()
        rep.inlier_mask = _ptr(mask) if num_samples else None
        _check(self._L, getattr(self._L, entry)(self._h, C.byref(c_opt), C.byref(rep)))
        k, t = last_timing()
        return Report(bool(rep.success), int(rep.num_trials), int(rep.num_inliers), float(rep.residual_sum),
                      Sim3d.from_params(list(rep.model)), mask.astype(bool), int(rep.num_scored), int(rep.num_launches), k, t)


# ----------------------------------------------------------------------------------------------------------------------
# the reprojection scorer
# ----------------------------------------------------------------------------------------------------------------------

@dataclass
class FlatPair:
    """The common images of two models and their common observations as the flat arrays of align_reproj_pair.
    cameras: sequences of (model_id, width, height, params), one per image slot."""
    src_cameras: Sequence
    tgt_cameras: Sequence
    src_poses: np.ndarray         # [I][7] qx qy qz qw tx ty tz
    tgt_poses: np.ndarray
    src_num_points2D: np.ndarray  # [I]
    tgt_num_points2D: np.ndarray
    rec_image: np.ndarray         # [N] image slot
    rec_src_xyz: np.ndarray       # [N][3]
    rec_tgt_xyz: np.ndarray
    rec_src_xy: np.ndarray        # [N][2]
    rec_tgt_xy: np.ndarray
    image_ids: List[Tuple[int, int]] = field(default_factory=list)  # (src id, tgt id) of every slot

    @property
    def num_images(self) -> int:
        return len(self.src_poses)


def _c_cameras(cams):
    out = (_Camera * max(len(cams), 1))()
    for i, (model_id, width, height, params) in enumerate(cams):
        p = np.asarray(params, np.float64).ravel()
        if len(p) > 16:
            raise AlignmentError(f"camera {i}: {len(p)} parameters")
        out[i].model_id, out[i].width, out[i].height, out[i].num_params = int(model_id), int(width), int(height), len(p)
        for k, v in enumerate(p):
            out[i].params[k] = float(v)
    return out


class ReprojScorer(_Handle):
    """align_reproj_create: a model pair on the device. score() evaluates hypotheses of the caller's choosing,
    estimate() runs the search."""

    def __init__(self, pair: FlatPair, gpu_index: int = 0):
        super().__init__()
        I = pair.num_images
        arr = lambda a, t, w: np.ascontiguousarray(a, t).reshape(-1, w) if w else np.ascontiguousarray(a, t).ravel()
        sp, tp = arr(pair.src_poses, np.float64, 7), arr(pair.tgt_poses, np.float64, 7)
        sn, tn = arr(pair.src_num_points2D, np.int32, 0), arr(pair.tgt_num_points2D, np.int32, 0)
        ri = arr(pair.rec_image, np.int32, 0)
        sx, tx = arr(pair.rec_src_xyz, np.float64, 3), arr(pair.rec_tgt_xyz, np.float64, 3)
        sxy, txy = arr(pair.rec_src_xy, np.float64, 2), arr(pair.rec_tgt_xy, np.float64, 2)
        if not (len(tp) == I and len(sn) == I and len(tn) == I and len(pair.src_cameras) == I and len(pair.tgt_cameras) == I):
            raise AlignmentError("the per-image arrays of the pair do not have one entry per common image")
        if not (len(sx) == len(ri) and len(tx) == len(ri) and len(sxy) == len(ri) and len(txy) == len(ri)):
            raise AlignmentError("the record arrays of the pair do not have the same length")
        sc, tc = _c_cameras(pair.src_cameras), _c_cameras(pair.tgt_cameras)
        cp = _Pair(I, 0, len(ri), C.cast(sc, C.c_void_p), C.cast(tc, C.c_void_p), _ptr(sp), _ptr(tp), _ptr(sn), _ptr(tn),
                   _ptr(ri), _ptr(sx), _ptr(tx), _ptr(sxy), _ptr(txy))
        self.num_images = I
        _check(self._L, self._L.align_reproj_create(C.byref(cp), C.c_int32(gpu_index), C.byref(self._h)))

    def score(self, hypotheses, max_reproj_error: float) -> Tuple[np.ndarray, np.ndarray]:
        """(inliers [B][I] uint32, common [I] uint32)."""
        sims = _sims(hypotheses)
        inliers = np.zeros((len(sims), self.num_images), np.uint32)
        common = np.zeros(self.num_images, np.uint32)
        _check(self._L, self._L.align_reproj_score(self._h, _ptr(sims), C.c_int32(len(sims)), C.c_double(max_reproj_error),
                                                   _ptr(inliers), _ptr(common)))
        return inliers, common

    def estimate(self, min_inlier_observations: float = 0.3, max_reproj_error: float = 8.0,
                 options: Optional[RANSACOptions] = None) -> Report:
        o = options or RANSACOptions(min_inlier_ratio=0.2)
        c = _c_options(o, min_inlier_observations)
        c.max_error = float(max_reproj_error)
        return self._estimate("align_reproj_estimate", c, self.num_images)


class PositionScorer(_Handle):
    """align_positions_create: two point sets of equal length on the device."""

    def __init__(self, src: np.ndarray, tgt: np.ndarray, gpu_index: int = 0):
        super().__init__()
        src = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
        tgt = np.ascontiguousarray(tgt, np.float64).reshape(-1, 3)
        if len(src) != len(tgt):
            raise AlignmentError("src and tgt must have the same number of points")
        self.num_points = len(src)
        _check(self._L, self._L.align_positions_create(_ptr(src), _ptr(tgt), C.c_int64(len(src)), C.c_int32(gpu_index),
                                                       C.byref(self._h)))

    def score(self, hypotheses, max_error: float, want_mask: bool = False):
        """(num_inliers [B] int64, residual_sum [B] float64[, inlier_mask [B][N] bool])."""
        sims = _sims(hypotheses)
        n = np.zeros(len(sims), np.int64)
        s = np.zeros(len(sims), np.float64)
        mask = np.zeros((len(sims), self.num_points), np.uint8) if want_mask else None
        _check(self._L, self._L.align_positions_score(self._h, _ptr(sims), C.c_int32(len(sims)), C.c_double(max_error),
                                                      _ptr(n), _ptr(s), _ptr(mask)))
        return (n, s, mask.astype(bool)) if want_mask else (n, s)

    def estimate(self, options: RANSACOptions) -> Report:
        return self._estimate("align_positions_estimate", _c_options(options), self.num_points)


def transform_points(points: np.ndarray, new_from_old: Sim3d, gpu_index: int = 0) -> np.ndarray:
    """align_transform_points: new_from_old * X for every row of points [N][3]; returns a new array."""
    out = np.array(points, np.float64, order="C").reshape(-1, 3)
    L = lib()
    sim = np.ascontiguousarray(new_from_old.params())
    _check(L, L.align_transform_points(_ptr(out), C.c_int64(len(out)), _ptr(sim), C.c_int32(gpu_index)))
    return out


def EstimateSim3dRobust(src: np.ndarray, tgt: np.ndarray, options: RANSACOptions, gpu_index: int = 0) -> Report:
    """solvers/similarity_transform.cc:103-115 on the GPU."""
    with PositionScorer(src, tgt, gpu_index) as scorer:
        return scorer.estimate(options)


# ----------------------------------------------------------------------------------------------------------------------
# estimators/alignment.h on scene.Reconstruction
# ----------------------------------------------------------------------------------------------------------------------

def FindCommonRegImageIds(src: scene.Reconstruction, tgt: scene.Reconstruction, src_names: Optional[Dict[int, str]] = None,
                          tgt_names: Optional[Dict[int, str]] = None) -> List[Tuple[int, int]]:
    """Reconstruction::FindCommonRegImageIds (scene/reconstruction.cc:856-871): the registered images of `src` that `tgt`
    holds under the same name, in the order of src's image ids. Without names an image's name is its id."""
    name_of = (lambda names, i: i) if src_names is None or tgt_names is None else (lambda names, i: names[i])
    by_name = {name_of(tgt_names, i): i for i in tgt.RegImageIds()}
    out = []
    for i in src.RegImageIds():
        j = by_name.get(name_of(src_names, i))
        if j is not None:
            out.append((i, j))
    return out


def _cam_tuple(rec, image_id):
    c = rec.cameras[rec.images[image_id].camera_id]
    return (c.model_id, c.width, c.height, c.params)


def flatten_pair(src: scene.Reconstruction, tgt: scene.Reconstruction, src_names=None, tgt_names=None) -> FlatPair:
    """The records of ReconstructionAlignmentEstimator::Residuals (alignment.cc:106-139): for every common image, every
    point2D_idx at which both images carry a 3D point."""
    ids = FindCommonRegImageIds(src, tgt, src_names, tgt_names)
    rec_image, sxyz, txyz, sxy, txy = [], [], [], [], []
    for slot, (i, j) in enumerate(ids):
        a, b = src.images[i], tgt.images[j]
        for pa, pb in zip(a.points2D, b.points2D):
            if pa.HasPoint3D() and pb.HasPoint3D():
                rec_image.append(slot)
                sxyz.append(src.points3D[pa.point3D_id].xyz)
                txyz.append(tgt.points3D[pb.point3D_id].xyz)
                sxy.append(pa.xy)
                txy.append(pb.xy)
    return FlatPair(
        [_cam_tuple(src, i) for i, _ in ids], [_cam_tuple(tgt, j) for _, j in ids],
        np.array([src.images[i].cam_from_world for i, _ in ids], np.float64).reshape(-1, 7),
        np.array([tgt.images[j].cam_from_world for _, j in ids], np.float64).reshape(-1, 7),
        np.array([len(src.images[i].points2D) for i, _ in ids], np.int32),
        np.array([len(tgt.images[j].points2D) for _, j in ids], np.int32),
        np.array(rec_image, np.int32), np.array(sxyz, np.float64).reshape(-1, 3), np.array(txyz, np.float64).reshape(-1, 3),
        np.array(sxy, np.float64).reshape(-1, 2), np.array(txy, np.float64).reshape(-1, 2), ids)


def AlignReconstructionsViaReprojections(src: scene.Reconstruction, tgt: scene.Reconstruction,
                                         min_inlier_observations: float = 0.3, max_reproj_error: float = 8.0,
                                         src_names=None, tgt_names=None, gpu_index: int = 0,
                                         options: Optional[RANSACOptions] = None, report: Optional[list] = None) -> Optional[Sim3d]:
    """alignment.cc:301-342: tgt_from_src, or None where the reference returns false. `report`, a list, receives the
    search's Report."""
    if not 0.0 <= min_inlier_observations <= 1.0:
        raise AlignmentError("min_inlier_observations must lie in [0, 1]")
    pair = flatten_pair(src, tgt, src_names, tgt_names)
    if pair.num_images < 3:
        return None
    with ReprojScorer(pair, gpu_index) as scorer:
        rep = scorer.estimate(min_inlier_observations, max_reproj_error, options)
    if report is not None:
        report.append(rep)
    return rep.model if rep.success else None


def AlignReconstructionToLocations(src: scene.Reconstruction, tgt_image_names: Sequence, tgt_image_locations: np.ndarray,
                                   min_common_images: int, ransac_options: RANSACOptions, src_names=None,
                                   gpu_index: int = 0) -> Optional[Sim3d]:
    """alignment.cc:185-238. tgt_image_names are image names (with `src_names`) or image ids (without)."""
    if min_common_images < 3:
        raise AlignmentError("min_common_images must be at least 3")
    locations = np.asarray(tgt_image_locations, np.float64).reshape(-1, 3)
    if len(tgt_image_names) != len(locations):
        raise AlignmentError("one location per image name")
    by_name = {(src_names[i] if src_names is not None else i): i for i in src.RegImageIds()}
    seen, a, b = set(), [], []
    for name, loc in zip(tgt_image_names, locations):
        i = by_name.get(name)
        if i is None or i in seen:  # not in the model; duplicates are ignored
            continue
        seen.add(i)
        a.append(src.ProjectionCenter(i))
        b.append(loc)
    if len(seen) < min_common_images:
        return None
    rep = EstimateSim3dRobust(np.array(a), np.array(b), ransac_options, gpu_index)
    if rep.num_inliers < min_common_images:
        return None
    return rep.model


def AlignReconstructionsViaProjCenters(src: scene.Reconstruction, tgt: scene.Reconstruction, max_proj_center_error: float,
                                       src_names=None, tgt_names=None, gpu_index: int = 0) -> Optional[Sim3d]:
    """alignment.cc:344-369."""
    if not max_proj_center_error > 0:
        raise AlignmentError("max_proj_center_error must be positive")
    ids = tgt.RegImageIds()
    names = [tgt_names[i] if (src_names is not None and tgt_names is not None) else i for i in ids]
    centers = np.array([tgt.ProjectionCenter(i) for i in ids], np.float64).reshape(-1, 3)
    return AlignReconstructionToLocations(src, names, centers, 3, RANSACOptions(max_error=max_proj_center_error),
                                          src_names if tgt_names is not None else None, gpu_index)


def associate_points(src: scene.Reconstruction, tgt: scene.Reconstruction, min_common_observations: int):
    """The association step of AlignReconstructionsViaPoints (alignment.cc:411-447) as written: a src point votes, per
    track element, for the tgt point the same (image, point2D_idx) carries; a tgt point's count STARTS AT 0, so it is
    the number of votes minus one; the first point with the largest count wins and is kept when that count reaches
    min_common_observations. Returns (src xyz [M][3], tgt xyz [M][3])."""
    a, b = [], []
    for pid, pt in src.points3D.items():
        counts: Dict[int, int] = {}
        for (image_id, idx) in pt.track:
            if image_id not in tgt.images:
                continue
            p2 = tgt.images[image_id].points2D[idx]
            if p2.HasPoint3D():
                counts[p2.point3D_id] = counts[p2.point3D_id] + 1 if p2.point3D_id in counts else 0
        if not counts:
            continue
        best = max(counts, key=lambda k: counts[k])  # the first of the largest, like std::max_element
        if counts[best] >= min_common_observations:
            a.append(pt.xyz)
            b.append(tgt.points3D[best].xyz)
    return np.array(a, np.float64).reshape(-1, 3), np.array(b, np.float64).reshape(-1, 3)


def AlignReconstructionsViaPoints(src: scene.Reconstruction, tgt: scene.Reconstruction, min_common_observations: int = 3,
                                  max_error: float = 0.005, min_inlier_ratio: float = 0.9, gpu_index: int = 0) -> Optional[Sim3d]:
    """alignment.cc:400-458."""
    if not (min_common_observations > 0 and max_error > 0.0 and 0.0 <= min_inlier_ratio <= 1.0):
        raise AlignmentError("min_common_observations and max_error must be positive, min_inlier_ratio in [0, 1]")
    a, b = associate_points(src, tgt, min_common_observations)
    rep = EstimateSim3dRobust(a, b, RANSACOptions(max_error=max_error, min_inlier_ratio=min_inlier_ratio), gpu_index)
    return rep.model if rep.success else None


@dataclass
class ImageAlignmentError:
    image_name: object
    rotation_error_deg: float
    proj_center_error: float


def _rigid_inverse(pose: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(rotation matrix, translation) of Inverse(Rigid3d)."""
    R = scene.quat_to_rot(pose[:4])
    return R.T, -R.T @ pose[4:]


def ComputeImageAlignmentError(src: scene.Reconstruction, tgt: scene.Reconstruction, tgt_from_src: Sim3d, src_names=None,
                               tgt_names=None) -> List[ImageAlignmentError]:
    """alignment.cc:371-398, on the host: per common image the angle between the two world_from_cam rotations, in
    degrees, and the distance of the two projection centres, after moving the src camera by tgt_from_src
    (TransformCameraWorld, geometry/sim3.h: R' = R_c R^T, t' = s t_c - R' t)."""
    R, s, t = tgt_from_src.RotationMatrix(), tgt_from_src.scale, np.asarray(tgt_from_src.translation, np.float64)
    errors = []
    for (i, j) in FindCommonRegImageIds(src, tgt, src_names, tgt_names):
        pose = src.images[i].cam_from_world
        Rn = scene.quat_to_rot(pose[:4]) @ R.T
        tn = s * pose[4:] - Rn @ t
        Ra, ca = Rn.T, -Rn.T @ tn
        Rb, cb = _rigid_inverse(tgt.images[j].cam_from_world)
        qa, qb = scene.rot_to_quat(Ra), scene.rot_to_quat(Rb)
        # Eigen's angularDistance: 2 * atan2(|vec(d)|, |d.w|) of d = a * conj(b)
        d = scene.quat_mul(qa, np.array([-qb[0], -qb[1], -qb[2], qb[3]]))
        angle = 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))
        errors.append(ImageAlignmentError(src_names[i] if src_names is not None else i, float(np.rad2deg(angle)),
                                          float(np.linalg.norm(ca - cb))))
    return errors


def transform_reconstruction(rec: scene.Reconstruction, new_from_old: Sim3d, gpu_index: int = 0):
    """Reconstruction::Transform (scene/reconstruction.cc:788-805) in place: the points on the device, poses, rigs and
    frames on the host."""
    ids = list(rec.points3D)
    pts = np.array([rec.points3D[p].xyz for p in ids], np.float64).reshape(-1, 3)
    moved = transform_points(pts, new_from_old, gpu_index)
    saved, rec.points3D = rec.points3D, {}
    try:
        rec.Transform(new_from_old.scale, new_from_old.RotationMatrix(), np.asarray(new_from_old.translation, np.float64))
    finally:
        rec.points3D = saved
    for k, p in enumerate(ids):
        rec.points3D[p].xyz = moved[k].copy()
