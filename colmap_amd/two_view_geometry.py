"""Two-view geometry estimation on MI355X (include/colmap_amd_tvg.h, colmap_amd/csrc/two_view.hip).

EstimateTwoViewGeometry of the reference's estimators/two_view_geometry.{h,cc} on the routes that need only a
fundamental matrix and a homography, thin over the C ABI: a batch of point sets is uploaded, minimal samples are solved
and models scored on the GPU, and the LORANSAC walk of colmap_amd/csrc/two_view_plan.h decides. The routes that need an
essential matrix or a focal solver are not built: `estimate_two_view_geometries` names the route of every pair and
returns None for those. There is no CPU fallback: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import camera as CAM

KIND_F, KIND_H, KIND_T = 0, 1, 2
MIN_SAMPLES = {KIND_F: 7, KIND_H: 4, KIND_T: 1}
MAX_MODELS = 3

# TwoViewGeometry::ConfigurationType (scene/two_view_geometry.h:44-67)
UNDEFINED, DEGENERATE, CALIBRATED, UNCALIBRATED, PLANAR, PANORAMIC, PLANAR_OR_PANORAMIC, WATERMARK, MULTIPLE = range(9)
CALIBRATED_RIG = 9
NOT_BUILT = -1

(ROUTE_FORCED_H_DEGENERATE, ROUTE_FORCED_H, ROUTE_ONE_SIDED_FOCAL, ROUTE_SPHERICAL, ROUTE_SHARED_FOCAL, ROUTE_CALIBRATED,
 ROUTE_FISHEYE_DEGENERATE, ROUTE_UNCALIBRATED) = range(8)


class _Camera(C.Structure):  # tvg_camera
    _fields_ = [("model_id", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("camera_id", C.c_int32),
                ("has_prior_focal_length", C.c_int32)]


class _Ransac(C.Structure):  # tvg_ransac_options
    _fields_ = [("max_error", C.c_double), ("min_inlier_ratio", C.c_double), ("confidence", C.c_double),
                ("dyn_num_trials_multiplier", C.c_double), ("min_num_trials", C.c_int32), ("max_num_trials", C.c_int32),
                ("random_seed", C.c_int32), ("trials_per_round", C.c_int32)]


class _Options(C.Structure):  # tvg_options
    _fields_ = [("ransac", _Ransac), ("min_num_inliers", C.c_int32), ("detect_watermark", C.c_int32),
                ("multiple_ignore_watermark", C.c_int32), ("filter_stationary_matches", C.c_int32),
                ("force_H_use", C.c_int32), ("multiple_models", C.c_int32), ("max_H_inlier_ratio", C.c_double),
                ("watermark_min_inlier_ratio", C.c_double), ("watermark_border_size", C.c_double),
                ("watermark_detection_max_error", C.c_double), ("stationary_matches_max_error", C.c_double)]


class _Report(C.Structure):  # tvg_report
    _fields_ = [("success", C.c_int32), ("has_model", C.c_int32), ("num_trials", C.c_int64), ("num_inliers", C.c_int64),
                ("residual_sum", C.c_double), ("model", C.c_double * 9), ("inlier_mask", C.c_void_p),
                ("num_scored", C.c_int64), ("num_launches", C.c_int64)]


class TwoViewGeometryError(RuntimeError):
    pass


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "tvg_score"):
        raise _lib.LibraryMissingError("the loaded library has no tvg_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    L.tvg_last_error.restype = C.c_char_p
    L.tvg_route_name.restype = C.c_char_p
    L.tvg_destroy.restype = None
    L.tvg_destroy.argtypes = [C.c_void_p]
    L.tvg_draw_sample.argtypes = [C.c_int32, C.c_uint64, C.c_int32, C.c_uint64, C.c_uint32, C.c_void_p]
    L.tvg_score.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 5
    return L


def _check(L, rc):
    if rc != 0:
        raise TwoViewGeometryError(L.tvg_last_error().decode())


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def model_tile() -> int:
    return int(lib().tvg_model_tile())


def match_tile() -> int:
    return int(lib().tvg_match_tile())


def trial_round() -> int:
    return int(lib().tvg_trial_round())


def last_timing() -> Tuple[float, float]:
    """(kernel ms, total ms) of the last call of this thread."""
    k, t = C.c_double(), C.c_double()
    lib().tvg_last_timing(C.byref(k), C.byref(t))
    return k.value, t.value


@dataclass
class RANSACOptions:
    """optim/ransac.h:50-83 with the values of TwoViewGeometryOptions' constructor."""
    max_error: float = 4.0
    min_inlier_ratio: float = 0.25
    confidence: float = 0.999
    dyn_num_trials_multiplier: float = 3.0
    min_num_trials: int = 100
    max_num_trials: int = 10000
    random_seed: int = -1
    trials_per_round: int = 0

    def c(self) -> _Ransac:
        return _Ransac(self.max_error, self.min_inlier_ratio, self.confidence, self.dyn_num_trials_multiplier,
                       self.min_num_trials, self.max_num_trials, self.random_seed, self.trials_per_round)


@dataclass
class TwoViewGeometryOptions:
    """estimators/two_view_geometry.h:44-131, the options of the built routes."""
    min_num_inliers: int = 15
    max_H_inlier_ratio: float = 0.8
    watermark_min_inlier_ratio: float = 0.7
    watermark_border_size: float = 0.1
    detect_watermark: bool = True
    multiple_ignore_watermark: bool = True
    watermark_detection_max_error: float = 4.0
    filter_stationary_matches: bool = False
    stationary_matches_max_error: float = 4.0
    force_H_use: bool = False
    multiple_models: bool = False
    ransac_options: RANSACOptions = field(default_factory=RANSACOptions)

    def c(self) -> _Options:
        return _Options(self.ransac_options.c(), self.min_num_inliers, int(self.detect_watermark),
                        int(self.multiple_ignore_watermark), int(self.filter_stationary_matches), int(self.force_H_use),
                        int(self.multiple_models), self.max_H_inlier_ratio, self.watermark_min_inlier_ratio,
                        self.watermark_border_size, self.watermark_detection_max_error, self.stationary_matches_max_error)


@dataclass
class CameraInfo:
    """What the router reads of a camera."""
    model_id: int
    width: int
    height: int
    camera_id: int = 1
    has_prior_focal_length: bool = False

    def c(self) -> _Camera:
        return _Camera(self.model_id, self.width, self.height, self.camera_id, int(self.has_prior_focal_length))

    def is_spherical(self) -> bool:
        return CAM.MODELS[self.model_id].is_spherical

    def is_perspective_fisheye(self) -> bool:
        return CAM.MODELS[self.model_id].is_fisheye

    def is_perspective_pinhole(self) -> bool:
        return not self.is_spherical() and not self.is_perspective_fisheye()


@dataclass
class TwoViewGeometry:
    """scene/two_view_geometry.h; inlier_matches are rows of the matches that were given."""
    config: int = UNDEFINED
    inlier_matches: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.uint32))
    F: Optional[np.ndarray] = None
    H: Optional[np.ndarray] = None
    inlier_mask: Optional[np.ndarray] = None
    route: int = ROUTE_UNCALIBRATED


@dataclass
class Report:
    """LORANSAC::Report of one point set."""
    success: bool
    has_model: bool
    num_trials: int
    num_inliers: int
    residual_sum: float
    model: np.ndarray
    inlier_mask: np.ndarray
    num_scored: int
    num_launches: int


def route(camera1: CameraInfo, camera2: CameraInfo, options: TwoViewGeometryOptions) -> int:
    o, c1, c2 = options.c(), camera1.c(), camera2.c()
    return int(lib().tvg_route(C.byref(c1), C.byref(c2), C.byref(o)))


def route_name(r: int) -> str:
    return lib().tvg_route_name(C.c_int32(r)).decode()


def route_is_built(r: int) -> bool:
    return bool(lib().tvg_route_is_built(C.c_int32(r)))


def draw_sample(random_seed: int, stream_id: int, kind: int, trial: int, num_points: int) -> np.ndarray:
    """The sample of (random_seed, stream_id, kind, trial) among num_points matches (two_view_solvers.h)."""
    L = lib()
    out = np.zeros(7, np.uint32)
    _check(L, L.tvg_draw_sample(random_seed, stream_id, kind, trial, num_points, _ptr(out)))
    return out[:MIN_SAMPLES[kind]].copy()


class PointSets:
    """A batch of point sets on the device. sets: arrays [n][4] (x1 y1 x2 y2); stream_ids: a 64-bit key per set."""

    def __init__(self, gpu_index: int = 0):
        self._L = lib()
        self._h = C.c_void_p()
        _check(self._L, self._L.tvg_create(C.c_int32(gpu_index), C.byref(self._h)))
        self.counts: List[int] = []

    def close(self):
        if self._h:
            self._L.tvg_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_points(self, sets: Sequence[np.ndarray], stream_ids: Sequence[int]):
        if len(sets) != len(stream_ids):
            raise TwoViewGeometryError("one stream id per set")
        sets = [np.ascontiguousarray(s, np.float64).reshape(-1, 4) for s in sets]
        self.counts = [len(s) for s in sets]
        offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        pts = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros((0, 4)))
        ids = np.array([int(i) & 0xFFFFFFFFFFFFFFFF for i in stream_ids], np.uint64)
        _check(self._L, self._L.tvg_set_points(self._h, C.c_int32(len(sets)), _ptr(offsets), _ptr(pts), _ptr(ids)))

    def hypothesize(self, kind: int, random_seed: int, items: Sequence[Tuple[int, int, int]], samples: bool = False):
        """items: (set, first_trial, num_trials). Returns num_models [trials], models [trials][3][9] (and samples)."""
        sets = np.array([i[0] for i in items], np.int32)
        first = np.array([i[1] for i in items], np.int64)
        count = np.array([i[2] for i in items], np.int32)
        total = int(count.sum()) if len(items) else 0
        num_models = np.zeros(total, np.int32)
        models = np.zeros((total, MAX_MODELS, 9), np.float64)
        smp = np.zeros((total, 7), np.uint32) if samples else None
        _check(self._L, self._L.tvg_hypothesize(self._h, C.c_int32(kind), C.c_int32(random_seed), C.c_int32(len(items)),
                                                _ptr(sets), _ptr(first), _ptr(count), _ptr(num_models), _ptr(models), _ptr(smp)))
        return (num_models, models, smp[:, :MIN_SAMPLES[kind]]) if samples else (num_models, models)

    def score(self, kind: int, max_error: float, model_set: Sequence[int], models: np.ndarray, masks: bool = False):
        """Returns num_inliers [m], residual_sum [m] (and a list of masks)."""
        model_set = np.ascontiguousarray(model_set, np.int32)
        models = np.ascontiguousarray(models, np.float64).reshape(-1, 9)
        if len(models) != len(model_set):
            raise TwoViewGeometryError("one set per model")
        n = np.zeros(len(models), np.int64)
        s = np.zeros(len(models), np.float64)
        flat = None
        if masks:
            for m in model_set:
                if not 0 <= m < len(self.counts):
                    raise TwoViewGeometryError(f"set {m} out of range")
            flat = np.zeros(int(sum(self.counts[m] for m in model_set)), np.uint8)
        _check(self._L, self._L.tvg_score(self._h, kind, max_error, len(models), _ptr(model_set), _ptr(models), _ptr(n),
                                          _ptr(s), _ptr(flat)))
        if not masks:
            return n, s
        cuts = np.cumsum([self.counts[m] for m in model_set])[:-1] if len(model_set) else []
        return n, s, [m.copy() for m in np.split(flat, cuts)] if len(model_set) else []

    def estimate(self, kind: int, options: RANSACOptions, min_inlier_ratios: Optional[Sequence[float]] = None) -> List[Report]:
        """LORANSAC of one kind over all sets at once."""
        S = len(self.counts)
        reports = (_Report * max(S, 1))()
        masks = [np.zeros(max(n, 1), np.uint8) for n in self.counts]
        for s in range(S):
            reports[s].inlier_mask = masks[s].ctypes.data
        o = options.c()
        ratios = None if min_inlier_ratios is None else np.ascontiguousarray(min_inlier_ratios, np.float64)
        _check(self._L, self._L.tvg_estimate(self._h, C.c_int32(kind), C.byref(o), _ptr(ratios), reports))
        return [Report(bool(r.success), bool(r.has_model), int(r.num_trials), int(r.num_inliers), float(r.residual_sum),
                       np.array(r.model[:]), masks[s][:self.counts[s]].copy(), int(r.num_scored), int(r.num_launches))
                for s, r in enumerate(reports[:S])]

    def verify_pairs(self, cameras1: Sequence[CameraInfo], cameras2: Sequence[CameraInfo], points: Sequence[np.ndarray],
                     stream_ids: Sequence[int], options: TwoViewGeometryOptions):
        """EstimateTwoViewGeometry for a batch of pairs; points[p] is [n][4]. Returns (geometries, stats)."""
        P = len(points)
        points = [np.ascontiguousarray(s, np.float64).reshape(-1, 4) for s in points]
        counts = [len(s) for s in points]
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pts = np.ascontiguousarray(np.concatenate(points) if points else np.zeros((0, 4)))
        ids = np.array([int(i) & 0xFFFFFFFFFFFFFFFF for i in stream_ids], np.uint64)
        c1 = (_Camera * max(P, 1))(*[c.c() for c in cameras1])
        c2 = (_Camera * max(P, 1))(*[c.c() for c in cameras2])
        rt, cfg, hF, hH = (np.zeros(P, np.int32) for _ in range(4))
        F, H = np.zeros((P, 9)), np.zeros((P, 9))
        mask = np.zeros(max(int(offsets[-1]), 1), np.uint8)
        stats = np.zeros(2, np.int64)
        o = options.c()
        _check(self._L, self._L.tvg_verify_pairs(self._h, C.byref(o), C.c_int32(P), c1, c2, _ptr(offsets), _ptr(pts), _ptr(ids),
                                                 _ptr(rt), _ptr(cfg), _ptr(hF), _ptr(F), _ptr(hH), _ptr(H), _ptr(mask), _ptr(stats)))
        out = []
        for p in range(P):
            m = mask[offsets[p]:offsets[p + 1]].astype(bool)
            out.append(TwoViewGeometry(int(cfg[p]), np.zeros((0, 2), np.uint32), F[p].reshape(3, 3).copy() if hF[p] else None,
                                       H[p].reshape(3, 3).copy() if hH[p] else None, m, int(rt[p])))
        return out, {"num_scored": int(stats[0]), "num_launches": int(stats[1])}


def estimate_two_view_geometries(cameras1: Sequence[CameraInfo], points1: Sequence[np.ndarray], cameras2: Sequence[CameraInfo],
                                 points2: Sequence[np.ndarray], matches: Sequence[np.ndarray], stream_ids: Sequence[int],
                                 options: Optional[TwoViewGeometryOptions] = None, gpu_index: int = 0):
    """EstimateTwoViewGeometry for a batch of pairs: points1[p] / points2[p] are the keypoints [.][2] of the two
    images, matches[p] the uint32 [n][2] index pairs. A pair on a route that is not built gets None. Returns
    (geometries, routes, stats)."""
    options = options or TwoViewGeometryOptions()
    sets = []
    for p1, p2, m in zip(points1, points2, matches):
        m = np.asarray(m, np.int64).reshape(-1, 2)
        p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
        sets.append(np.hstack([p1[m[:, 0], :2], p2[m[:, 1], :2]]) if len(m) else np.zeros((0, 4)))
    with PointSets(gpu_index) as ps:
        geoms, stats = ps.verify_pairs(cameras1, cameras2, sets, stream_ids, options)
    out = []
    for g, m in zip(geoms, matches):
        if g.config == NOT_BUILT:
            out.append(None)
            continue
        g.inlier_matches = np.ascontiguousarray(np.asarray(m, np.uint32).reshape(-1, 2)[g.inlier_mask])
        out.append(g)
    return out, [g.route for g in geoms], stats


def estimate_two_view_geometry(camera1: CameraInfo, points1: np.ndarray, camera2: CameraInfo, points2: np.ndarray,
                               matches: np.ndarray, options: Optional[TwoViewGeometryOptions] = None, stream_id: int = 0,
                               gpu_index: int = 0) -> TwoViewGeometry:
    """EstimateTwoViewGeometry of one pair; raises for a route that is not built."""
    geoms, routes, _ = estimate_two_view_geometries([camera1], [points1], [camera2], [points2], [matches], [stream_id],
                                                    options, gpu_index)
    if geoms[0] is None:
        raise TwoViewGeometryError(f"the {route_name(routes[0])} route of EstimateTwoViewGeometry is not built: it needs an "
                                   "essential matrix or a focal solver")
    return geoms[0]
