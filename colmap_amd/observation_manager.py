"""Observation and point filtering of a sparse model on MI355X (include/colmap_amd_obs.h, colmap_amd/csrc/obs_filter.hip).

Mirrors the filter methods of colmap::ObservationManager (reference sfm/observation_manager.{h,cc}:353-585) on a
colmap_amd.scene.Reconstruction: each method flattens the points it looks at, lets the library decide on the GPU (one
keep byte per observation, one status byte per point) and applies the deletions here -- tracks, points2D[].point3D_id,
deleted points, Point3D.error -- returning the reference's filtered-observation count. There is no CPU fallback:
without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib
from . import scene

PIXEL, NORMALIZED, ANGULAR = 0, 1, 2                     # colmap::ReprojectionErrorType
RULE_REPROJ_ERROR, RULE_TRI_ANGLE = 1, 2                 # OBS_RULE_*
KEPT, DELETED_ERROR, DELETED_ANGLE, DELETED_SHORT, DELETED_DEPTH = range(5)  # OBS_POINT_*
_ERROR_TYPES = {"PIXEL": PIXEL, "NORMALIZED": NORMALIZED, "ANGULAR": ANGULAR}


class _Options(C.Structure):  # obs_filter_options
    _fields_ = [("max_reproj_error", C.c_double), ("min_tri_angle", C.c_double), ("min_track_len", C.c_int32),
                ("error_type", C.c_int32), ("rules", C.c_int32), ("reserved", C.c_int32)]


class _Camera(C.Structure):  # obs_camera
    _fields_ = [("model_id", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("num_params", C.c_int32),
                ("params", C.c_double * 16)]


class _Model(C.Structure):  # obs_model
    _fields_ = [("num_cameras", C.c_int32), ("num_images", C.c_int32), ("num_points", C.c_int64),
                ("num_observations", C.c_int64), ("cameras", C.c_void_p), ("image_poses", C.c_void_p),
                ("image_camera", C.c_void_p), ("points", C.c_void_p), ("obs_offsets", C.c_void_p),
                ("obs_image", C.c_void_p), ("obs_xy", C.c_void_p)]


class _Result(C.Structure):  # obs_result
    _fields_ = [("obs_keep", C.c_void_p), ("point_status", C.c_void_p), ("point_error", C.c_void_p),
                ("point_count", C.c_void_p), ("num_filtered", C.c_int64)]


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "obs_filter_all_points3D"):
        raise _lib.LibraryMissingError("the loaded library has no obs_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    L.obs_last_error.restype = C.c_char_p
    return L


class ObservationFilterError(RuntimeError):
    pass


def error_type_id(error_type) -> int:
    if isinstance(error_type, str):
        if error_type.upper() not in _ERROR_TYPES:
            raise ObservationFilterError(f"unknown ReprojectionErrorType {error_type}")
        return _ERROR_TYPES[error_type.upper()]
    return int(error_type)


@dataclass
class FlatModel:
    """A sparse model as the flat arrays of obs_model. cameras: sequence of (model_id, width, height, params)."""
    cameras: Sequence
    image_poses: np.ndarray    # [I][7] qx qy qz qw tx ty tz
    image_camera: np.ndarray   # [I] index into cameras
    points: np.ndarray         # [P][3]
    obs_offsets: np.ndarray    # [P + 1]
    obs_image: np.ndarray      # [O] index into the images
    obs_xy: np.ndarray         # [O][2]


@dataclass
class FilterResult:
    obs_keep: np.ndarray       # [O] uint8
    point_status: np.ndarray   # [P] uint8, OBS_POINT_*
    point_error: np.ndarray    # [P] float64, -1 where the rule assigns none
    point_count: np.ndarray    # [P] uint32
    num_filtered: int
    kernel_ms: float = 0.0
    total_ms: float = 0.0


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def run_flat(entry: str, m: FlatModel, max_reproj_error: float = 4.0, min_tri_angle: float = 1.5, min_track_len: int = 2,
             error_type=PIXEL, rules: int = RULE_REPROJ_ERROR | RULE_TRI_ANGLE, gpu_index: int = 0) -> FilterResult:
    """One call of the C ABI: entry is "filter_all_points3D", "filter_short_tracks", "filter_negative_depth" or
    "point_errors"."""
    L = lib()
    cams = (_Camera * max(len(m.cameras), 1))()
    for i, (model_id, width, height, params) in enumerate(m.cameras):
        p = np.asarray(params, np.float64).ravel()
        if len(p) > 16:
            raise ObservationFilterError(f"camera {i}: {len(p)} parameters")
        cams[i].model_id, cams[i].width, cams[i].height, cams[i].num_params = int(model_id), int(width), int(height), len(p)
        for k, v in enumerate(p):
            cams[i].params[k] = float(v)
    poses = np.ascontiguousarray(m.image_poses, np.float64).reshape(-1, 7)
    image_camera = np.ascontiguousarray(m.image_camera, np.int32).ravel()
    points = np.ascontiguousarray(m.points, np.float64).reshape(-1, 3)
    offsets = np.ascontiguousarray(m.obs_offsets, np.int64).ravel()
    obs_image = np.ascontiguousarray(m.obs_image, np.int32).ravel()
    obs_xy = np.ascontiguousarray(m.obs_xy, np.float64).reshape(-1, 2)
    if len(offsets) != len(points) + 1 or len(image_camera) != len(poses) or len(obs_xy) != len(obs_image):
        raise ObservationFilterError("array lengths of the flat model do not fit together")
    P, O = len(points), len(obs_image)
    cm = _Model(len(m.cameras), len(poses), P, O, C.cast(cams, C.c_void_p), _ptr(poses), _ptr(image_camera), _ptr(points),
                _ptr(offsets), _ptr(obs_image), _ptr(obs_xy))
    out = FilterResult(np.zeros(O, np.uint8), np.zeros(P, np.uint8), np.zeros(P, np.float64), np.zeros(P, np.uint32), 0)
    res = _Result(_ptr(out.obs_keep), _ptr(out.point_status), _ptr(out.point_error), _ptr(out.point_count), 0)
    opt = _Options(float(max_reproj_error), float(min_tri_angle), int(min_track_len), error_type_id(error_type), int(rules), 0)
    fn = getattr(L, "obs_" + entry)
    if entry in ("filter_all_points3D", "filter_short_tracks"):
        rc = fn(C.byref(cm), C.byref(opt), C.byref(res), C.c_int32(gpu_index))
    else:
        rc = fn(C.byref(cm), C.byref(res), C.c_int32(gpu_index))
    if rc != 0:
        raise ObservationFilterError(L.obs_last_error().decode())
    out.num_filtered = int(res.num_filtered)
    k, t = C.c_double(), C.c_double()
    L.obs_last_timing(C.byref(k), C.byref(t))
    out.kernel_ms, out.total_ms = k.value, t.value
    return out


def flatten(rec: scene.Reconstruction, point3D_ids: Optional[Iterable[int]] = None):
    """(FlatModel, point ids in flat order) of the given points of `rec` (all of them by default); ids that do not
    exist are skipped, as the reference's loops skip them."""
    cam_ids = sorted(rec.cameras)
    cam_index = {c: i for i, c in enumerate(cam_ids)}
    img_ids = sorted(rec.images)
    img_index = {im: i for i, im in enumerate(img_ids)}
    ids = list(rec.points3D) if point3D_ids is None else [p for p in dict.fromkeys(point3D_ids) if p in rec.points3D]
    offsets = np.zeros(len(ids) + 1, np.int64)
    obs_image, obs_xy = [], []
    for k, pid in enumerate(ids):
        for (im, idx) in rec.points3D[pid].track:
            obs_image.append(img_index[im])
            obs_xy.append(rec.images[im].points2D[idx].xy)
        offsets[k + 1] = len(obs_image)
    m = FlatModel(
        cameras=[(rec.cameras[c].model_id, rec.cameras[c].width, rec.cameras[c].height, rec.cameras[c].params) for c in cam_ids],
        image_poses=np.array([rec.images[im].cam_from_world for im in img_ids], np.float64).reshape(-1, 7),
        image_camera=np.array([cam_index[rec.images[im].camera_id] for im in img_ids], np.int32),
        points=np.array([rec.points3D[p].xyz for p in ids], np.float64).reshape(-1, 3),
        obs_offsets=offsets, obs_image=np.array(obs_image, np.int32), obs_xy=np.array(obs_xy, np.float64).reshape(-1, 2))
    return m, ids


def apply_result(rec: scene.Reconstruction, ids, m: FlatModel, res: FilterResult, set_error: bool = False) -> int:
    """Applies the decisions of one call to `rec`; returns the filtered-observation count."""
    off = m.obs_offsets
    for k, pid in enumerate(ids):
        if res.point_status[k] != KEPT:
            rec.DeletePoint3D(pid)
            continue
        pt = rec.points3D[pid]
        keep = res.obs_keep[off[k]:off[k + 1]]
        if not keep.all():
            for (im, idx), kp in zip(pt.track, keep):
                if not kp:
                    rec.images[im].points2D[idx].point3D_id = -1
            pt.track = [el for el, kp in zip(pt.track, keep) if kp]
        if set_error:
            pt.error = float(res.point_error[k])
    return res.num_filtered


def point3D_errors(rec: scene.Reconstruction, gpu_index: int = 0) -> dict:
    """Reconstruction::UpdatePoint3DErrors as a dict point3D_id -> error (obs_point_errors)."""
    m, ids = flatten(rec)
    res = run_flat("point_errors", m, gpu_index=gpu_index)
    return {pid: float(res.point_error[k]) for k, pid in enumerate(ids)}


class ObservationManager:
    """The filter methods of colmap::ObservationManager (sfm/observation_manager.h) on the GPU."""

    def __init__(self, reconstruction: scene.Reconstruction, gpu_index: int = 0):
        self.reconstruction_ = reconstruction
        self.gpu_index = gpu_index

    def _filter(self, point3D_ids, rules, max_reproj_error=0.0, min_tri_angle=0.0, error_type=PIXEL) -> int:
        m, ids = flatten(self.reconstruction_, point3D_ids)
        if not ids:
            return 0
        res = run_flat("filter_all_points3D", m, max_reproj_error=max_reproj_error, min_tri_angle=min_tri_angle,
                       error_type=error_type, rules=rules, gpu_index=self.gpu_index)
        return apply_result(self.reconstruction_, ids, m, res, set_error=bool(rules & RULE_REPROJ_ERROR))

    def FilterPoints3D(self, max_reproj_error: float, min_tri_angle: float, point3D_ids) -> int:
        """observation_manager.cc:353-363."""
        return self._filter(point3D_ids, RULE_REPROJ_ERROR | RULE_TRI_ANGLE, max_reproj_error, min_tri_angle)

    def FilterPoints3DInImages(self, max_reproj_error: float, min_tri_angle: float, image_ids) -> int:
        """observation_manager.cc:365-379."""
        ids = []
        for image_id in image_ids:
            ids += [p.point3D_id for p in self.reconstruction_.images[image_id].points2D if p.HasPoint3D()]
        return self.FilterPoints3D(max_reproj_error, min_tri_angle, ids)

    def FilterAllPoints3D(self, max_reproj_error: float, min_tri_angle: float) -> int:
        """observation_manager.cc:381-393."""
        return self._filter(None, RULE_REPROJ_ERROR | RULE_TRI_ANGLE, max_reproj_error, min_tri_angle)

    def FilterPoints3DWithShortTracks(self, min_track_length: int) -> int:
        """observation_manager.cc:395-407."""
        m, ids = flatten(self.reconstruction_)
        if not ids:
            return 0
        res = run_flat("filter_short_tracks", m, min_track_len=min_track_length, gpu_index=self.gpu_index)
        return apply_result(self.reconstruction_, ids, m, res)

    def FilterPoints3DWithLargeReprojectionError(self, max_error: float, point3D_ids, error_type=PIXEL) -> int:
        """observation_manager.cc:496-585."""
        return self._filter(point3D_ids, RULE_REPROJ_ERROR, max_reproj_error=max_error, error_type=error_type)

    def FilterPoints3DWithSmallTriangulationAngle(self, min_tri_angle: float, point3D_ids) -> int:
        """observation_manager.cc:435-494."""
        return self._filter(point3D_ids, RULE_TRI_ANGLE, min_tri_angle=min_tri_angle)

    def FilterObservationsWithNegativeDepth(self) -> int:
        """observation_manager.cc:409-433."""
        m, ids = flatten(self.reconstruction_)
        if not ids:
            return 0
        res = run_flat("filter_negative_depth", m, gpu_index=self.gpu_index)
        return apply_result(self.reconstruction_, ids, m, res)
