"""The statistics of a dense-stage model on MI355X (include/colmap_amd_model.h, colmap_amd/csrc/model_stats.hip).

Mirrors Model::ComputeDepthRanges / ComputeSharedPoints / ComputeTriangulationAngles / GetMaxOverlappingImages
(reference mvs/model.cc:120-277) on a colmap_amd.workspace.Model: the model is flattened, the library computes on the
GPU, and the functions return exactly the Python structures the workspace.Model methods of the same names return --
those methods stay what they are, the sequential checker. There is no CPU fallback: without the library or a device
the calls raise.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from . import _lib


class _Model(C.Structure):  # model_flat
    _fields_ = [("num_images", C.c_int32), ("reserved", C.c_int32), ("num_points", C.c_int64),
                ("num_observations", C.c_int64), ("R", C.c_void_p), ("T", C.c_void_p), ("points", C.c_void_p),
                ("track_offsets", C.c_void_p), ("track_image", C.c_void_p)]


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "model_compute_pair_statistics"):
        raise _lib.LibraryMissingError("the loaded library has no model_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    return L


class ModelStatisticsError(RuntimeError):
    pass


@dataclass
class FlatModel:
    """mvs::Model as the flat arrays of model_flat."""
    R: np.ndarray              # [I][9] float32, row-major
    T: np.ndarray              # [I][3] float32
    points: np.ndarray         # [P][3] float32
    track_offsets: np.ndarray  # [P + 1] int64
    track_image: np.ndarray    # [O] int32 image indices, in track order


@dataclass
class Timing:
    kernel_ms: float = 0.0
    total_ms: float = 0.0


last_timing = Timing()


def flatten(model) -> FlatModel:
    """The flat arrays of a workspace.Model; coordinates as the floats mvs::Model holds."""
    images, points = model.images, model.points
    offsets = np.zeros(len(points) + 1, np.int64)
    for k, pt in enumerate(points):
        offsets[k + 1] = offsets[k] + len(pt.track)
    track_image = np.fromiter((i for pt in points for i in pt.track), np.int32, count=int(offsets[-1]))
    return FlatModel(
        R=np.array([np.asarray(im.R, np.float32).ravel() for im in images], np.float32).reshape(-1, 9),
        T=np.array([np.asarray(im.T, np.float32).ravel() for im in images], np.float32).reshape(-1, 3),
        points=np.array([(pt.x, pt.y, pt.z) for pt in points], np.float32).reshape(-1, 3),
        track_offsets=offsets, track_image=track_image)


def _as_flat(model) -> FlatModel:
    return model if isinstance(model, FlatModel) else flatten(model)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class _Bound:
    """A FlatModel as a model_flat, with the arrays it points to kept alive."""

    def __init__(self, m: FlatModel):
        self.R = np.ascontiguousarray(m.R, np.float32).reshape(-1, 9)
        self.T = np.ascontiguousarray(m.T, np.float32).reshape(-1, 3)
        self.points = np.ascontiguousarray(m.points, np.float32).reshape(-1, 3)
        self.offsets = np.ascontiguousarray(m.track_offsets, np.int64).ravel()
        self.track_image = np.ascontiguousarray(m.track_image, np.int32).ravel()
        if len(self.T) != len(self.R) or len(self.offsets) != len(self.points) + 1:
            raise ModelStatisticsError("array lengths of the flat model do not fit together")
        self.num_images = len(self.R)
        self.struct = _Model(self.num_images, 0, len(self.points), len(self.track_image), _ptr(self.R), _ptr(self.T),
                             _ptr(self.points), _ptr(self.offsets), _ptr(self.track_image))


def _check(L, rc):
    if rc != 0:
        L.model_last_error.restype = C.c_char_p
        raise ModelStatisticsError(L.model_last_error().decode())
    k, t = C.c_double(), C.c_double()
    L.model_last_timing(C.byref(k), C.byref(t))
    last_timing.kernel_ms, last_timing.total_ms = k.value, t.value


def depth_ranges_flat(m: FlatModel, gpu_index: int = 0) -> np.ndarray:
    """model_compute_depth_ranges: [I][2] float32."""
    L, b = lib(), _Bound(m)
    ranges = np.zeros((b.num_images, 2), np.float32)
    _check(L, L.model_compute_depth_ranges(C.byref(b.struct), _ptr(ranges), C.c_int32(gpu_index)))
    return ranges


def pair_statistics_flat(m: FlatModel, percentile: float = 75.0, gpu_index: int = 0):
    """model_compute_pair_statistics: (row_offsets [I + 1] int64, other int32, count int32, angle float32)."""
    L, b = lib(), _Bound(m)
    handle = C.c_void_p()
    _check(L, L.model_compute_pair_statistics(C.byref(b.struct), C.c_double(percentile), C.byref(handle),
                                              C.c_int32(gpu_index)))
    try:
        n_img, n = C.c_int32(), C.c_size_t()
        L.model_pairs_size(handle, C.byref(n_img), C.byref(n))
        row_offsets = np.zeros(n_img.value + 1, np.int64)
        other, count = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        angle = np.zeros(n.value, np.float32)
        L.model_pairs_get(handle, _ptr(row_offsets), _ptr(other), _ptr(count), _ptr(angle))
    finally:
        L.model_pairs_free(handle)
    return row_offsets, other, count, angle


def max_overlapping_images_flat(m: FlatModel, num_images: int, min_triangulation_angle: float, gpu_index: int = 0):
    """model_get_max_overlapping_images: (ptr [I + 1] int64, idx int32) -- the CSR fusion_run takes. One call: idx is
    sized for the most a row can hold."""
    L, b = lib(), _Bound(m)
    per_row = max(0, min(int(num_images), b.num_images - 1))
    ptr = np.zeros(b.num_images + 1, np.int64)
    idx = np.zeros(max(1, per_row * b.num_images), np.int32)
    total = C.c_size_t()
    _check(L, L.model_get_max_overlapping_images(C.byref(b.struct), C.c_int64(int(num_images)),
                                                 C.c_double(min_triangulation_angle), _ptr(ptr), _ptr(idx),
                                                 C.byref(total), C.c_int32(gpu_index)))
    return ptr, idx[:total.value].copy()


# ---- the structures of workspace.Model -----------------------------------------------------------------------------------

def compute_depth_ranges(model, gpu_index: int = 0) -> List[Tuple[float, float]]:
    """Model::ComputeDepthRanges (model.cc:178-218)."""
    return [(float(lo), float(hi)) for lo, hi in depth_ranges_flat(_as_flat(model), gpu_index)]


def _rows(row_offsets, other, values, convert) -> list:
    return [{int(o): convert(v) for o, v in zip(other[row_offsets[i]:row_offsets[i + 1]],
                                                values[row_offsets[i]:row_offsets[i + 1]])}
            for i in range(len(row_offsets) - 1)]


def compute_shared_points(model, gpu_index: int = 0) -> List[Dict[int, int]]:
    """Model::ComputeSharedPoints (model.cc:220-235)."""
    row_offsets, other, count, _ = pair_statistics_flat(_as_flat(model), 75.0, gpu_index)
    return _rows(row_offsets, other, count, int)


def compute_triangulation_angles(model, pct: float = 75.0, gpu_index: int = 0) -> List[Dict[int, float]]:
    """Model::ComputeTriangulationAngles (model.cc:237-277); the values are np.float32 like the checker's."""
    row_offsets, other, _, angle = pair_statistics_flat(_as_flat(model), pct, gpu_index)
    return _rows(row_offsets, other, angle, np.float32)


def get_max_overlapping_images(model, num_images: int, min_triangulation_angle: float, gpu_index: int = 0) -> List[List[int]]:
    """Model::GetMaxOverlappingImages (model.cc:120-171); equal shared counts in ascending image index."""
    ptr, idx = max_overlapping_images_flat(_as_flat(model), num_images, min_triangulation_angle, gpu_index)
    return [[int(j) for j in idx[ptr[i]:ptr[i + 1]]] for i in range(len(ptr) - 1)]


class DeviceStatistics:
    """What read_patch_match_config and PatchMatchController.FromWorkspace take as `model_statistics`: the overlap
    lists and depth ranges of a model, on one device."""

    def __init__(self, gpu_index: int = 0):
        self.gpu_index = gpu_index

    def compute_depth_ranges(self, model):
        return compute_depth_ranges(model, self.gpu_index)

    def get_max_overlapping_images(self, model, num_images: int, min_triangulation_angle: float):
        return get_max_overlapping_images(model, num_images, min_triangulation_angle, self.gpu_index)
