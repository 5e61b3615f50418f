"""Colour extraction on MI355X: the colours of a sparse model's 3D points from its source images
(include/colmap_amd_color.h, colmap_amd/csrc/color_extract.hip).

Mirrors (reference file:line in each docstring):
  scene/reconstruction.cc:1122-1184  Reconstruction::ExtractColorsForAllImages
  scene/reconstruction.cc:1094-1120  Reconstruction::ExtractColorsForImage
The samples and the means are computed behind the C ABI on the GPU; this module reads the images and lays the model's
observations out in slots. There is no CPU fallback: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import workspace as W
from .undistortion import read_bitmap


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "color_add_image"):
        raise _lib.LibraryMissingError("the loaded library has no color_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    L.color_last_error.restype = C.c_char_p
    L.color_create.restype = C.c_void_p
    L.color_create.argtypes = [C.c_int64, C.c_int32]
    L.color_add_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.color_finish.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.color_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.color_destroy.argtypes = [C.c_void_p]
    L.color_destroy.restype = None
    L.color_slot_layout.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 5
    L.color_timing.argtypes = [C.c_void_p] * 4
    L.color_timing.restype = None
    return L


class ColorError(RuntimeError):
    pass


def _check(rc: int):
    if rc != 0:
        raise ColorError(lib().color_last_error().decode())


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def SlotLayout(obs_point: np.ndarray, obs_image: np.ndarray, obs_point2D: np.ndarray, num_points: int
               ) -> Tuple[np.ndarray, np.ndarray]:
    """color_slot_layout (host only): -> (ptr [num_points + 1], slot [n]); CSR by point, the observations of a point in
    ascending image id, then point2D index."""
    op, oi, o2 = (np.ascontiguousarray(a, np.int64) for a in (obs_point, obs_image, obs_point2D))
    ptr, slot = np.zeros(num_points + 1, np.int64), np.zeros(len(op), np.int64)
    _check(lib().color_slot_layout(len(op), int(num_points), _ptr(op), _ptr(oi), _ptr(o2), _ptr(ptr), _ptr(slot)))
    return ptr, slot


class ColorExtractor:
    """A color_extractor handle: one slot per observation; images stream through AddImage as the host decodes them."""

    def __init__(self, num_observations: int, gpu_index: int = 0):
        self._lib = lib()
        self.num_observations = int(num_observations)
        self._h = self._lib.color_create(self.num_observations, int(gpu_index))
        if not self._h:
            raise ColorError(self._lib.color_last_error().decode())

    def AddImage(self, bitmap: np.ndarray, xy: np.ndarray, slot: np.ndarray):
        bmp = np.ascontiguousarray(bitmap, np.uint8)
        if bmp.ndim not in (2, 3):
            raise ColorError("a bitmap is (H, W) grey or (H, W, 3) RGB")
        ch = 1 if bmp.ndim == 2 else bmp.shape[2]
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        slot = np.ascontiguousarray(slot, np.int64).reshape(-1)
        if len(slot) != len(xy):
            raise ColorError("one slot per observation")
        _check(self._lib.color_add_image(self._h, _ptr(bmp), bmp.shape[1], bmp.shape[0], ch, len(xy), _ptr(xy), _ptr(slot)))

    def Finish(self, ptr: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """-> (rgb [num_points, 3] uint8, count [num_points] int32)"""
        ptr = np.ascontiguousarray(ptr, np.int64).reshape(-1)
        if len(ptr) < 1:
            raise ColorError("ptr has num_points + 1 entries")
        n = len(ptr) - 1
        rgb, count = np.zeros((n, 3), np.uint8), np.zeros(n, np.int32)
        _check(self._lib.color_finish(self._h, n, _ptr(ptr), _ptr(rgb), _ptr(count)))
        return rgb, count

    def Samples(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (rgb [num_observations, 3] float32, valid [num_observations] bool)"""
        rgb = np.zeros((self.num_observations, 3), np.float32)
        valid = np.zeros(self.num_observations, np.uint8)
        _check(self._lib.color_samples(self._h, _ptr(rgb), _ptr(valid)))
        return rgb, valid.astype(bool)

    def Timing(self) -> Tuple[float, float, float]:
        """(sample kernels ms, point kernels ms, all calls ms) of this handle so far."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._lib.color_timing(self._h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def Close(self):
        if self._h:
            self._lib.color_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Close()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


class ModelSlots:
    """The slot layout of a workspace.SparseModel: point_ids in ascending id order own ptr; per_image[image_id] is
    (point2D indices, slots) of the image's observations that have a 3D point of the model."""

    def __init__(self, model: W.SparseModel, image_ids: Optional[Sequence[int]] = None):
        self.point_ids = np.array(sorted(model.points3D), np.int64)
        ids = sorted(model.images) if image_ids is None else list(image_ids)
        obs_point, obs_image, obs_idx, kept = [], [], [], []
        for iid in ids:
            p3d = np.asarray(model.images[iid].point3D_ids, np.int64).reshape(-1)
            idx = np.nonzero(p3d != -1)[0]
            if len(idx) == 0:
                continue
            pos = np.searchsorted(self.point_ids, p3d[idx])
            pos = np.minimum(pos, max(len(self.point_ids) - 1, 0))
            known = (self.point_ids[pos] == p3d[idx]) if len(self.point_ids) else np.zeros(len(idx), bool)
            obs_point.append(pos[known])
            obs_image.append(np.full(int(known.sum()), iid, np.int64))
            obs_idx.append(idx[known])
            kept.append(iid)
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        self.obs_point, self.obs_image, self.obs_point2D = cat(obs_point), cat(obs_image), cat(obs_idx)
        self.ptr, self.slot = SlotLayout(self.obs_point, self.obs_image, self.obs_point2D, len(self.point_ids))
        self.per_image: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}
        at = 0
        for iid, part in zip(kept, obs_idx):
            self.per_image[iid] = (part, self.slot[at:at + len(part)])
            at += len(part)

    @property
    def num_observations(self) -> int:
        return len(self.slot)


def ExtractColorsForAllImages(model: W.SparseModel, image_path: str, gpu_index: int = 0) -> int:
    """Reconstruction::ExtractColorsForAllImages (scene/reconstruction.cc:1122-1184) on a workspace.SparseModel, in
    place: every point becomes the rounded mean of its bilinear samples over the images that can be read; a missing or
    unreadable file warns and is skipped; a point without a sample becomes black. -> the number of images read."""
    slots = ModelSlots(model)
    num_read = 0
    with ColorExtractor(slots.num_observations, gpu_index) as ex:
        for iid in sorted(model.images):
            image = model.images[iid]
            path = os.path.join(image_path, image.name)
            bmp = read_bitmap(path)
            if bmp is None:
                print(f"W Could not read image {image.name} at path {path}")
                continue
            num_read += 1
            if iid not in slots.per_image:
                continue
            idx, slot = slots.per_image[iid]
            ex.AddImage(bmp, np.asarray(image.xys, np.float64).reshape(-1, 2)[idx], slot)
        rgb, _ = ex.Finish(slots.ptr)
    for pid, colour in zip(slots.point_ids, rgb):  # every point of the model is rewritten (:1172-1183)
        model.points3D[int(pid)].rgb = (int(colour[0]), int(colour[1]), int(colour[2]))
    return num_read


def _cast_u8(values: np.ndarray) -> np.ndarray:
    """BitmapColor<float>::Cast<uint8_t> (sensor/bitmap.h:216-223): round half away from zero, clamp."""
    v = np.asarray(values, np.float32)
    r = np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))
    return np.clip(r, 0, 255).astype(np.uint8)


def ExtractColorsForImage(model: W.SparseModel, image_id: int, image_path: str, gpu_index: int = 0) -> bool:
    """Reconstruction::ExtractColorsForImage (scene/reconstruction.cc:1094-1120): False when the file cannot be read.
    The samples come from the device; the host applies the rule in point2D order: only a point whose colour is currently
    (0, 0, 0) takes Cast<uint8_t> of its sample (:1104-1117)."""
    image = model.images[image_id]
    bmp = read_bitmap(os.path.join(image_path, image.name))
    if bmp is None:
        return False
    p3d = np.asarray(image.point3D_ids, np.int64).reshape(-1)
    idx = np.array([i for i in np.nonzero(p3d != -1)[0] if int(p3d[i]) in model.points3D], np.int64)
    if len(idx) == 0:
        return True
    with ColorExtractor(len(idx), gpu_index) as ex:
        ex.AddImage(bmp, np.asarray(image.xys, np.float64).reshape(-1, 2)[idx], np.arange(len(idx), dtype=np.int64))
        rgb, valid = ex.Samples()
    colours = _cast_u8(rgb)
    for k, i in enumerate(idx):  # point2D order
        point = model.points3D[int(p3d[i])]
        if tuple(int(c) for c in point.rgb) == (0, 0, 0) and valid[k]:
            point.rgb = (int(colours[k, 0]), int(colours[k, 1]), int(colours[k, 2]))
    return True
