"""SIFT feature extraction on MI355X (include/colmap_amd_sift.h, colmap_amd/csrc/sift.hip).

The GPU extractor of the reference (SiftGPUFeatureExtractor, feature/sift.cc:552-746) with the arithmetic of its VLFeat
route (SiftCPUFeatureExtractor::Extract, feature/sift.cc:138-341), thin over the C ABI. Rows come out in
vl_sift_detect's order. There is no CPU fallback: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _lib

L1_ROOT, L2 = 0, 1
NORMALIZATIONS = {"L1_ROOT": L1_ROOT, "L2": L2}
STAGES = ("pyramid", "detection", "orientation", "descriptor")
DESCRIPTOR_DIM = 128


class _Options(C.Structure):  # sift_options
    _fields_ = [("max_num_features", C.c_int32), ("first_octave", C.c_int32), ("num_octaves", C.c_int32),
                ("octave_resolution", C.c_int32), ("peak_threshold", C.c_double), ("edge_threshold", C.c_double),
                ("max_num_orientations", C.c_int32), ("upright", C.c_int32), ("normalization", C.c_int32),
                ("reserved", C.c_int32)]


DETECTION_DTYPE = np.dtype([("o", np.int32), ("ix", np.int32), ("iy", np.int32), ("is", np.int32), ("x", np.float32),
                            ("y", np.float32), ("s", np.float32), ("sigma", np.float32)])  # sift_detection


class FeatureExtractionError(RuntimeError):
    pass


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "sift_extract"):
        raise _lib.LibraryMissingError("the loaded library has no sift_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    return L


def _declare(L):
    if getattr(L, "_sift_declared", False):
        return L
    L.sift_last_error.restype = C.c_char_p
    L.sift_options_check.restype = C.c_char_p
    L.sift_destroy.restype = None
    L.sift_destroy.argtypes = [C.c_void_p]
    L.sift_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    for name in ("sift_num_features", "sift_num_reruns"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [C.c_void_p]
    for name in ("sift_num_candidates", "sift_num_detections"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [C.c_void_p, C.c_int32]
    for name in ("sift_copy_keypoints", "sift_copy_descriptors", "sift_copy_float_descriptors"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.sift_num_octaves.argtypes = [C.c_void_p]
    L.sift_octave_info.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("sift_copy_level", "sift_copy_dog", "sift_copy_gradient"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.sift_copy_detections.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.sift_copy_orientations.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
    L.sift_set_candidate_capacity.restype = None
    L.sift_set_candidate_capacity.argtypes = [C.c_void_p, C.c_int32]
    L.sift_last_timing.restype = None
    L.sift_conv_tile.restype = None
    L._sift_declared = True
    return L


def _check(L, rc):
    if rc != 0:
        raise FeatureExtractionError(L.sift_last_error().decode())


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


@dataclass
class SiftExtractionOptions:
    """feature/sift.h:41-101, the options of the built route."""
    max_num_features: int = 8192
    first_octave: int = -1
    num_octaves: int = 4
    octave_resolution: int = 3
    peak_threshold: float = 0.02 / 3.0
    edge_threshold: float = 10.0
    max_num_orientations: int = 2
    upright: bool = False
    normalization: int = L1_ROOT

    def c(self) -> _Options:
        return _Options(self.max_num_features, self.first_octave, self.num_octaves, self.octave_resolution,
                        self.peak_threshold, self.edge_threshold, self.max_num_orientations, int(self.upright),
                        int(self.normalization), 0)

    def check(self) -> str:
        """SiftExtractionOptions::Check (sift.cc:72-84) and the limits of the kernels: '' or what is wrong."""
        o = self.c()
        return _declare(lib()).sift_options_check(C.byref(o)).decode()


def default_options() -> SiftExtractionOptions:
    o = _Options()
    _declare(lib()).sift_options_init(C.byref(o))
    return SiftExtractionOptions(o.max_num_features, o.first_octave, o.num_octaves, o.octave_resolution, o.peak_threshold,
                                 o.edge_threshold, o.max_num_orientations, bool(o.upright), o.normalization)


def conv_tile(which: int) -> Tuple[int, int]:
    """Outputs of one workgroup of the column (0) or row (1) pass of the separable Gaussian: (x, y)."""
    x, y = C.c_int32(), C.c_int32()
    _declare(lib()).sift_conv_tile(C.c_int32(which), C.byref(x), C.byref(y))
    return x.value, y.value


def halo_limit() -> int:
    return int(_declare(lib()).sift_halo_limit())


def candidate_capacity(width: int, height: int, octave_resolution: int) -> int:
    return int(_declare(lib()).sift_candidate_capacity(C.c_int32(width), C.c_int32(height), C.c_int32(octave_resolution)))


def grown_capacity(count: int) -> int:
    return int(_declare(lib()).sift_grown_capacity(C.c_int32(count)))


def last_timing() -> Tuple[float, float, dict]:
    """(event ms, total ms, {stage: ms}) of the last extraction of this thread. The stage times are intervals between HIP
    events at the borders of the stages: they hold the host synchronisations, copies and gaps inside a stage, not only
    kernel time; event ms is their sum; total ms is the whole call."""
    k, t, s = C.c_double(), C.c_double(), (C.c_double * 4)()
    _declare(lib()).sift_last_timing(C.byref(k), C.byref(t), s)
    return k.value, t.value, dict(zip(STAGES, list(s)))


_libm = None


def _cosf_sinf(a: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The C library's cosf and sinf (std::cos / std::sin of a float, feature/types.cc:49-50), not numpy's."""
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in (_libm.cosf, _libm.sinf):
            f.restype = C.c_float
            f.argtypes = [C.c_float]
    a = np.asarray(a, np.float32)
    c = np.array([_libm.cosf(float(v)) for v in a], np.float32)
    s = np.array([_libm.sinf(float(v)) for v in a], np.float32)
    return c, s


def keypoints_to_affine(kp4: np.ndarray) -> np.ndarray:
    """FeatureKeypoint(x, y, scale, orientation) (feature/types.cc:43-55): [n][4] -> [n][6] = x, y, a11, a12, a21, a22,
    the form the database stores."""
    kp4 = np.asarray(kp4, np.float32).reshape(-1, 4)
    c, s = _cosf_sinf(kp4[:, 3])
    sc, ss = kp4[:, 2] * c, kp4[:, 2] * s
    return np.stack([kp4[:, 0], kp4[:, 1], sc, -ss, ss, sc], axis=1).astype(np.float32)


def rescale_keypoints(kp6: np.ndarray, scale_x: float, scale_y: float) -> np.ndarray:
    """FeatureKeypoint::Rescale (feature/types.cc:83-93) on [n][6] rows."""
    sx, sy = np.float32(scale_x), np.float32(scale_y)
    if not (sx > 0 and sy > 0):
        raise ValueError("rescale_keypoints: scales must be positive")
    out = np.array(kp6, np.float32, copy=True).reshape(-1, 6)
    out[:, 0] *= sx
    out[:, 1] *= sy
    out[:, 2] *= sx
    out[:, 3] *= sy
    out[:, 4] *= sx
    out[:, 5] *= sy
    return out


class SiftFeatureExtractor:
    """CreateSiftFeatureExtractor(...) on one GPU; reused across images of any size."""

    def __init__(self, options: Optional[SiftExtractionOptions] = None, gpu_index: int = 0):
        self._L = _declare(lib())
        self.options = options or SiftExtractionOptions()
        bad = self.options.check()
        if bad:
            raise FeatureExtractionError("SiftExtractionOptions: " + bad)
        self._h = C.c_void_p()
        _check(self._L, self._L.sift_create(C.c_int32(max(int(gpu_index), 0)), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.sift_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def extract(self, grey: np.ndarray, options: Optional[SiftExtractionOptions] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Extract(bitmap, &keypoints, &descriptors): grey uint8 [h][w] -> (keypoints [n][4] float32 = x, y, scale,
        orientation, descriptors [n][128] uint8)."""
        grey = np.ascontiguousarray(grey)
        if grey.dtype != np.uint8 or grey.ndim != 2:
            raise FeatureExtractionError("extract: a grey uint8 image [height][width] is needed")
        o = (options or self.options).c()
        _check(self._L, self._L.sift_extract(self._h, _ptr(grey), grey.shape[1], grey.shape[0], C.byref(o)))
        n = int(self._L.sift_num_features(self._h))
        kp = np.zeros((n, 4), np.float32)
        desc = np.zeros((n, DESCRIPTOR_DIM), np.uint8)
        _check(self._L, self._L.sift_copy_keypoints(self._h, _ptr(kp), n))
        _check(self._L, self._L.sift_copy_descriptors(self._h, _ptr(desc), n))
        return kp, desc

    # ---- what the tests compare
    def float_descriptors(self) -> np.ndarray:
        n = int(self._L.sift_num_features(self._h))
        out = np.zeros((n, DESCRIPTOR_DIM), np.float32)
        _check(self._L, self._L.sift_copy_float_descriptors(self._h, _ptr(out), n))
        return out

    def num_octaves(self) -> int:
        return int(self._L.sift_num_octaves(self._h))

    def octave_info(self, k: int) -> Tuple[int, int, int]:
        """(width, height, octave index o) of the k-th octave of the last extraction."""
        w, h, o = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self._L, self._L.sift_octave_info(self._h, k, C.byref(w), C.byref(h), C.byref(o)))
        return w.value, h.value, o.value

    def _plane(self, fn, k, level, channels=1):
        w, h, _ = self.octave_info(k)
        out = np.zeros((h, w) if channels == 1 else (h, w, channels), np.float32)
        _check(self._L, fn(self._h, k, level, _ptr(out)))
        return out

    def level(self, k: int, level: int) -> np.ndarray:
        return self._plane(self._L.sift_copy_level, k, level)

    def dog(self, k: int, level: int) -> np.ndarray:
        return self._plane(self._L.sift_copy_dog, k, level)

    def gradient(self, k: int, plane: int) -> np.ndarray:
        return self._plane(self._L.sift_copy_gradient, k, plane, 2)

    def num_candidates(self, k: int) -> int:
        return int(self._L.sift_num_candidates(self._h, k))

    def detections(self, k: int) -> np.ndarray:
        n = int(self._L.sift_num_detections(self._h, k))
        out = np.zeros(n, DETECTION_DTYPE)
        _check(self._L, self._L.sift_copy_detections(self._h, k, _ptr(out), n))
        return out

    def orientations(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        n = int(self._L.sift_num_detections(self._h, k))
        counts, angles = np.zeros(n, np.int32), np.zeros((n, 4), np.float64)
        _check(self._L, self._L.sift_copy_orientations(self._h, k, _ptr(counts), _ptr(angles), n))
        return counts, angles

    def set_candidate_capacity(self, capacity: int):
        """Test hook: the first candidate capacity of every octave (0: the default)."""
        self._L.sift_set_candidate_capacity(self._h, int(capacity))

    def num_reruns(self) -> int:
        return int(self._L.sift_num_reruns(self._h))


def extract_features(images: List[np.ndarray], options: Optional[SiftExtractionOptions] = None,
                     gpu_index: int = 0) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Keypoints [n][6] (the database form) and descriptors [n][128] of every grey image, on one handle."""
    out = []
    with SiftFeatureExtractor(options, gpu_index) as ex:
        for im in images:
            kp, desc = ex.extract(im)
            out.append((keypoints_to_affine(kp), desc))
    return out
