"""CPU checker of colour extraction (tests only): numpy, written from the reference's sources (scene/reconstruction.cc:
1094-1184, sensor/bitmap.cc InterpolateBilinear) and not from colmap_amd/csrc/color_extract.hip: the double interpolant
narrowed to float32, the per-point sums in slot order in double, std::round, the cast."""
from __future__ import annotations

import numpy as np


def sample(bitmap, xy):
    """Bitmap::InterpolateBilinear(x - 1/2, y - 1/2) of an (H, W) grey or (H, W, 3) RGB uint8 image read as RGB:
    -> (rgb float32 [n, 3], valid bool [n]); invalid rows are 0."""
    img = np.asarray(bitmap, np.uint8)
    if img.ndim == 2:
        img = np.repeat(img[..., None], 3, -1)   # Bitmap::Read(as_rgb = true)
    src = img.astype(np.float64)
    H, W = src.shape[:2]
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = xy[:, 0] - 0.5, xy[:, 1] - 0.5
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(x), np.floor(y)
        valid = (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)   # NaN compares false
    xi, yi = np.where(valid, x0, 0).astype(np.int64), np.where(valid, y0, 0).astype(np.int64)
    xj, yj = np.minimum(xi + 1, W - 1), np.minimum(yi + 1, H - 1)
    dx, dy = np.where(valid, x - x0, 0.0)[:, None], np.where(valid, y - y0, 0.0)[:, None]
    dx_1, dy_1 = 1.0 - dx, 1.0 - dy
    v0 = dx_1 * src[yi, xi] + dx * src[yi, xj]
    v1 = dx_1 * src[yj, xi] + dx * src[yj, xj]
    out = (dy_1 * v0 + dy * v1).astype(np.float32)
    out[~valid] = 0.0
    return out, valid


def cround(x):
    """std::round: half away from zero."""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def point_colours(rgb, valid, ptr, half_tol=1e-4):
    """The merge and the final loop of ExtractColorsForAllImages (:1162-1183) over slot ranges:
    -> (colours uint8 [P, 3], count int32 [P], near_half bool [P, 3]: the double mean of a channel lies within half_tol
    of a half-integer, where one ulp of a sample may flip the rounding)."""
    ptr = np.asarray(ptr, np.int64)
    P = len(ptr) - 1
    colours, count = np.zeros((P, 3), np.uint8), np.zeros(P, np.int32)
    near_half = np.zeros((P, 3), bool)
    for p in range(P):
        total = np.zeros(3, np.float64)
        for s in range(ptr[p], ptr[p + 1]):   # slot order
            if valid[s]:
                total += rgb[s].astype(np.float64)
                count[p] += 1
        if count[p]:
            mean = total / count[p]
            colours[p] = cround(mean).astype(np.uint8)
            near_half[p] = np.abs(mean - np.floor(mean) - 0.5) < half_tol
    return colours, count, near_half


def slot_layout(obs_point, obs_image, obs_point2D, num_points):
    """CSR by point; inside a point ascending image id, then point2D index -> (ptr, slot)."""
    obs_point, obs_image, obs_point2D = (np.asarray(a, np.int64) for a in (obs_point, obs_image, obs_point2D))
    order = np.lexsort((obs_point2D, obs_image, obs_point))
    slot = np.empty(len(order), np.int64)
    slot[order] = np.arange(len(order))
    ptr = np.zeros(num_points + 1, np.int64)
    np.add.at(ptr, obs_point + 1, 1)
    return np.cumsum(ptr), slot
