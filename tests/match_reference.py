"""Checker and case generator of descriptor matching (colmap_amd/csrc/feature_match.hip, match_plan.h): a restatement in
numpy of the reference's brute-force matcher (feature/sift.cc:772-864, 967-1004). The product is int32 and exact, the
selection is a plain scan over the columns in the reference's order, and the thresholds go through ctypes to the C
library's acosf -- the function the host plan calls --, so every comparison with the device path is for equality."""
import ctypes
import ctypes.util
import functools

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.acosf.restype = ctypes.c_float
_libm.acosf.argtypes = [ctypes.c_float]

INV_SQ_NORM = np.float32(1.0 / (512.0 * 512.0))


def dots(A, B):
    """[n1][n2] int32; a dot is at most 128 * 255^2 < 2^24."""
    return A.astype(np.int32) @ B.astype(np.int32).T


def select(D):
    """[rows][3] int32 (idx, best, second) of FindBestMatchesOneWayBruteForce's scan (sift.cc:783-796), all rows at once,
    the columns in order."""
    n = D.shape[0]
    best, second, idx = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for j in range(D.shape[1]):
        d = D[:, j]
        gt = d > best
        mid = ~gt & (d > second)
        second = np.where(gt, best, np.where(mid, d, second))
        idx = np.where(gt, np.int32(j), idx)
        best = np.where(gt, d, best)
    return np.stack([idx, best, second], axis=1).astype(np.int32)


def acosf(x):
    return np.float32(_libm.acosf(ctypes.c_float(float(x))))


def decide(sel, max_ratio=0.8, max_distance=0.7):
    """The matched column or -1 per row (sift.cc:798-822), in float like the reference."""
    out = np.full(len(sel), -1, np.int32)
    ratio, dist = np.float32(max_ratio), np.float32(max_distance)
    for i, (idx, best, second) in enumerate(sel):
        if idx < 0:
            continue
        d1 = acosf(min(INV_SQ_NORM * np.float32(best), np.float32(1.0)))
        if d1 > dist:
            continue
        d2 = acosf(min(INV_SQ_NORM * np.float32(second), np.float32(1.0)))
        if d1 >= ratio * d2:
            continue
        out[i] = idx
    return out


def cross(m12, m21, cross_check=True, min_num_inliers=15):
    """FindBestMatchesBruteForce (sift.cc:828-864) and the controller's cut: [n][2] uint32."""
    rows = [(i, j) for i, j in enumerate(m12) if j >= 0 and (not cross_check or m21[j] == i)]
    if len(rows) < min_num_inliers:
        rows = []
    return np.array(rows, np.uint32).reshape(-1, 2)


def match(A, B, max_ratio=0.8, max_distance=0.7, cross_check=True, min_num_inliers=15, max_num_matches=32768):
    """(matches, sel12, sel21) of one pair."""
    A, B = A[:max_num_matches], B[:max_num_matches]
    D = dots(A, B)
    sel12, sel21 = select(D), select(D.T)
    m = cross(decide(sel12, max_ratio, max_distance), decide(sel21, max_ratio, max_distance), cross_check, min_num_inliers)
    return m, sel12, sel21


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------

def descriptors(rng, n):
    """Gamma-distributed non-negative vectors scaled to norm 512 and clipped to 255, like SIFT's normalised histograms."""
    g = rng.gamma(0.7, 1.0, size=(n, 128))
    g *= 512.0 / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def pair(n1, n2, seed):
    """A of n1 rows; B of n2 rows. With m = min(n1, n2): m / 2 rows of B are noisy copies of distinct rows of A (sigma
    per row uniform in 5..70: from a sure match to one beyond max_distance), m / 5 are exact copies of further distinct
    rows, half of those sources twice over (a doubled maximum, which the ratio test must reject), the rest are
    distractors; B is permuted."""
    rng = np.random.default_rng(seed)
    A = descriptors(rng, n1)
    m = min(n1, n2)
    n_noisy, n_exact = m // 2, m // 5
    order = rng.permutation(n1)
    sigma = rng.uniform(5.0, 70.0, size=(n_noisy, 1))
    noisy = np.clip(np.rint(A[order[:n_noisy]].astype(np.float64) + sigma * rng.standard_normal((n_noisy, 128))), 0, 255)
    singles = -(-2 * n_exact // 3)                         # sources; the first n_exact - singles of them appear twice
    chosen = order[n_noisy:n_noisy + singles]
    exact = A[np.concatenate([chosen, chosen[:n_exact - singles]])]
    B = np.concatenate([noisy.astype(np.uint8), exact, descriptors(rng, n2 - n_noisy - n_exact)])
    return A, np.ascontiguousarray(B[rng.permutation(n2)])


@functools.lru_cache(maxsize=None)
def case(n1, n2, seed=1):
    """(A, B, sel12, sel21) computed once and shared; the arrays are read-only."""
    A, B = pair(n1, n2, seed)
    D = dots(A, B)
    out = (A, B, select(D), select(D.T))
    for a in out:
        a.setflags(write=False)
    return out


def asymmetric(n1=37, n2=53):
    """Exact-integer sets that are not symmetric in anything: a row <-> column swap or a wrong operand map shows."""
    i, k = np.arange(n1)[:, None], np.arange(128)[None, :]
    j = np.arange(n2)[:, None]
    return ((3 * i + 5 * k) % 251).astype(np.uint8), ((7 * j + 11 * k + 1) % 256).astype(np.uint8)


def extremes():
    """Rows of all 0, all 255 and alternating 0 / 255 (both phases), on both sides."""
    alt = np.tile(np.array([0, 255], np.uint8), 64)
    A = np.stack([np.zeros(128, np.uint8), np.full(128, 255, np.uint8), alt, alt[::-1].copy(), np.full(128, 1, np.uint8)])
    B = np.stack([np.full(128, 255, np.uint8), alt[::-1].copy(), np.zeros(128, np.uint8), alt, np.full(128, 255, np.uint8),
                  np.zeros(128, np.uint8)])
    return A, B
