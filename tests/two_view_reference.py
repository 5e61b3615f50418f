"""The numpy checker of two-view geometry estimation: a sequential restatement, in float64 numpy, of what
colmap_amd/csrc/two_view_solvers.h, two_view_plan.h and two_view.hip compute.

Bit-exact restatements (same operations in the same order): the sample draw, the three residuals, residual_sum in the
device's documented order (ONE accumulator adds the inlier residuals in match order).
Independent restatements (other algorithms, agreeing to rounding): the minimal solvers with numpy.linalg.svd,
numpy.linalg.solve and numpy.roots, the local estimators with numpy.linalg.svd, and on top of them the whole LORANSAC
(optim/loransac.h:131-393) and the decisions of estimators/two_view_geometry.cc:180-382, 552-640, 1503-1584.
`f7_mp` / `h4_mp` solve a sample in 50-digit mpmath arithmetic: the floor against which solver tolerances are measured.
"""
import math

import numpy as np

KIND_F, KIND_H, KIND_T = 0, 1, 2
MIN_SAMPLES = {KIND_F: 7, KIND_H: 4, KIND_T: 1}
LOCAL_MIN_SAMPLES = {KIND_F: 8, KIND_H: 4, KIND_T: 1}
DBL_MAX = float(np.finfo(np.float64).max)
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15

UNDEFINED, DEGENERATE, CALIBRATED, UNCALIBRATED, PLANAR, PANORAMIC, PLANAR_OR_PANORAMIC, WATERMARK, MULTIPLE = range(9)


# ---- the sample draw -------------------------------------------------------------------------------------------------

def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_key(seed, stream_id, kind, trial):
    h = mix64((0 if seed < 0 else seed) + GOLDEN)
    h = mix64(h ^ (stream_id & M64))
    h = mix64(h ^ kind)
    return mix64(h ^ trial)


def draw_sample(seed, stream_id, kind, trial, n):
    key, c, idx = sample_key(seed, stream_id, kind, trial), 0, []
    while len(idx) < MIN_SAMPLES[kind]:
        v = mix64(key + c * GOLDEN) % n
        c += 1
        if v not in idx:
            idx.append(v)
    return np.array(idx, np.uint32)


def iteration_stream(stream_id, it):
    return stream_id & M64 if it == 0 else mix64((stream_id & M64) ^ mix64(it))


# ---- residuals, operation by operation ---------------------------------------------------------------------------------

def residuals(kind, M, pts):
    """pts [n][4]; every sum left to right, as two_view_solvers.h."""
    M = np.asarray(M, np.float64).ravel()
    pts = np.asarray(pts, np.float64).reshape(-1, 4)
    x1, y1, x2, y2 = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    with np.errstate(all="ignore"):
        if kind == KIND_F:
            l0 = M[0] * x1 + M[1] * y1 + M[2]
            l1 = M[3] * x1 + M[4] * y1 + M[5]
            l2 = M[6] * x1 + M[7] * y1 + M[8]
            num = x2 * l0 + y2 * l1 + l2
            d0 = x2 * M[0] + y2 * M[3] + M[6]
            d1 = x2 * M[1] + y2 * M[4] + M[7]
            denom = d0 * d0 + d1 * d1 + l0 * l0 + l1 * l1
            return np.where(denom == 0.0, DBL_MAX, num * num / denom)
        if kind == KIND_H:
            pd0 = M[0] * x1 + M[1] * y1 + M[2]
            pd1 = M[3] * x1 + M[4] * y1 + M[5]
            pd2 = M[6] * x1 + M[7] * y1 + M[8]
            inv = 1.0 / pd2
            dd0 = x2 - pd0 * inv
            dd1 = y2 - pd1 * inv
            return dd0 * dd0 + dd1 * dd1
        dx = x2 - x1 - M[0]
        dy = y2 - y1 - M[1]
        return dx * dx + dy * dy


def support(kind, M, pts, max_error):
    """(num_inliers, residual_sum, mask): InlierSupportMeasurer::Evaluate with max_residual = max_error^2."""
    r = residuals(kind, M, pts)
    with np.errstate(invalid="ignore"):
        mask = r <= max_error * max_error
    inl = r[mask]
    total = float(np.cumsum(inl)[-1]) if len(inl) else 0.0  # cumsum adds one by one, in order
    return int(mask.sum()), total, mask.astype(np.uint8)


def is_left_better(l, r):
    return l[0] > r[0] or (l[0] == r[0] and l[1] < r[1])


# ---- minimal solvers ---------------------------------------------------------------------------------------------------

def _f7_system(p):
    x1, y1, x2, y2 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    one = np.ones_like(x1)
    return np.stack([x1 * x2, x1 * y2, x1, y1 * x2, y1 * y2, y1, x2, y2, one], 1)  # unknown 3 c + r = F(r, c)


def f7_cubic(f1, f2):
    """Coefficients (descending) of det(l f1 + f2) by interpolation-free expansion: evaluated exactly as a polynomial
    through four points would be ill-conditioned, so expand by multilinearity of the determinant."""
    A, B = f1.reshape(3, 3), f2.reshape(3, 3)
    def d(c0, c1, c2):
        return np.linalg.det(np.stack([c0, c1, c2]))
    c3 = d(A[0], A[1], A[2])
    c2 = d(B[0], A[1], A[2]) + d(A[0], B[1], A[2]) + d(A[0], A[1], B[2])
    c1 = d(A[0], B[1], B[2]) + d(B[0], A[1], B[2]) + d(B[0], B[1], A[2])
    c0 = d(B[0], B[1], B[2])
    return np.array([c3, c2, c1, c0])


def solve_f7(p):
    """Models [m][9] row-major, unit norm, of 7 matches p [7][4] (fundamental_matrix.cc:47-114 with another null-space
    basis and numpy.roots for the cubic)."""
    A = _f7_system(np.asarray(p, np.float64))
    _, s, vt = np.linalg.svd(A)
    if s[6] <= 1e-13 * s[0]:
        return np.zeros((0, 9))
    f2 = vt[8]
    f1 = vt[7] - f2
    c = f7_cubic(f1, f2)
    if abs(c[0]) < 1e-16:
        return np.zeros((0, 9))
    roots = np.roots(c)
    out = []
    for r in roots:
        if abs(r.imag) > 1e-9 * max(1.0, abs(r.real)):
            continue
        f = f1 * r.real + f2
        f = f / np.linalg.norm(f)
        out.append(f.reshape(3, 3).T.ravel())  # f is column-major F
    return np.array(out).reshape(-1, 9)


def cubic_condition(p):
    """(|leading coefficient|, smallest relative gap between two roots of the cubic) of a 7-point sample: the case
    lists keep away from a zero leading coefficient and from a double root."""
    A = _f7_system(np.asarray(p, np.float64))
    _, _, vt = np.linalg.svd(A)
    c = f7_cubic(vt[7] - vt[8], vt[8])
    roots = np.roots(c)
    gap = min(abs(roots[i] - roots[j]) for i in range(3) for j in range(i)) / max(1.0, max(abs(roots)))
    return abs(c[0]), float(gap)


def solve_h4(p):
    """Models [m][9] of 4 matches (homography_matrix.cc:45-96, the 4-point branch)."""
    p = np.asarray(p, np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i, (x1, y1, x2, y2) in enumerate(p):
        A[2 * i] = [x1, y1, 1, 0, 0, 0, -x2 * x1, -x2 * y1]
        A[2 * i + 1] = [0, 0, 0, x1, y1, 1, -y2 * x1, -y2 * y1]
        b[2 * i], b[2 * i + 1] = x2, y2
    try:
        h = np.append(np.linalg.solve(A, b), 1.0)
    except np.linalg.LinAlgError:
        return np.zeros((0, 9))
    if np.isnan(h).any() or abs(np.linalg.det(h.reshape(3, 3))) < 1e-8:
        return np.zeros((0, 9))
    return h.reshape(1, 9)


def solve_t1(p):
    p = np.asarray(p, np.float64).reshape(-1, 4)
    return np.array([[p[0, 2] - p[0, 0], p[0, 3] - p[0, 1], 0, 0, 0, 0, 0, 0, 0]], np.float64)


def solve_minimal(kind, p):
    return solve_f7(p) if kind == KIND_F else solve_h4(p) if kind == KIND_H else solve_t1(p)


def f7_mp(p, digits=50):
    """The 7-point models in `digits`-digit arithmetic, [m][9] float64 rounded at the end."""
    import mpmath as mp
    with mp.workdps(digits):
        A = mp.matrix(7, 9)
        for i, (x1, y1, x2, y2) in enumerate(np.asarray(p, np.float64).tolist()):
            x1, y1, x2, y2 = mp.mpf(x1), mp.mpf(y1), mp.mpf(x2), mp.mpf(y2)
            row = [x1 * x2, x1 * y2, x1, y1 * x2, y1 * y2, y1, x2, y2, mp.mpf(1)]
            for c in range(9):
                A[i, c] = row[c]
        # null space: Gauss-Jordan with full pivoting
        perm = list(range(9))
        for k in range(7):
            pr, pc = max(((r, c) for r in range(k, 7) for c in range(k, 9)), key=lambda rc: abs(A[rc[0], rc[1]]))
            for c in range(9):
                A[k, c], A[pr, c] = A[pr, c], A[k, c]
            for r in range(7):
                A[r, k], A[r, pc] = A[r, pc], A[r, k]
            perm[k], perm[pc] = perm[pc], perm[k]
            for r in range(7):
                if r != k:
                    f = A[r, k] / A[k, k]
                    for c in range(k, 9):
                        A[r, c] -= f * A[k, c]
        null = []
        for j in (7, 8):
            v = [mp.mpf(0)] * 9
            v[perm[j]] = mp.mpf(1)
            for i in range(7):
                v[perm[i]] = -A[i, j] / A[i, i]
            null.append(v)
        f2 = null[1]
        f1 = [a - b for a, b in zip(null[0], f2)]

        def det(f):
            return mp.det(mp.matrix([[f[0], f[1], f[2]], [f[3], f[4], f[5]], [f[6], f[7], f[8]]]))
        # det(l f1 + f2) is a cubic in l: fit it through four exact evaluations
        xs = [mp.mpf(v) for v in (-1, 0, 1, 2)]
        ys = [det([a * x + b for a, b in zip(f1, f2)]) for x in xs]
        V = mp.matrix([[x ** 3, x ** 2, x, 1] for x in xs])
        c = mp.lu_solve(V, mp.matrix(ys))
        roots = mp.polyroots([c[0], c[1], c[2], c[3]], maxsteps=200, extraprec=200)
        out = []
        for r in roots:
            if abs(mp.im(r)) > mp.mpf(10) ** (-digits // 2):
                continue
            f = [a * mp.re(r) + b for a, b in zip(f1, f2)]
            n = mp.sqrt(sum(v * v for v in f))
            F = [[f[3 * cc + rr] / n for cc in range(3)] for rr in range(3)]
            out.append([float(v) for row in F for v in row])
        return np.array(out).reshape(-1, 9)


def h4_mp(p, digits=50):
    import mpmath as mp
    with mp.workdps(digits):
        A, b = mp.matrix(8, 8), mp.matrix(8, 1)
        for i, (x1, y1, x2, y2) in enumerate(np.asarray(p, np.float64).tolist()):
            x1, y1, x2, y2 = mp.mpf(x1), mp.mpf(y1), mp.mpf(x2), mp.mpf(y2)
            r0 = [x1, y1, 1, 0, 0, 0, -x2 * x1, -x2 * y1]
            r1 = [0, 0, 0, x1, y1, 1, -y2 * x1, -y2 * y1]
            for c in range(8):
                A[2 * i, c], A[2 * i + 1, c] = r0[c], r1[c]
            b[2 * i], b[2 * i + 1] = x2, y2
        h = mp.lu_solve(A, b)
        return np.array([[float(h[k]) for k in range(8)] + [1.0]])


def model_distance(a, b, up_to_sign=True):
    """Relative distance of two models; F is defined up to sign (unit norm), H is normalised by h22 = 1."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    d = np.linalg.norm(a - b)
    if up_to_sign:
        d = min(d, np.linalg.norm(a + b))
    return d / max(np.linalg.norm(b), 1e-300)


# ---- local estimators --------------------------------------------------------------------------------------------------

def _normalize(xy):
    c = xy.mean(0)
    rms = math.sqrt(((xy - c) ** 2).sum(1).mean())
    f = math.sqrt(2.0) / rms
    T = np.array([[f, 0, -f * c[0]], [0, f, -f * c[1]], [0, 0, 1]])
    return f * xy + T[:2, 2], T


def estimate_f8(p):
    p = np.asarray(p, np.float64)
    if len(p) < 8:
        return None
    with np.errstate(all="ignore"):
        a, T1 = _normalize(p[:, :2])
        b, T2 = _normalize(p[:, 2:])
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            return np.full(9, np.nan)
    one = np.ones(len(p))
    A = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1], one], 1)
    Q = np.linalg.svd(A)[2][8].reshape(3, 3)
    U, s, Vt = np.linalg.svd(Q)
    s[2] = 0.0
    return (T2.T @ (U @ np.diag(s) @ Vt) @ T1).ravel()


def estimate_h_dlt(p):
    p = np.asarray(p, np.float64)
    A = np.zeros((2 * len(p), 9))
    for i, (x1, y1, x2, y2) in enumerate(p):
        A[2 * i] = [x1, y1, 1, 0, 0, 0, -x2 * x1, -x2 * y1, -x2]
        A[2 * i + 1] = [0, 0, 0, x1, y1, 1, -y2 * x1, -y2 * y1, -y2]
    _, s, vt = np.linalg.svd(A)
    s = np.concatenate([s, np.zeros(9 - len(s))])
    if (s > s[0] * max(A.shape) * np.finfo(np.float64).eps).sum() < 8:
        return None
    h = vt[8]
    if abs(np.linalg.det(h.reshape(3, 3))) < 1e-8:
        return None
    return h.copy()


def estimate_t_mean(p):
    p = np.asarray(p, np.float64)
    m = p.mean(0)
    return np.array([m[2] - m[0], m[3] - m[1], 0, 0, 0, 0, 0, 0, 0])


def local_estimate(kind, p):
    return estimate_f8(p) if kind == KIND_F else estimate_h_dlt(p) if kind == KIND_H else estimate_t_mean(p)


# ---- RANSAC ------------------------------------------------------------------------------------------------------------

NO_LIMIT = (1 << 64) - 1


def compute_num_trials(num_inliers, num_samples, confidence, multiplier, min_samples):
    prob_failure = 1 - confidence
    if prob_failure <= 0:
        return NO_LIMIT
    prob_inlier = 1.0
    for i in range(min_samples):
        prob_inlier *= float((num_inliers - i) & M64) / float((num_samples - i) & M64)
    prob_outlier = 1 - prob_inlier
    if prob_outlier <= 0:
        return 1
    if prob_outlier == 1.0:
        return NO_LIMIT
    v = math.ceil(math.log(prob_failure) / math.log(prob_outlier) * multiplier)
    return NO_LIMIT if v >= 2 ** 64 else max(int(v), 0)


def clamped_max_num_trials(o, ratio, min_samples):
    dyn = compute_num_trials(int(ratio * 100000), 100000, o["confidence"], o["dyn_num_trials_multiplier"], min_samples)
    return min(o["max_num_trials"], dyn)


def ransac_options(**kw):
    o = dict(max_error=4.0, min_inlier_ratio=0.25, confidence=0.999, dyn_num_trials_multiplier=3.0, min_num_trials=100,
             max_num_trials=10000, random_seed=-1)
    o.update(kw)
    return o


def loransac(kind, pts, stream_id, o, ratio=None, minimal=solve_minimal):
    """optim/loransac.h:131-393 on one point set. Returns a dict like tvg_report."""
    pts = np.asarray(pts, np.float64).reshape(-1, 4)
    n, k = len(pts), MIN_SAMPLES[kind]
    rep = dict(success=False, has_model=False, num_trials=0, num_inliers=0, residual_sum=DBL_MAX, model=np.zeros(9),
               inlier_mask=np.zeros(n, np.uint8))
    if n < k:
        return rep
    max_trials = clamped_max_num_trials(o, o["min_inlier_ratio"] if ratio is None else ratio, k)
    dyn_max, best, best_model = max_trials, (0, DBL_MAX), None
    t, stop = 0, False
    while True:
        if t >= max_trials:
            t += 1
            break
        idx = draw_sample(o["random_seed"], stream_id, kind, t, n)
        for model in minimal(kind, pts[idx]):
            s = support(kind, model, pts, o["max_error"])
            if is_left_better(s, best):
                lbest, lmodel = s, model
                if s[0] > k and s[0] >= LOCAL_MIN_SAMPLES[kind]:
                    mask = s[2]
                    for _ in range(10):
                        m = local_estimate(kind, pts[mask.astype(bool)])
                        if m is None:
                            break
                        ls = support(kind, m, pts, o["max_error"])
                        if not is_left_better(ls, lbest):
                            break
                        lbest, lmodel, mask = ls, m, ls[2]
                if is_left_better(lbest, best):
                    best, best_model = lbest, lmodel
                    dyn_max = compute_num_trials(best[0], n, o["confidence"], o["dyn_num_trials_multiplier"], k)
            if t >= dyn_max and t >= o["min_num_trials"]:
                stop = True
                break
        t += 1
        if stop:
            break
    rep["num_trials"] = t
    if best_model is None:
        return rep
    rep.update(has_model=True, num_inliers=best[0], residual_sum=best[1], model=np.asarray(best_model, np.float64))
    if best[0] < k:
        return rep
    rep["success"] = True
    rep["inlier_mask"] = support(kind, best_model, pts, o["max_error"])[2]
    return rep


# ---- decisions ---------------------------------------------------------------------------------------------------------

def tvg_options(**kw):
    o = dict(min_num_inliers=15, max_H_inlier_ratio=0.8, watermark_min_inlier_ratio=0.7, watermark_border_size=0.1,
             detect_watermark=True, multiple_ignore_watermark=True, watermark_detection_max_error=4.0,
             filter_stationary_matches=False, stationary_matches_max_error=4.0, force_H_use=False, multiple_models=False,
             ransac=ransac_options())
    o.update(kw)
    return o


def detect_watermark(size1, size2, pts, mask, num_inliers, stream_id, o):
    """DetectWatermarkMatches; size = (width, height)."""
    if num_inliers == 0:
        return False
    inl = pts[mask.astype(bool)]
    b1 = o["watermark_border_size"] * math.sqrt(size1[0] ** 2 + size1[1] ** 2)
    b2 = o["watermark_border_size"] * math.sqrt(size2[0] ** 2 + size2[1] ** 2)
    in1 = (inl[:, 0] >= b1) & (inl[:, 1] >= b1) & (inl[:, 0] <= size1[0] - b1) & (inl[:, 1] <= size1[1] - b1)
    in2 = (inl[:, 2] >= b2) & (inl[:, 3] >= b2) & (inl[:, 2] <= size2[0] - b2) & (inl[:, 3] <= size2[1] - b2)
    if (~in1 & ~in2).sum() / num_inliers < o["watermark_min_inlier_ratio"]:
        return False
    r = dict(o["ransac"], max_error=o["watermark_detection_max_error"], min_inlier_ratio=o["watermark_min_inlier_ratio"])
    rep = loransac(KIND_T, inl, stream_id, r)
    return rep["num_inliers"] / num_inliers >= o["watermark_min_inlier_ratio"]


def estimate_single(size1, size2, pts, stream_id, o, forced_h=False):
    """EstimateUncalibratedTwoViewGeometry / EstimateCalibratedHomography: (config, mask over pts)."""
    n, none = len(pts), np.zeros(len(pts), np.uint8)
    if n < o["min_num_inliers"]:
        return DEGENERATE, none
    if forced_h:
        H = loransac(KIND_H, pts, stream_id, o["ransac"])
        if not H["success"] or H["num_inliers"] < o["min_num_inliers"]:
            return DEGENERATE, none
        config, mask, num = PLANAR_OR_PANORAMIC, H["inlier_mask"], H["num_inliers"]
    else:
        F = loransac(KIND_F, pts, stream_id, o["ransac"])
        ratio = max(o["ransac"]["min_inlier_ratio"], o["max_H_inlier_ratio"] * F["num_inliers"] / n)
        H = loransac(KIND_H, pts, stream_id, o["ransac"], ratio)
        if (not F["success"] and not H["success"]) or (F["num_inliers"] < o["min_num_inliers"] and H["num_inliers"] < o["min_num_inliers"]):
            return DEGENERATE, none
        hf = H["num_inliers"] / F["num_inliers"] if F["num_inliers"] else math.inf
        mask, num = F["inlier_mask"], F["num_inliers"]
        if hf > o["max_H_inlier_ratio"]:
            config = PLANAR_OR_PANORAMIC
            if H["num_inliers"] >= F["num_inliers"]:
                mask, num = H["inlier_mask"], H["num_inliers"]
        else:
            config = UNCALIBRATED
    if o["detect_watermark"] and detect_watermark(size1, size2, pts, mask, num, stream_id, o):
        config = WATERMARK
    return config, mask


def estimate_two_view_geometry(size1, size2, pts, stream_id, o, forced_h=False):
    """EstimateTwoViewGeometry on the built routes: (config, mask over pts)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 4)
    keep = np.arange(len(pts))
    if o["filter_stationary_matches"]:
        d = (pts[:, 0] - pts[:, 2]) ** 2 + (pts[:, 1] - pts[:, 3]) ** 2
        keep = keep[~(d <= o["stationary_matches_max_error"] ** 2)]
    full = np.zeros(len(pts), np.uint8)
    if not o["multiple_models"]:
        config, mask = estimate_single(size1, size2, pts[keep], stream_id, o, forced_h)
        full[keep[mask.astype(bool)]] = 1
        return config, full
    found, it = [], 0
    while True:
        config, mask = estimate_single(size1, size2, pts[keep], iteration_stream(stream_id, it), o, forced_h)
        if config == DEGENERATE:
            break
        m = np.zeros(len(pts), np.uint8)
        m[keep[mask.astype(bool)]] = 1
        keep = keep[~mask.astype(bool)]
        if not (o["multiple_ignore_watermark"] and config == WATERMARK):
            found.append((config, m))
        it += 1
    if not found:
        return DEGENERATE, full
    if len(found) == 1:
        return found[0]
    for _, m in found:
        full |= m
    return MULTIPLE, full
