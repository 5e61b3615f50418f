"""Times geometric verification (include/colmap_amd_tvg.h) on synthetic image pairs: 1000 matches each, exact inliers
of a two-camera set-up plus uniformly random outliers, at inlier ratios 0.3 and 0.7. Runs on the GPU only (there is no
CPU path to time). Not part of bench.py.

    python scripts/bench_geometric_verification.py [--pairs 512] [--out profiles/geometric_verification_bench_mi355x.json]

Reports, per inlier ratio,
  * pairs per second of tvg_verify_pairs (F search, H search, decisions) by whole-call time, with kernel and total ms from
    tvg_last_timing and the number of models scored;
  * scored (model x match) residuals per second by kernel time and by whole-call time;
  * as context only, the seconds the numpy checker (tests/two_view_reference.py) takes for --checker-pairs of the same pairs.
Every figure comes from a warm-up call followed by a timed window of at least --window seconds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from colmap_amd import two_view_geometry as TV  # noqa: E402

W, H = 1000, 800
K = np.array([[800.0, 0, 500.0], [0, 800.0, 400.0], [0, 0, 1]])


def make_pair(n, inlier_ratio, rng):
    """n matches: round(n * ratio) exact projections of random points into two cameras of a random relative pose, the
    rest uniformly random in both images."""
    n_in = int(round(n * inlier_ratio))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.05, 0.25)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.stack([rng.uniform(-2, 2, n_in), rng.uniform(-1.6, 1.6, n_in), rng.uniform(4, 8, n_in)], 1)
    p1 = (K @ X.T).T
    p2 = (K @ (Rm @ X.T + t[:, None])).T
    inl = np.hstack([p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]])
    out = rng.uniform(0, 1, (n - n_in, 4)) * np.array([W, H, W, H])
    pts = np.vstack([inl, out])
    return np.ascontiguousarray(pts[rng.permutation(n)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--checker-pairs", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        ps = TV.PointSets()
    except (TV.TwoViewGeometryError, RuntimeError) as e:
        sys.exit(f"bench_geometric_verification needs a GPU: {e}")
    cam1, cam2 = TV.CameraInfo(1, W, H, 1), TV.CameraInfo(1, W, H, 2)
    options = TV.TwoViewGeometryOptions(ransac_options=TV.RANSACOptions(random_seed=0))
    result = dict(pairs=a.pairs, matches=a.matches, model_tile=TV.model_tile(), match_tile=TV.match_tile(),
                  trial_round=TV.trial_round(), window_s=a.window, ratios={})
    for ratio in (0.3, 0.7):
        rng = np.random.default_rng(int(ratio * 10))
        sets = [make_pair(a.matches, ratio, rng) for _ in range(a.pairs)]
        ids = list(range(1, a.pairs + 1))
        run = lambda: ps.verify_pairs([cam1] * a.pairs, [cam2] * a.pairs, sets, ids, options)  # noqa: E731
        geoms, stats = run()
        calls, kernel_ms, total_ms, t0 = 0, 0.0, 0.0, time.perf_counter()
        while True:
            run()
            k, t = TV.last_timing()
            calls, kernel_ms, total_ms = calls + 1, kernel_ms + k, total_ms + t
            wall = time.perf_counter() - t0
            if wall >= a.window:
                break
        residuals = stats["num_scored"] * a.matches
        r = dict(calls=calls, kernel_ms_per_call=kernel_ms / calls, total_ms_per_call=total_ms / calls, wall_ms_per_call=1e3 * wall / calls,
                 pairs_per_s=a.pairs * calls / wall, models_scored=stats["num_scored"], launches=stats["num_launches"],
                 residuals_per_s_kernel=residuals * calls / (kernel_ms * 1e-3), residuals_per_s_wall=residuals * calls / wall,
                 configs={str(c): int(sum(g.config == c for g in geoms)) for c in sorted({g.config for g in geoms})},
                 mean_inliers=float(np.mean([g.inlier_mask.sum() for g in geoms])))
        if a.checker_pairs > 0:
            import two_view_reference as R
            o = R.tvg_options(ransac=R.ransac_options(random_seed=0))
            t1 = time.perf_counter()
            for p in range(min(a.checker_pairs, a.pairs)):
                R.estimate_two_view_geometry((W, H), (W, H), sets[p], ids[p], o)
            r["checker_s_per_pair"] = (time.perf_counter() - t1) / min(a.checker_pairs, a.pairs)
        result["ratios"][str(ratio)] = r
        print(json.dumps({str(ratio): r}), flush=True)
    ps.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
