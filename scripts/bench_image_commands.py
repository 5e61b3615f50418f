#!/usr/bin/env python3
"""Throughput of stereo rectification and colour extraction on one MI355X.

    python scripts/bench_image_commands.py [--pairs 16] [--images 1000] [--points 200000] [--repeats 3]
                                           [--out profiles/image_commands_bench.json]

Two measurements, each repeat in a child process of its own under a timeout:
  rectify  `--pairs` pairs of 2560x1920 RGB images through an OPENCV lens, pose Euler (0, 0.05, 0), t = (0.1, 0, 0):
           the rectify kernels' time (HIP events, undistort_last_timing) and the wall time of the one
           undistort_rectify_images call (allocation, both copies, kernels).
  colour   a synthetic model of `--points` points, each observed in 5 of `--images` images of 1024x768 RGB noise held in
           memory: the sample kernels' time, the point kernels' time (HIP events, color_timing) and the time of all calls of
           the handle (allocation, the copies of every image and its observations, kernels, the copy back).
floor_ms is what HBM alone would need for the bytes the kernels must move, at 8 TB/s.
Both calls are expected to be bound by the host<->device copies (and, in the commands, by image decode), not by the
kernels. Not the project benchmark (bench.py) and no pass/fail number: the parent commit has no such path."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
TRACK = 5   # observations per point of the colour model


def rectify_child(n_pairs: int) -> dict:
    import numpy as np
    from colmap_amd import undistortion as U
    from colmap_amd import workspace as WS
    W, H = 2560, 1920
    cam = WS.SparseCamera(1, WS.CAMERA_MODEL_IDS["OPENCV"], W, H,
                          np.array([2400.0, 2410.0, 1283.0, 957.0, 0.05, -0.01, 0.001, -0.002]))
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    c, s = np.cos(0.05), np.sin(0.05)
    R, t = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.array([0.1, 0.0, 0.0])
    pairs = [(np.roll(base, 17 * i, axis=1), np.roll(base, 17 * i + 5, axis=0), cam, cam, R, t) for i in range(n_pairs)]
    t0 = time.perf_counter()
    res = U.RectifyAndUndistortStereoImagePairs(U.UndistortCameraOptions(), pairs)
    wall = time.perf_counter() - t0
    kernel_ms, total_ms = U.LastTiming()
    oc = res[0][2]
    pix = 2 * n_pairs * oc.width * oc.height
    return dict(pairs=n_pairs, source=[W, H], target=[oc.width, oc.height], kernel_ms=kernel_ms, call_ms=total_ms,
                wall_ms=wall * 1e3, kernel_ms_per_image=kernel_ms / (2 * n_pairs), kernel_mpix_s=pix / kernel_ms / 1e3,
                end_to_end_mpix_s=pix / total_ms / 1e3,
                floor_ms_per_image=(W * H * 3 + oc.width * oc.height * 3) / HBM_BYTES_PER_S * 1e3,
                nonblank=float((res[0][0] != 0).mean()))


def colour_child(n_images: int, n_points: int) -> dict:
    import numpy as np
    from colmap_amd import color_extraction as CE
    W, H = 1024, 768
    rng = np.random.default_rng(1)
    bitmaps = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]   # held in memory, cycled
    n_obs = n_points * TRACK
    obs_point = np.repeat(np.arange(n_points, dtype=np.int64), TRACK)
    obs_image = rng.integers(0, n_images, n_obs).astype(np.int64)
    obs_p2d = np.arange(n_obs, dtype=np.int64)
    xy = np.stack([rng.uniform(-2.0, W + 2.0, n_obs), rng.uniform(-2.0, H + 2.0, n_obs)], 1)   # a few fall outside
    ptr, slot = CE.SlotLayout(obs_point, obs_image, obs_p2d, n_points)
    order = np.argsort(obs_image, kind="stable")
    starts = np.searchsorted(obs_image[order], np.arange(n_images + 1))
    t0 = time.perf_counter()
    with CE.ColorExtractor(n_obs) as ex:
        for i in range(n_images):
            sel = order[starts[i]:starts[i + 1]]
            if len(sel):
                ex.AddImage(bitmaps[i % len(bitmaps)], xy[sel], slot[sel])
        rgb, count = ex.Finish(ptr)
        sample_ms, point_ms, calls_ms = ex.Timing()
    wall = time.perf_counter() - t0
    # bytes the kernels must move: per observation xy + slot + 4 texels x 3 bytes + the 13-byte slot; per point the slots
    # read back, two ptr entries' worth and the 7 bytes out
    sample_bytes = n_obs * (16 + 8 + 12 + 13)
    point_bytes = n_obs * 13 + n_points * (8 + 7)
    return dict(images=n_images, points=n_points, observations=n_obs, image=[W, H], sample_kernel_ms=sample_ms,
                point_kernel_ms=point_ms, calls_ms=calls_ms, wall_ms=wall * 1e3,
                sample_floor_ms=sample_bytes / HBM_BYTES_PER_S * 1e3, point_floor_ms=point_bytes / HBM_BYTES_PER_S * 1e3,
                upload_mb=n_images * W * H * 3 / 1e6, coloured=float((count > 0).mean()),
                mean_colour=[float(v) for v in rgb.mean(0)])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(rectify_child(a.pairs) if a.child == "rectify" else colour_child(a.images, a.points)))
        return 0
    out = dict(workload=dict(rectify=f"{a.pairs} pairs of RGB images 2560x1920, OPENCV, bilinear, default options",
                             colour=f"{a.images} RGB images 1024x768, {a.points} points with {TRACK} observations each"))
    for what, key in (("rectify", "kernel_ms"), ("colour", "sample_kernel_ms")):
        runs = []
        for _ in range(a.repeats):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--pairs", str(a.pairs),
                                "--images", str(a.images), "--points", str(a.points)],
                               capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:   # a failed GPU step ends the script: nothing more is started on the device
                sys.stderr.write(r.stderr)
                return r.returncode or 1
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        out[what] = dict(median=sorted(runs, key=lambda d: d[key])[len(runs) // 2], runs=runs)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
