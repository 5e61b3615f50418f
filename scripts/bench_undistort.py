#!/usr/bin/env python3
"""Throughput of image undistortion on one MI355X: 16 RGB images of 2560x1920 through an OPENCV lens.

    python scripts/bench_undistort.py [--images 16] [--repeats 3] [--out profiles/undistort_bench.json]

Reports, per repeat and as the median:
  kernel_mpix_s      target pixels / time of the warp kernels alone (HIP events, undistort_last_timing)
  end_to_end_mpix_s  target pixels / wall time of undistort_images: allocation, both copies and the kernels
  floor_ms_per_image (source bytes + target bytes) / 8 TB/s, the time HBM alone would need
The end-to-end figure is expected to be bounded by the host<->device copies of pageable memory (and, in the command,
by image decode and encode), not by the kernel. Every GPU step runs in a child process under its own timeout.
Not the project benchmark (bench.py) and no pass/fail number: the parent commit has no such path to compare with."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 2560, 1920
HBM_BYTES_PER_S = 8e12


def child(n_images: int) -> dict:
    import numpy as np
    from colmap_amd import undistortion as U
    from colmap_amd import workspace as WS
    cam = WS.SparseCamera(1, WS.CAMERA_MODEL_IDS["OPENCV"], W, H,
                          np.array([2400.0, 2410.0, 1283.0, 957.0, 0.05, -0.01, 0.001, -0.002]))
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    imgs = [np.roll(base, 17 * i, axis=1) for i in range(n_images)]
    opt = U.UndistortCameraOptions()
    t0 = time.perf_counter()
    res = U.UndistortImages(opt, imgs, [cam] * n_images)
    wall = time.perf_counter() - t0
    kernel_ms, total_ms = U.LastTiming()
    oc = res[0][1]
    pix = n_images * oc.width * oc.height
    return dict(images=n_images, source=[W, H], target=[oc.width, oc.height], kernel_ms=kernel_ms, call_ms=total_ms,
                wall_ms=wall * 1e3, kernel_mpix_s=pix / kernel_ms / 1e3, end_to_end_mpix_s=pix / total_ms / 1e3,
                floor_ms_per_image=(W * H * 3 + oc.width * oc.height * 3) / HBM_BYTES_PER_S * 1e3,
                kernel_ms_per_image=kernel_ms / n_images, nonblank=float((res[0][0] != 0).mean()))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per GPU step")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.images)))
        return 0
    runs = []
    for _ in range(a.repeats):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--images", str(a.images)],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:   # a failed GPU step ends the script: nothing more is started on the device
            sys.stderr.write(r.stderr)
            return r.returncode or 1
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    med = sorted(runs, key=lambda d: d["kernel_ms"])[len(runs) // 2]
    out = dict(workload=f"{a.images} RGB images {W}x{H}, OPENCV, bilinear, default options", median=med, runs=runs)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
