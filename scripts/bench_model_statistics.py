"""Times the model statistics (include/colmap_amd_model.h) on the benchmark's BA-1 model -- synthesize_flat with the
arguments of bench.py's secondary workload: 1000 images x 200 k points, track length 10 -- and on one tenth of it, next
to the interpreted loops of colmap_amd.workspace.Model that did this work before (ComputeDepthRanges,
ComputeSharedPoints, ComputeTriangulationAngles). Not part of bench.py.

    python scripts/bench_model_statistics.py [--repeats 5] [--python-full] [--out profiles/model_statistics_bench_mi355x.json]

Per call it reports the kernel time and the whole-call time of model_last_timing (best of --repeats after one warm-up)
and track pairs per second of the whole call. The Python loops are timed on the tenth-size model; their full-size figure
is an EXTRAPOLATION by the pair count unless --python-full measures it. It also times
PatchMatchController.FromWorkspace on a tenth-size workspace on disk (`__auto__, 20` for every image), Python route
against device route.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colmap_amd import model_statistics as MS  # noqa: E402
from colmap_amd import scene  # noqa: E402
from colmap_amd import workspace as W  # noqa: E402


def rotations(poses):
    x, y, z, w = poses[:, 0], poses[:, 1], poses[:, 2], poses[:, 3]
    R = np.empty((len(poses), 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def flat_model(d, track):
    points = len(d["points"])
    return MS.FlatModel(R=rotations(d["poses"]).reshape(-1, 9).astype(np.float32), T=d["poses"][:, 4:].astype(np.float32),
                        points=d["points"].astype(np.float32), track_offsets=np.arange(points + 1, dtype=np.int64) * track,
                        track_image=d["obs_pose"].astype(np.int32))


def python_model(f):
    m = W.Model()
    K = np.array([[1280, 0, 512], [0, 1280, 384], [0, 0, 1]], np.float32)
    for R, T in zip(f.R, f.T):
        m.images.append(W.ModelImage("", 1024, 768, K, R.reshape(3, 3), T))
    for p, X in enumerate(f.points):
        m.points.append(W.ModelPoint(float(X[0]), float(X[1]), float(X[2]),
                                     [int(i) for i in f.track_image[f.track_offsets[p]:f.track_offsets[p + 1]]]))
    return m


def time_device(f, repeats, pairs):
    calls = {"compute_depth_ranges": lambda: MS.depth_ranges_flat(f),
             "compute_pair_statistics": lambda: MS.pair_statistics_flat(f, 75.0),
             "get_max_overlapping_images": lambda: MS.max_overlapping_images_flat(f, 20, 1.0)}
    out = {}
    for name, call in calls.items():
        call()  # warm-up: code object load, first allocation
        runs = []
        for _ in range(repeats):
            call()
            runs.append((MS.last_timing.kernel_ms, MS.last_timing.total_ms))
        total = min(t for _, t in runs)
        out[name] = dict(kernel_ms=min(k for k, _ in runs), total_ms=total, pairs_per_s=pairs / (total * 1e-3),
                         all_total_ms=[round(t, 3) for _, t in runs])
    return out


def time_python(f):
    m = python_model(f)
    t0 = time.perf_counter()
    m.ComputeDepthRanges()
    t1 = time.perf_counter()
    m.ComputeSharedPoints()
    t2 = time.perf_counter()
    m.ComputeTriangulationAngles(75.0)
    t3 = time.perf_counter()
    return dict(ComputeDepthRanges_s=t1 - t0, ComputeSharedPoints_s=t2 - t1, ComputeTriangulationAngles_s=t3 - t2)


def time_from_workspace(d, track):
    """FromWorkspace on a workspace on disk: 16x12 bitmaps, the sparse model of `d`, `__auto__, 20` for every image."""
    from PIL import Image as PILImage
    from colmap_amd import mvs
    frames, points = len(d["poses"]), len(d["points"])
    sm = W.SparseModel()
    sm.cameras[1] = W.SparseCamera(1, 1, 16, 12, np.array([20.0, 20.0, 8.0, 6.0]))
    obs_image = d["obs_pose"].reshape(points, track)
    for i in range(frames):
        q = d["poses"][i, [3, 0, 1, 2]]  # w x y z
        im = W.SparseImage(i + 1, q, d["poses"][i, 4:], 1, f"img{i:04d}.png")
        pts = np.nonzero((obs_image == i).any(axis=1))[0]
        im.xys = np.zeros((len(pts), 2))
        im.point3D_ids = pts + 1
        sm.images[i + 1] = im
    slot = [dict((int(p) - 1, k) for k, p in enumerate(sm.images[i + 1].point3D_ids)) for i in range(frames)]
    for p in range(points):
        sm.points3D[p + 1] = W.SparsePoint3D(p + 1, d["points"][p], (0, 0, 0), 0.0,
                                             [(int(i) + 1, slot[int(i)][p]) for i in obs_image[p]])
    with tempfile.TemporaryDirectory() as ws:
        W.write_model_binary(sm, os.path.join(ws, "sparse"))
        os.makedirs(os.path.join(ws, "images"))
        os.makedirs(os.path.join(ws, "stereo"))
        for im in sm.images.values():
            PILImage.fromarray(np.zeros((12, 16), np.uint8)).save(os.path.join(ws, "images", im.name))
        W.write_patch_match_config(os.path.join(ws, "stereo", "patch-match.cfg"), [im.name for im in sm.images.values()])
        options = mvs.PatchMatchOptions(gpu_index="0")
        device = MS.DeviceStatistics(0)
        mvs.PatchMatchController.FromWorkspace(options, ws, model_statistics=device)  # warm-up
        t0 = time.perf_counter()
        got = mvs.PatchMatchController.FromWorkspace(options, ws, model_statistics=device)
        t1 = time.perf_counter()
        want = mvs.PatchMatchController.FromWorkspace(options, ws)
        t2 = time.perf_counter()
    return dict(device_route_s=t1 - t0, python_route_s=t2 - t1, problems=len(got.problems_),
                same_problems=got.problems_ == want.problems_)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--python-full", action="store_true", help="time the Python loops on the full model too (minutes)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    result = dict(track=a.track, repeats=a.repeats, sizes={})
    for label, frames, points in (("tenth", a.frames // 10, a.points // 10), ("ba1", a.frames, a.points)):
        d = scene.synthesize_flat(frames, points, a.track, seed=42)
        f = flat_model(d, a.track)
        pairs = points * a.track * (a.track - 1) // 2
        entry = dict(frames=frames, points=points, observations=len(f.track_image), track_pairs=pairs,
                     device=time_device(f, a.repeats, pairs))
        if label == "tenth" or a.python_full:
            entry["python"] = time_python(f)
            entry["python"]["measured"] = True
        else:
            scale = pairs / result["sizes"]["tenth"]["track_pairs"]
            entry["python"] = {k: v * scale for k, v in result["sizes"]["tenth"]["python"].items() if k.endswith("_s")}
            entry["python"]["measured"] = False
            entry["python"]["note"] = f"EXTRAPOLATED from the tenth-size model by the pair count (x{scale:g})"
        if label == "tenth":
            entry["from_workspace"] = time_from_workspace(d, a.track)
        result["sizes"][label] = entry
        print(json.dumps({label: entry}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
