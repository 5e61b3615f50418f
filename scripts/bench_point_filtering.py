"""Times observation / point filtering (include/colmap_amd_obs.h) on the benchmark's BA-1 model -- synthesize_flat with
the arguments of bench.py's secondary workload: 1000 images x 200 k points, track length 10 -- and on one tenth of it,
next to the two interpreted loops of colmap_amd/bundle_adjuster.py that did this work before
(filter_observations_with_negative_depth, point3D_errors). Not part of bench.py.

    python scripts/bench_point_filtering.py [--repeats 5] [--python-full] [--out profiles/point_filtering_bench_mi355x.json]

Per call it reports the kernel time and the whole-call time of obs_last_timing (best of --repeats after one warm-up) and
observations per second of the whole call. The Python loops are timed on the tenth-size model; their full-size figure is
an EXTRAPOLATION by the observation count unless --python-full measures it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colmap_amd import bundle_adjuster as BA  # noqa: E402
from colmap_amd import observation_manager as OM  # noqa: E402
from colmap_amd import scene  # noqa: E402

NOISE = scene.SyntheticNoiseOptions(0.01, 1.0, 0.05, 1.0)  # bench.py ba_secondary


def flat_model(d, track):
    frames, points = len(d["poses"]), len(d["points"])
    cams = [(int(d["cam_model"][i]), 1024, 768, d["cams"][i, :scene.MODEL_NUM_PARAMS[int(d["cam_model"][i])]]) for i in range(frames)]
    return OM.FlatModel(cameras=cams, image_poses=d["poses"], image_camera=np.arange(frames, dtype=np.int32), points=d["points"],
                        obs_offsets=np.arange(points + 1, dtype=np.int64) * track, obs_image=d["obs_pose"], obs_xy=d["obs_xy"])


def reconstruction(d, track):
    rec = scene.Reconstruction()
    for i in range(len(d["poses"])):
        m = int(d["cam_model"][i])
        rec.cameras[i + 1] = scene.Camera(i + 1, m, 1024, 768, d["cams"][i, :scene.MODEL_NUM_PARAMS[m]].copy())
        rec.images[i + 1] = scene.Image(i + 1, i + 1, d["poses"][i].copy())
    for p in range(len(d["points"])):
        pt = scene.Point3D(d["points"][p].copy())
        for o in range(p * track, (p + 1) * track):
            img = rec.images[int(d["obs_pose"][o]) + 1]
            img.points2D.append(scene.Point2D(d["obs_xy"][o].copy(), p + 1))
            pt.track.append((img.image_id, len(img.points2D) - 1))
        rec.points3D[p + 1] = pt
    return rec


def time_device(m, repeats):
    out = {}
    for entry in ("filter_negative_depth", "point_errors", "filter_all_points3D", "filter_short_tracks"):
        OM.run_flat(entry, m)  # warm-up: code object load, first allocation
        runs = [OM.run_flat(entry, m) for _ in range(repeats)]
        best = min(runs, key=lambda r: r.total_ms)
        out[entry] = dict(kernel_ms=min(r.kernel_ms for r in runs), total_ms=best.total_ms,
                          observations_per_s=len(m.obs_image) / (best.total_ms * 1e-3), num_filtered=best.num_filtered,
                          all_total_ms=[round(r.total_ms, 3) for r in runs])
    return out


def time_python(d, track):
    rec = reconstruction(d, track)
    t0 = time.perf_counter()
    n = BA.filter_observations_with_negative_depth(rec)
    t1 = time.perf_counter()
    BA.point3D_errors(rec)
    t2 = time.perf_counter()
    return dict(filter_observations_with_negative_depth_s=t1 - t0, point3D_errors_s=t2 - t1, num_filtered=n)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--python-full", action="store_true", help="time the Python loops on the full model too (minutes)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    result = dict(noise=[0.01, 1.0, 0.05, 1.0], track=a.track, repeats=a.repeats, sizes={})
    for label, frames, points in (("tenth", a.frames // 10, a.points // 10), ("ba1", a.frames, a.points)):
        d = scene.synthesize_flat(frames, points, a.track, seed=42, noise=NOISE)
        m = flat_model(d, a.track)
        entry = dict(frames=frames, points=points, observations=len(m.obs_image), device=time_device(m, a.repeats))
        if label == "tenth" or a.python_full:
            entry["python"] = time_python(d, a.track)
            entry["python"]["measured"] = True
        else:
            scale = len(m.obs_image) / result["sizes"]["tenth"]["observations"]
            entry["python"] = {k: v * scale for k, v in result["sizes"]["tenth"]["python"].items() if k.endswith("_s")}
            entry["python"]["measured"] = False
            entry["python"]["note"] = f"EXTRAPOLATED from the tenth-size model by the observation count (x{scale:g})"
        result["sizes"][label] = entry
        print(json.dumps({label: entry}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
