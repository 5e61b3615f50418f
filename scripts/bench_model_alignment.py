"""Times model alignment (include/colmap_amd_align.h) on two noisy copies of a model of the shape of the benchmark's BA-1
model -- scene.synthesize_flat with 1000 images x 200 k points, track length 10, 2 M observations -- one of them moved
by a known similarity. Runs on the GPU only (there is no CPU path to time). Not part of bench.py.

    python scripts/bench_model_alignment.py [--out profiles/model_alignment_bench_mi355x.json]

Reports
  * scored (hypothesis, observation) pairs per second of align_reproj_score for B = 1, 8, 16, 32, 64, 128 hypotheses per
    launch, by kernel time and by whole-call time;
  * kernel and total ms of a whole AlignReconstructionsViaReprojections search at the default batch size, and of the same
    search with B = 1 (the reports are asserted equal);
  * points per second of align_transform_points on 20 M points.
Every figure comes from a warm-up followed by a timed window of at least --window seconds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from colmap_amd import alignment as AL  # noqa: E402
from colmap_amd import scene  # noqa: E402

SIM = AL.Sim3d.from_srt(1.7, scene.quat_to_rot(np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9])),
                        np.array([0.5, -1.0, 2.0]))


def make_pair(frames, points, track, seed=42):
    """Two copies of the BA-1-shaped model in its adjusted state (exact geometry, thirds of SIMPLE_RADIAL / PINHOLE /
    OPENCV cameras), each with pixel noise of its own (0.5 px). src: points moved by 1e-3 and the whole model taken
    through Inverse(SIM); 5 % of the images get a wrong src pose."""
    d = scene.synthesize_flat(frames, points, track, seed=seed, mixed_models="three")
    rng = np.random.default_rng(seed + 1)
    cams = [(int(d["cam_model"][i]), 1024, 768, d["cams"][i, :scene.MODEL_NUM_PARAMS[int(d["cam_model"][i])]]) for i in range(frames)]
    inv = AL.Inverse(SIM)
    obs_point = np.repeat(np.arange(points), track)
    tgt_xyz = d["points"][obs_point]
    src_xyz = inv * (d["points"] + 1e-3 * rng.normal(size=d["points"].shape))
    R, s, t = SIM.RotationMatrix(), SIM.scale, SIM.translation
    src_poses = np.zeros((frames, 7))
    for i in range(frames):
        Rt = scene.quat_to_rot(d["poses"][i, :4])
        ts = (Rt @ t + d["poses"][i, 4:]) / s
        if rng.uniform() < 0.05:
            ts = ts + rng.uniform(-1, 1, 3)
        src_poses[i] = np.concatenate([scene.rot_to_quat(Rt @ R), ts])
    n2d = np.bincount(d["obs_pose"], minlength=frames).astype(np.int32)
    return AL.FlatPair(cams, cams, src_poses, d["poses"], n2d, n2d, d["obs_pose"].astype(np.int32), src_xyz[obs_point], tgt_xyz,
                       d["obs_xy"] + 0.5 * rng.normal(size=d["obs_xy"].shape), d["obs_xy"] + 0.5 * rng.normal(size=d["obs_xy"].shape))


def window(fn, seconds):
    """(calls, wall seconds, kernel ms summed) of fn() repeated for at least `seconds` after one warm-up call."""
    fn()
    calls, kernel_ms, t0 = 0, 0.0, time.perf_counter()
    while True:
        fn()
        calls += 1
        kernel_ms += AL.last_timing()[0]
        wall = time.perf_counter() - t0
        if wall >= seconds:
            return calls, wall, kernel_ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--transform-points", type=int, default=20_000_000)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    pair = make_pair(a.frames, a.points, a.track)
    try:
        scorer = AL.ReprojScorer(pair)
    except AL.AlignmentError as e:
        sys.exit(f"bench_model_alignment needs a GPU: {e}")
    n = len(pair.rec_image)
    result = dict(images=pair.num_images, observations=n, hypothesis_tile=AL.hypothesis_tile(), window_s=a.window, score={})
    rng = np.random.default_rng(3)
    for B in (1, 8, 16, 32, 64, 128):
        hyps = []
        for _ in range(B):  # near the truth, so that both reprojections of most observations are evaluated
            q = np.asarray(SIM.rotation) + 1e-3 * rng.normal(size=4)
            hyps.append(np.concatenate([[SIM.scale * (1 + 1e-3 * rng.normal())], q / np.linalg.norm(q),
                                        np.asarray(SIM.translation) + 1e-2 * rng.normal(size=3)]))
        calls, wall, kernel_ms = window(lambda: scorer.score(hyps, 8.0), a.window)
        result["score"][B] = dict(calls=calls, kernel_ms_per_call=kernel_ms / calls, wall_ms_per_call=1e3 * wall / calls,
                                  pairs_per_s_kernel=B * n * calls / (kernel_ms * 1e-3), pairs_per_s_wall=B * n * calls / wall)
        print(json.dumps({"score": {B: result["score"][B]}}), flush=True)

    reports = {}
    for label, B in (("default", 0), ("B1", 1)):
        opt = AL.RANSACOptions(min_inlier_ratio=0.2, batch_size=B)
        runs = []
        calls, wall, kernel_ms = window(lambda: runs.append(scorer.estimate(0.3, 8.0, opt)), a.window)
        rep = runs[-1]
        reports[label] = rep
        result["search_" + label] = dict(calls=calls, kernel_ms=kernel_ms / calls, total_ms=1e3 * wall / calls, success=rep.success,
                                         num_trials=rep.num_trials, num_inliers=rep.num_inliers, num_scored=rep.num_scored,
                                         num_launches=rep.num_launches, model=[float(v) for v in rep.model.params()])
        print(json.dumps({"search_" + label: result["search_" + label]}), flush=True)
    r0, r1 = reports["default"], reports["B1"]
    assert (r0.success, r0.num_trials, r0.num_inliers) == (r1.success, r1.num_trials, r1.num_inliers)
    assert np.array_equal(r0.model.params(), r1.model.params()) and np.array_equal(r0.inlier_mask, r1.inlier_mask)
    scorer.close()

    pts = np.random.default_rng(5).uniform(-10, 10, (a.transform_points, 3))
    calls, wall, kernel_ms = window(lambda: AL.transform_points(pts, SIM), a.window)
    result["transform"] = dict(points=a.transform_points, calls=calls, kernel_ms=kernel_ms / calls, total_ms=1e3 * wall / calls,
                               points_per_s_kernel=a.transform_points * calls / (kernel_ms * 1e-3),
                               points_per_s_wall=a.transform_points * calls / wall)
    print(json.dumps({"transform": result["transform"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
