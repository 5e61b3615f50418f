"""Times the GPU covariance estimate (include/colmap_amd_ba_covariance.h) on a BA-1-shaped problem and prints one JSON
line. Every mode runs once untimed, then once timed; wall times include the host set-up (flattening into the device
layout, upload) and end with the batched block query, which synchronises the device.

    python scripts/ba_covariance_timing.py [--frames 1000 --points 200000 --track 10]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from colmap_amd import estimators as est  # noqa: E402
from colmap_amd import scene  # noqa: E402

FP64_MFMA_SPEC_TFLOPS = 78.6  # MI355X fp64 matrix-core peak (datasheet figure DESIGN.md uses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args()
    d = scene.synthesize_flat(a.frames, a.points, a.track, seed=42, noise=scene.SyntheticNoiseOptions(0.01, 1.0, 0.05, 1.0))
    fp = est.FlatProblem.from_arrays(d)
    est.fix_gauge_two_cams(fp)
    P = est.BACovarianceParams
    out = {"workload": f"BA-1 shape: {a.frames} images x {a.points} points, track {a.track}, SIMPLE_RADIAL, gauge "
                       f"TWO_CAMS_FROM_WORLD, {len(fp.obs_pose)} observations; evaluated at the synthesized parameters",
           "camera_side_columns": est.num_camera_parameters(fp), "modes": {}}
    for mode in (P.ALL, P.POSES, P.POSES_AND_POINTS, P.POINTS):
        rec = None
        for rep in range(2):
            t0 = time.perf_counter()
            flat = est.estimate_covariance_flat(fp, est.BACovarianceOptions(params=mode), gpu_index=a.gpu)
            if flat is None:
                raise SystemExit(f"not estimable: {est.last_covariance_message}")
            t_est = time.perf_counter() - t0
            pairs = [(est.COV_KIND_POSE, i, est.COV_KIND_POSE, i) for i in range(len(fp.poses))]
            if mode == P.ALL:
                pairs += [(est.COV_KIND_CAMERA, k, est.COV_KIND_CAMERA, k) for k in range(len(fp.cams))]
            t1 = time.perf_counter()
            blocks = flat.blocks(pairs) if mode != P.POINTS else []
            t_q = time.perf_counter() - t1
            t = flat.timing()
            flat.close()
            rec = {"wall_s_estimate": round(t_est, 4), "wall_s_batched_diagonal_query": round(t_q, 4),
                   "diagonal_blocks_returned": sum(b is not None for b in blocks),
                   "hip_event_ms": {"formation": round(t["form_ms"], 3), "factorisation": round(t["factor_ms"], 3),
                                    "triangular_inverse": round(t["inverse_ms"], 3),
                                    "extraction_of_the_query": round(t["extract_ms"], 3)},
                   "factored_dimension": t["n"], "inverted_dimension": t["n_inverted"]}
            if t["inverse_ms"] > 0:
                flop = t["n_inverted"] ** 3 / 3.0
                tf = flop / (t["inverse_ms"] * 1e-3) / 1e12
                rec["inverse_flop_n3_over_3"] = flop
                rec["inverse_tflops_achieved"] = round(tf, 3)
                rec["inverse_fraction_of_fp64_mfma_spec"] = round(tf / FP64_MFMA_SPEC_TFLOPS, 4)
        out["modes"][mode.name] = rec
    out["fp64_mfma_spec_tflops"] = FP64_MFMA_SPEC_TFLOPS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
