"""Times SIFT extraction (include/colmap_amd_sift.h) on synthetic blob images at 1600 x 1200 and 3200 x 2400 with the
default options. Runs on the GPU only (there is no CPU path to time). Not part of bench.py.

    python scripts/bench_feature_extraction.py [--window 1.0] [--out profiles/feature_extraction_bench_mi355x.json]

Reports, per size, images / s and Mpix / s by event time and by whole call, the split of the event time over pyramid,
detection, orientation and descriptor, and the numbers of candidates, detections and output rows. Event time is what
sift_last_timing gives: intervals between HIP events at the borders of the stages, which hold the host synchronisations,
copies and gaps inside a stage as well as its kernels. `pyramid_bytes` are the algorithmic bytes of the kernels that run
INSIDE the pyramid interval and of no others: the base level of every octave written once, and every smoothing (S + 2 per
octave, one more for the base of the first octave) read once and written once by each of its two passes;
`pyramid_gb_per_s` divides them by that interval. The DoG levels (`dog_bytes`: two reads and a write per level) are moved
in the detection interval and the gradient planes (`gradient_bytes`: a read and two floats written per plane) in the
orientation interval, next to other work, so no rate is formed from them. Every figure comes from a warm-up call
followed by a timed window of at least --window seconds. The image is a 400 x 300 tile of 320 anisotropic Gaussian blobs
from a seeded generator, mirrored and repeated to the size.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from colmap_amd import feature_extraction as FE  # noqa: E402


def blob_tile(w, h, n, seed):
    """A sum of n anisotropic Gaussian blobs of random sign, sigma 1 to 5 px, around mid-grey, quantised to uint8."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.zeros((h, w))
    for _ in range(n):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        sx, sy = rng.uniform(1.0, 5.0, 2)
        th = rng.uniform(0, np.pi)
        a = rng.uniform(0.08, 0.35) * (1 if rng.randint(2) else -1)
        u = np.cos(th) * (xx - cx) + np.sin(th) * (yy - cy)
        v = -np.sin(th) * (xx - cx) + np.cos(th) * (yy - cy)
        im += a * np.exp(-(u * u / (2 * sx * sx) + v * v / (2 * sy * sy)))
    return np.clip(np.floor((0.5 + im) * 255 + 0.5), 0, 255).astype(np.uint8)


def make_image(w, h):
    tile = blob_tile(400, 300, 320, 7)
    row = np.hstack([tile, tile[:, ::-1]])
    quad = np.vstack([row, row[::-1]])
    reps = ((h + quad.shape[0] - 1) // quad.shape[0], (w + quad.shape[1] - 1) // quad.shape[1])
    return np.ascontiguousarray(np.tile(quad, reps)[:h, :w])


def stage_bytes(w, h, o):
    """Algorithmic bytes per image by the interval their kernels run in: (pyramid, dog, gradient). See the module text."""
    S, pyramid, dog, grad = o.octave_resolution, 0, 0, 0
    for k in range(o.num_octaves):
        oc = o.first_octave + k
        ow, oh = (w << -oc, h << -oc) if oc < 0 else (w >> oc, h >> oc)
        if ow < 2 or oh < 2:
            break
        plane = 4 * ow * oh
        smooths = (S + 2) + (1 if k == 0 else 0)
        pyramid += plane + smooths * 4 * plane
        dog += (S + 2) * 3 * plane
        grad += S * 3 * plane
    return pyramid, dog, grad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--sizes", default="1600x1200,3200x2400")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        ex = FE.SiftFeatureExtractor()
    except (FE.FeatureExtractionError, RuntimeError) as e:
        sys.exit(f"bench_feature_extraction needs a GPU: {e}")
    o = ex.options
    result = dict(window_s=a.window, conv_tiles=[FE.conv_tile(0), FE.conv_tile(1)], halo_limit=FE.halo_limit(), sizes={})
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        img = make_image(w, h)
        kp, _ = ex.extract(img)   # warm-up: buffers grow here
        calls, kernel_ms, total_ms, stages, t0 = 0, 0.0, 0.0, dict.fromkeys(FE.STAGES, 0.0), time.perf_counter()
        while True:
            ex.extract(img)
            k, t, s = FE.last_timing()
            calls, kernel_ms, total_ms = calls + 1, kernel_ms + k, total_ms + t
            for name in FE.STAGES:
                stages[name] += s[name]
            wall = time.perf_counter() - t0
            if wall >= a.window:
                break
        mpix = w * h * 1e-6
        nbytes, dog_bytes, grad_bytes = stage_bytes(w, h, o)
        detections = sum(len(ex.detections(i)) for i in range(ex.num_octaves()))
        candidates = sum(ex.num_candidates(i) for i in range(ex.num_octaves()))
        r = dict(calls=calls, images_per_s_events=calls / (kernel_ms * 1e-3), images_per_s_call=calls / (total_ms * 1e-3),
                 images_per_s_wall=calls / wall, mpix_per_s_events=mpix * calls / (kernel_ms * 1e-3),
                 mpix_per_s_call=mpix * calls / (total_ms * 1e-3), event_ms_per_image=kernel_ms / calls,
                 call_ms_per_image=total_ms / calls, stage_ms_per_image={n: stages[n] / calls for n in FE.STAGES},
                 candidates=candidates, detections=detections, rows=len(kp), reruns=ex.num_reruns(),
                 pyramid_bytes=nbytes, dog_bytes=dog_bytes, gradient_bytes=grad_bytes,
                 pyramid_gb_per_s=nbytes * 1e-9 / (stages["pyramid"] / calls * 1e-3))
        result["sizes"][size] = r
        print(json.dumps({size: r}), flush=True)
    ex.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
