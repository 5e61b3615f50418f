"""Times SIFT descriptor matching (include/colmap_amd_match.h) on generated descriptor sets: sets of 2048, 8192 and 32768
descriptors, batches of 1, 8 and 64 pairs per launch. Runs on the GPU only (there is no CPU path to time). Not part of
bench.py.

    python scripts/bench_feature_matching.py [--out profiles/feature_matching_bench_mi355x.json]

A batch of B pairs is the chain (1, 2), (2, 3), ... over B + 1 sets, as the sequential matcher makes them. Reports, per
(set size, batch size):
  * kernel time (HIP events) and whole-call time of match_pairs with the sets already resident -- pairs per second and
    descriptor comparisons per second (rows1 x rows2 per pair, both directions counted once), and the int8
    multiply-adds per second the shapes imply (2 directions x rows1 x rows2 x 128);
  * cold time: a new handle, the upload of the B + 1 sets and the call;
  * the bytes a launch streams from device memory or its caches, from the shapes: every tile of 256 query rows reads the
    whole other set (132 bytes a row).
For scale only, the numpy checker's time on one pair of the smallest size is given, labelled as such.
Every figure comes from a warm-up followed by a timed window of at least --window seconds.
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
from colmap_amd import feature_matching as FM  # noqa: E402


def make_sets(rows, count, seed=1):
    """count sets of `rows` descriptors: views of one scene -- noisy copies (sigma 12) of a base set, each permuted."""
    import match_reference as R
    rng = np.random.default_rng(seed)
    base = R.descriptors(rng, rows).astype(np.float32)
    sets = []
    for _ in range(count):
        noisy = np.clip(np.rint(base + 12.0 * rng.standard_normal(base.shape, dtype=np.float32)), 0, 255).astype(np.uint8)
        sets.append(np.ascontiguousarray(noisy[rng.permutation(rows)]))
    return sets


def window(fn, seconds, timing=None):
    """(calls, wall seconds, kernel ms summed) of fn() repeated for at least `seconds` after one warm-up call."""
    fn()
    calls, kernel_ms, t0 = 0, 0.0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if timing:
            kernel_ms += timing()[0]
        wall = time.perf_counter() - t0
        if wall >= seconds:
            return calls, wall, kernel_ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[2048, 8192, 32768])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    try:
        FM.FeatureMatcher().close()
    except (FM.FeatureMatchingError, RuntimeError) as e:
        sys.exit(f"bench_feature_matching needs a GPU: {e}")
    tile = FM.tile_rows()
    result = dict(tile_rows=tile, window_s=a.window, cases=[])
    for rows in a.rows:
        sets = make_sets(rows, max(a.batches) + 1)
        for B in a.batches:
            pairs = [(k + 1, k + 2) for k in range(B)]
            comparisons = B * rows * rows
            with FM.FeatureMatcher() as M:
                for k in range(B + 1):
                    M.set_descriptors(k + 1, sets[k])
                found = []
                calls, wall, kernel_ms = window(lambda: found.append(sum(len(m) for m in M.match_resident(pairs))), a.window,
                                                M.last_timing)

            def cold():
                with FM.FeatureMatcher() as C:
                    for k in range(B + 1):
                        C.set_descriptors(k + 1, sets[k])
                    C.match_resident(pairs)
            cold_calls, cold_wall, _ = window(cold, a.window)
            kernel_s, tiles = kernel_ms * 1e-3 / calls, 2 * B * ((rows + tile - 1) // tile)
            case = dict(rows=rows, batch_pairs=B, calls=calls, matches_per_call=found[-1], workgroups=tiles,
                        kernel_ms_per_call=1e3 * kernel_s, wall_ms_per_call=1e3 * wall / calls,
                        cold_ms_per_call=1e3 * cold_wall / cold_calls,
                        pairs_per_s_kernel=B / kernel_s, pairs_per_s_wall=B * calls / wall,
                        pairs_per_s_cold=B * cold_calls / cold_wall,
                        comparisons_per_s_kernel=comparisons / kernel_s, comparisons_per_s_wall=comparisons * calls / wall,
                        int8_macs_per_s_kernel=2 * 128 * comparisons / kernel_s,
                        streamed_bytes_per_call=tiles * rows * 132,
                        streamed_bytes_per_s_kernel=tiles * rows * 132 / kernel_s,
                        upload_bytes_cold=(B + 1) * FM.device_bytes(rows))
            result["cases"].append(case)
            print(json.dumps(case), flush=True)

    # for scale only: the numpy checker (tests/match_reference.py) on one pair of the smallest size, on the host CPU
    import match_reference as R
    rows = min(a.rows)
    s = make_sets(rows, 2)
    t0 = time.perf_counter()
    R.match(s[0], s[1])
    result["numpy_checker_for_scale_only"] = dict(rows=rows, seconds_per_pair=time.perf_counter() - t0)
    print(json.dumps(result["numpy_checker_for_scale_only"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
