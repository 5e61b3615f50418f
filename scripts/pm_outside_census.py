#!/usr/bin/env python3
"""How much of a PatchMatch solve on the benchmark's geometry is tap work with a known answer? CPU only.

    python scripts/pm_outside_census.py [--w 320 --h 240 --iters 2] [--S 20] [--markdown]

Runs the oracle's census build (oracle/pm_oracle.py: run_census) on bench.py's scene at a reduced size -- the camera
ring with a 3.6 degree step, focal 2400 * W / 2560, S sources, the reference image in the middle, photometric with
filter -- and prints, per problem: the evaluations the oracle cuts at `src_var < 1e-5` and at `ref_var < 1e-5`
(ncc_finish returns 2.0f), the taps that fall wholly outside the source image and those on its border or outside. An
evaluation cut at src_var on this texture is a patch that lies wholly beside its source image: what the 11 x 11 wave
kernels answer without taps (colmap_amd/csrc/pm_patch_class.h). About three minutes on eight cores for 320 x 240 with two
iterations or 240 x 180 with five. MEASUREMENT INFRASTRUCTURE."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def census(w, h, iters, S):
    import pm_oracle
    from colmap_amd import synthetic as syn
    pm_oracle.build()
    views = syn.make_scene(S + 1, w, h, arc_deg=3.6 * S)
    ref = S // 2
    src = [i for i in range(S + 1) if i != ref]
    dmin, dmax = syn.depth_range(views, ref)
    o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=1, num_iterations=iters,
                                  order=1)
    t = time.time()
    _, counts = pm_oracle.run_census(o, syn.as_image_dicts(views), ref, src)
    return counts, time.time() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=320)
    ap.add_argument("--h", type=int, default=240)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--S", type=int, default=20)
    ap.add_argument("--markdown", action="store_true", help="print the row of the table in DESIGN.md 1.5")
    a = ap.parse_args()
    c, seconds = census(a.w, a.h, a.iters, a.S)
    ev, taps = max(c["ncc_evals"], 1), max(c["taps"], 1)
    if a.markdown:
        print("| problem | evaluations cut by `src_var < 1e-5` | cut by `ref_var < 1e-5` | taps fully outside (`tap_outside`) "
              "| border or outside (`tap_border`) |")
        print("|---|---|---|---|---|")
        print(f"| {a.w}x{a.h}, {a.iters} iterations | {100 * c['ncc_cut_src_var'] / ev:.1f} % "
              f"({c['ncc_cut_src_var'] / 1e6:.2f} M of {ev / 1e6:.1f} M) | {100 * c['ncc_cut_ref_var'] / ev:.1f} % | "
              f"{100 * c['tap_outside'] / taps:.1f} % | {100 * c['tap_border'] / taps:.1f} % |")
        return
    print(f"{a.w}x{a.h}, S = {a.S}, {a.iters} iterations, {seconds:.0f} s")
    print(f"  evaluations                   {ev}")
    print(f"  cut by src_var < 1e-5         {c['ncc_cut_src_var']}  ({100 * c['ncc_cut_src_var'] / ev:.1f} %)")
    print(f"  cut by ref_var < 1e-5         {c['ncc_cut_ref_var']}  ({100 * c['ncc_cut_ref_var'] / ev:.1f} %)")
    print(f"  taps                          {taps}")
    print(f"  fully outside (tap_outside)   {c['tap_outside']}  ({100 * c['tap_outside'] / taps:.1f} %)")
    print(f"  border or outside (tap_border) {c['tap_border']}  ({100 * c['tap_border'] / taps:.1f} %)")


if __name__ == "__main__":
    main()
