"""`colmap model_comparer` with the MI355X backend (reference exe/model.cc:520-631):

    python -m colmap_amd model_comparer --input_path1 SPARSE1 --input_path2 SPARSE2 [--output_path OUT] \\
        [--alignment_error reprojection|proj_center] [--min_inlier_observations 0.3] [--max_reproj_error 8] \\
        [--max_proj_center_error 0.1]

reads two sparse models, aligns the first to the second -- by two-way reprojections of the common observations
(AlignReconstructionsViaReprojections, hypotheses scored on the GPU) or by projection centres
(AlignReconstructionsViaProjCenters) --, prints the per-image rotation and projection-centre error statistics and, with
`--output_path`, writes `errors.csv` and `errors_summary.txt` in the reference's format.
"""
from __future__ import annotations

import argparse
import io
import os
import sys

import numpy as np

from . import alignment as AL
from . import bundle_adjuster as BA
from . import workspace as W


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="model_comparer", description=__doc__.split("\n\n")[0])
    ap.add_argument("--input_path1", required=True)
    ap.add_argument("--input_path2", required=True)
    ap.add_argument("--output_path", default="")
    ap.add_argument("--alignment_error", default="reprojection", help="{reprojection, proj_center}")
    ap.add_argument("--min_inlier_observations", type=float, default=0.3)
    ap.add_argument("--max_reproj_error", type=float, default=8.0)
    ap.add_argument("--max_proj_center_error", type=float, default=0.1)
    ap.add_argument("--gpu_index", type=int, default=0)
    return ap


def read_model(path: str):
    """(SparseModel, scene.Reconstruction, image_id -> name) of a model directory."""
    sm = W.read_sparse_model(path)
    return sm, BA.reconstruction_from_sparse_model(sm), {i: im.name for i, im in sm.images.items()}


def write_comparison_errors_csv(path: str, errors):
    """WriteComparisonErrorsCSV (exe/model.cc:179-192)."""
    with open(path, "w") as f:
        f.write("# Model comparison pose errors: one entry per common image\n")
        f.write("# <rotation error (deg)>, <proj center error>\n")
        for e in errors:
            f.write(f"{e.rotation_error_deg:.17g}, {e.proj_center_error:.17g}\n")


def read_comparison_errors_csv(path: str) -> np.ndarray:
    with open(path) as f:
        rows = [[float(v) for v in line.split(",")] for line in f if line.strip() and not line.startswith("#")]
    return np.array(rows, np.float64).reshape(-1, 2)


def _stats(out, values):
    """PrintErrorStats over AlignmentErrorSummary::Statistics (alignment.cc:629-665): 6 significant digits like a stream."""
    for label, v in (("Min:    ", W.percentile(values, 0)), ("Max:    ", W.percentile(values, 100)),
                     ("Mean:   ", float(np.sum(values) / len(values))), ("Median: ", W.percentile(values, 50)),
                     ("P90:    ", W.percentile(values, 90)), ("P99:    ", W.percentile(values, 99))):
        out.write(f"{label}{v:.6g}\n")


def print_comparison_summary(out, errors):
    """PrintComparisonSummary (exe/model.cc:204-215)."""
    if not errors:
        out.write("Cannot extract error statistics from empty input\n")
        return
    out.write("\nRotation errors (degrees)\n")
    _stats(out, [e.rotation_error_deg for e in errors])
    out.write("\nProjection center errors\n")
    _stats(out, [e.proj_center_error for e in errors])


def compare_models(rec1, rec2, names1, names2, alignment_error="reprojection", min_inlier_observations=0.3,
                   max_reproj_error=8.0, max_proj_center_error=0.1, gpu_index=0):
    """CompareModels (exe/model.cc:575-631): (errors, rec2_from_rec1), or None where the alignment fails."""
    for k, rec in ((1, rec1), (2, rec2)):
        print(f"Reconstruction {k}\nImages: {len(rec.images)}\nPoints: {len(rec.points3D)}")
    print(f"Comparing reconstructed image poses\nCommon images: {len(AL.FindCommonRegImageIds(rec1, rec2, names1, names2))}")
    if alignment_error == "reprojection":
        sim = AL.AlignReconstructionsViaReprojections(rec1, rec2, min_inlier_observations, max_reproj_error, names1, names2,
                                                      gpu_index)
    elif alignment_error == "proj_center":
        sim = AL.AlignReconstructionsViaProjCenters(rec1, rec2, max_proj_center_error, names1, names2, gpu_index)
    else:
        print("E Invalid alignment_error specified.", file=sys.stderr)
        return None
    if sim is None:
        print("=> Reconstruction alignment failed")
        return None
    print("Computed alignment transform:\n" + "\n".join(" ".join(f"{v:.6g}" for v in row) for row in sim.ToMatrix()))
    errors = AL.ComputeImageAlignmentError(rec1, rec2, sim, names1, names2)
    print("Image alignment error summary")
    buf = io.StringIO()
    print_comparison_summary(buf, errors)
    print(buf.getvalue(), end="")
    return errors, sim


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if a.output_path and not os.path.isdir(a.output_path):
        print("E Provided output path is not a valid directory", file=sys.stderr)
        return 1
    _, rec1, names1 = read_model(a.input_path1)
    _, rec2, names2 = read_model(a.input_path2)
    result = compare_models(rec1, rec2, names1, names2, a.alignment_error, a.min_inlier_observations, a.max_reproj_error,
                            a.max_proj_center_error, a.gpu_index)
    if result is None:
        return 1
    if a.output_path:
        write_comparison_errors_csv(os.path.join(a.output_path, "errors.csv"), result[0])
        with open(os.path.join(a.output_path, "errors_summary.txt"), "w") as f:
            print_comparison_summary(f, result[0])
    return 0


if __name__ == "__main__":
    sys.exit(main())
