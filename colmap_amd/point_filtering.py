"""`colmap point_filtering` with the MI355X backend (reference exe/sfm.cc:556-587):

    python -m colmap_amd point_filtering --input_path SPARSE --output_path OUT \\
        [--min_track_len 2] [--max_reproj_error 4.0] [--min_tri_angle 1.5]

reads a sparse model (binary or text), drops observations with a large reprojection error and points with a small
triangulation angle (ObservationManager::FilterAllPoints3D), then points with short tracks
(FilterPoints3DWithShortTracks), prints the number of filtered observations and writes the model in the binary format.
"""
from __future__ import annotations

import argparse
import os
import sys

from . import bundle_adjuster as BA
from . import observation_manager as OM
from . import workspace as W


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="point_filtering", description=__doc__.split("\n\n")[0])
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--min_track_len", type=int, default=2)
    ap.add_argument("--max_reproj_error", type=float, default=4.0)
    ap.add_argument("--min_tri_angle", type=float, default=1.5)
    ap.add_argument("--gpu_index", type=int, default=0)
    return ap


def filter_model(sm: W.SparseModel, min_track_len: int, max_reproj_error: float, min_tri_angle: float,
                 gpu_index: int = 0, manager=None) -> int:
    """The body of the command on a file model, in place; `manager` replaces the ObservationManager class (tests)."""
    rec = BA.reconstruction_from_sparse_model(sm)
    om = manager(rec) if manager else OM.ObservationManager(rec, gpu_index=gpu_index)
    num_filtered = om.FilterAllPoints3D(max_reproj_error, min_tri_angle)
    num_filtered += om.FilterPoints3DWithShortTracks(min_track_len)
    for iid, img in rec.images.items():
        ids = sm.images[iid].point3D_ids
        for idx, p2 in enumerate(img.points2D):
            ids[idx] = p2.point3D_id
    for pid in list(sm.points3D):
        if pid not in rec.points3D:
            del sm.points3D[pid]
            continue
        sm.points3D[pid].track = list(rec.points3D[pid].track)
        if rec.points3D[pid].HasError():
            sm.points3D[pid].error = rec.points3D[pid].error
    return num_filtered


def main(argv=None, manager=None) -> int:
    a = build_parser().parse_args(argv)
    if not os.path.isdir(a.input_path):
        print("E `input_path` is not a directory", file=sys.stderr)
        return 1
    if not os.path.isdir(a.output_path):
        print("E `output_path` is not a directory", file=sys.stderr)
        return 1
    if a.min_track_len < 0:
        print("E `min_track_len` must not be negative", file=sys.stderr)
        return 1
    sm = W.read_sparse_model(a.input_path)
    num_filtered = filter_model(sm, a.min_track_len, a.max_reproj_error, a.min_tri_angle, a.gpu_index, manager)
    print(f"Filtered observations: {num_filtered}")
    W.write_model_binary(sm, a.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
