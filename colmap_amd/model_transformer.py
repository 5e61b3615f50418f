"""`colmap model_transformer` with the MI355X backend (reference exe/model.cc:1081-1129):

    python -m colmap_amd model_transformer --input_path SPARSE_OR_PLY --output_path OUT --transform_path SIM3.txt \\
        [--is_inverse 0]

applies a stored similarity (one line: scale qw qx qy qz tx ty tz, Sim3d::ToFile) to a sparse model directory or to a
`.ply` point cloud. The points are transformed on the GPU; poses, rigs and frames on the host. Like the reference's
ImportPLY / ExportPLY, a PLY keeps positions and colours and drops its normals.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import alignment as AL
from . import bundle_adjuster as BA
from . import fusion
from . import workspace as W


def _parse_bool(v: str) -> bool:
    if str(v).lower() in ("1", "true", "yes", "on"):
        return True
    if str(v).lower() in ("0", "false", "no", "off"):
        return False
    raise argparse.ArgumentTypeError(f"not a boolean: {v}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="model_transformer", description=__doc__.split("\n\n")[0])
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--transform_path", required=True)
    ap.add_argument("--is_inverse", type=_parse_bool, default=False)
    ap.add_argument("--gpu_index", type=int, default=0)
    return ap


def transform_sparse_model(sm: W.SparseModel, tform: AL.Sim3d, gpu_index: int = 0):
    """Reconstruction::Transform on a file model, in place; tracks, colours and point errors stay as they are."""
    rec = BA.reconstruction_from_sparse_model(sm)
    AL.transform_reconstruction(rec, tform, gpu_index)
    for rid, rig in rec.rigs.items():  # sensor_from_rig translations scale with the model
        for cid, sfr in rig.sensors.items():
            if not rig.IsRefSensor(cid):
                sm.rigs[rid].sensors[(0, cid)] = BA._wxyz_t(sfr)
    for rid, rig in sm.rigs.items():  # the same for the rigs the Reconstruction keeps as trivial frames
        if rid in rec.rigs:
            continue
        for sid, pose in rig.sensors.items():
            if pose is not None and sid != rig.ref_sensor:
                rig.sensors[sid] = np.concatenate([pose[:4], tform.scale * np.asarray(pose[4:], np.float64)])
    BA.update_sparse_model(sm, rec, errors={pid: p.error for pid, p in sm.points3D.items()})


def transform_ply(input_path: str, output_path: str, tform: AL.Sim3d, gpu_index: int = 0) -> int:
    pts = fusion.read_binary_ply_points(input_path)
    moved = AL.transform_points(np.asarray(pts.xyz, np.float64), tform, gpu_index)
    out = fusion.FusedPoints(moved.astype(np.float32), np.zeros((len(moved), 3), np.float32), pts.rgb)
    fusion.write_binary_ply_points(output_path, out, write_normal=False, write_rgb=True)
    return len(moved)


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    is_dense = a.input_path.lower().endswith(".ply")
    if not is_dense and not os.path.isdir(a.input_path):
        print("E Invalid model input; not a PLY file or sparse reconstruction directory.", file=sys.stderr)
        return 1
    print(f"Reading transform input: {a.transform_path}")
    tform = AL.Sim3d.FromFile(a.transform_path)
    if a.is_inverse:
        tform = AL.Inverse(tform)
    print(f"Reading points input: {a.input_path}")
    if is_dense:
        n = transform_ply(a.input_path, a.output_path, tform, a.gpu_index)
        print(f"Applied transform to {n} points\nWriting output: {a.output_path}")
        return 0
    sm = W.read_sparse_model(a.input_path)
    print(f"Applying transform to recon with {len(sm.points3D)} points")
    transform_sparse_model(sm, tform, a.gpu_index)
    print(f"Writing output: {a.output_path}")
    os.makedirs(a.output_path, exist_ok=True)
    W.write_model_binary(sm, a.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
