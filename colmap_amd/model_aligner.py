"""`colmap model_aligner` with the MI355X backend (reference exe/model.cc:257-424):

    python -m colmap_amd model_aligner --input_path SPARSE --output_path OUT --alignment_max_error E \\
        (--ref_model_path SPARSE_REF | --ref_images_path LOCATIONS.txt --ref_is_gps 0) [--alignment_type custom] \\
        [--min_common_images 3] [--merge_image_and_ref_origins 0] [--transform_path SIM3.txt]

moves a sparse model into the frame of reference positions of its cameras: the projection centres of a reference
model, or a text file with one `image_name x y z` per line. The similarity is estimated robustly
(AlignReconstructionToLocations, hypotheses scored on the GPU), applied to the model (points on the GPU), and the mean
and median distance of the aligned centres from their references is printed.

Not built: `--database_path`, GPS input (`--ref_is_gps 1`) and the alignment types plane, ecef, enu, enu-plane and
enu-plane-unscaled; asking for one of them is an error that says so.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import alignment as AL
from . import workspace as W
from .model_comparer import read_model
from .model_transformer import _parse_bool, transform_sparse_model

ALIGNMENT_TYPES = ("plane", "ecef", "enu", "enu-plane", "enu-plane-unscaled", "custom")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="model_aligner", description=__doc__.split("\n\n")[0])
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--database_path", default="")
    ap.add_argument("--ref_model_path", default="")
    ap.add_argument("--ref_images_path", default="")
    ap.add_argument("--ref_is_gps", type=_parse_bool, default=True)
    ap.add_argument("--merge_image_and_ref_origins", type=_parse_bool, default=False)
    ap.add_argument("--transform_path", default="")
    ap.add_argument("--alignment_type", default="custom", help="{plane, ecef, enu, enu-plane, enu-plane-unscaled, custom}")
    ap.add_argument("--min_common_images", type=int, default=3)
    ap.add_argument("--alignment_max_error", type=float, default=0.0)
    ap.add_argument("--gpu_index", type=int, default=0)
    return ap


def read_file_camera_locations(path: str):
    """ReadFileCameraLocations (exe/model.cc:129-147) for Cartesian coordinates: one `name x y z` per line."""
    names, locations = [], []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            parts = line.split()
            if len(parts) < 4:
                raise ValueError(f"{path}: expected `image_name x y z`, got `{line.strip()}`")
            names.append(parts[0])
            locations.append([float(v) for v in parts[1:4]])
    return names, np.array(locations, np.float64).reshape(-1, 3)


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    alignment_type = a.alignment_type.lower()
    if alignment_type not in ALIGNMENT_TYPES:
        print("E Invalid `alignment_type` - supported values are {'plane', 'ecef', 'enu', 'enu-plane', "
              "'enu-plane-unscaled', 'custom'}", file=sys.stderr)
        return 1
    if a.alignment_max_error <= 0:
        print("E You must provide a maximum alignment error > 0", file=sys.stderr)
        return 1
    if not a.ref_model_path and not a.database_path and not a.ref_images_path and alignment_type != "plane":
        print("E One of the following arguments must be specified: --ref_model_path, --database_path, "
              "--ref_images_path, --alignment_type=plane", file=sys.stderr)
        return 1
    if alignment_type != "custom":
        print(f"E alignment_type `{alignment_type}` is not built: only `custom` (Cartesian reference positions) is; "
              "plane, ecef, enu and enu-plane alignment need the principal-plane and GPS transforms", file=sys.stderr)
        return 1
    if a.database_path:
        print("E --database_path is not built: reference positions come from --ref_model_path or --ref_images_path",
              file=sys.stderr)
        return 1

    if a.ref_model_path:
        _, ref, ref_names_by_id = read_model(a.ref_model_path)
        ref_ids = sorted(ref.images)
        ref_names = [ref_names_by_id[i] for i in ref_ids]
        ref_locations = np.array([ref.ProjectionCenter(i) for i in ref_ids], np.float64).reshape(-1, 3)
    else:
        if a.ref_is_gps:
            print("E GPS reference positions are not built: give Cartesian coordinates with --ref_is_gps 0", file=sys.stderr)
            return 1
        print("Cartesian Alignment Coordinates extracted (MUST NOT BE GPS coords!).")
        ref_names, ref_locations = read_file_camera_locations(a.ref_images_path)
    if len(ref_locations) < a.min_common_images:
        print("E Cannot align with insufficient reference locations.", file=sys.stderr)
        return 1

    sm, rec, names = read_model(a.input_path)
    print(f"Aligning reconstruction to {alignment_type}\n=> Using {len(ref_names)} reference images")
    tform = AL.AlignReconstructionToLocations(rec, ref_names, ref_locations, a.min_common_images,
                                              AL.RANSACOptions(max_error=a.alignment_max_error), names, a.gpu_index)
    if tform is None:
        print("E => Alignment failed", file=sys.stderr)
        return 1
    transform_sparse_model(sm, tform, a.gpu_index)
    _, rec, _ = _reload(sm)
    by_name = {n: i for i, n in names.items()}
    errors = [float(np.linalg.norm(rec.ProjectionCenter(by_name[n]) - loc)) for n, loc in zip(ref_names, ref_locations)
              if n in by_name]
    print(f"=> Alignment error: {np.mean(errors):f} (mean), {W.percentile(errors, 50):f} (median)")

    if a.merge_image_and_ref_origins:
        for n, loc in zip(ref_names, ref_locations):
            if n in by_name:
                trans_align = loc - rec.ProjectionCenter(by_name[n])
                print(f"\n Aligning reconstruction's origin with ref origin: {' '.join(f'{v:.6g}' for v in loc)}\n")
                transform_sparse_model(sm, AL.Sim3d(1.0, np.array([1.0, 0.0, 0.0, 0.0]), trans_align), a.gpu_index)
                tform = AL.Sim3d(tform.scale, tform.rotation, np.asarray(tform.translation) + trans_align)
                break

    print("=> Alignment succeeded")
    os.makedirs(a.output_path, exist_ok=True)
    W.write_model_binary(sm, a.output_path)
    if a.transform_path:
        tform.ToFile(a.transform_path)
    return 0


def _reload(sm: W.SparseModel):
    from . import bundle_adjuster as BA
    return sm, BA.reconstruction_from_sparse_model(sm), None


if __name__ == "__main__":
    sys.exit(main())
