"""`colmap image_undistorter_standalone` on MI355X (reference exe/image.cc:427-523,
controllers/undistorters.cc:633-710):

    python -m colmap_amd image_undistorter_standalone --image_path IMAGES --input_file CAMERAS.txt --output_path OUT \\
        [--max_image_size 2000] [--blank_pixels 0] [--roi_min_x 0 ...] [--gpu_index 0]

undistorts images whose cameras come from a text file, one `name MODEL width height params...` per line, with no model
on disk.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Tuple

import numpy as np

from . import undistortion as U
from . import workspace as W
from .camera import MODELS


class UnknownCameraModel(ValueError):
    pass


def build_parser() -> argparse.ArgumentParser:
    d, c = U.UndistortCameraOptions(), U.StandaloneImageUndistorterOptions()
    ap = argparse.ArgumentParser(prog="image_undistorter_standalone", description=__doc__.split("\n\n")[0])
    ap.add_argument("--image_path", required=True)
    ap.add_argument("--input_file", required=True, help="text file: image_name CAMERA_MODEL width height camera_params")
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--copy_policy", default="copy", help="{copy, soft-link, hard-link}")
    ap.add_argument("--blank_pixels", type=float, default=d.blank_pixels)
    ap.add_argument("--min_scale", type=float, default=d.min_scale)
    ap.add_argument("--max_scale", type=float, default=d.max_scale)
    ap.add_argument("--max_image_size", type=int, default=d.max_image_size)
    for name in ("roi_min_x", "roi_min_y", "roi_max_x", "roi_max_y"):
        ap.add_argument(f"--{name}", type=float, default=getattr(d, name))
    ap.add_argument("--jpeg_quality", type=int, default=c.jpeg_quality)
    ap.add_argument("--gpu_index", type=int, default=0, help="(MI355X) the device the images are undistorted on")
    return ap


def parse_image_names_and_cameras(lines) -> List[Tuple[str, W.SparseCamera]]:
    """exe/image.cc:469-513: `image_name CAMERA_MODEL width height params...` per non-empty line. UnknownCameraModel for
    a model name that is not in the table; ValueError for a malformed line or a wrong parameter count (VerifyParams)."""
    ids = {m.name: i for i, m in enumerate(MODELS)}
    out = []
    for number, line in enumerate(lines, 1):
        line = line.strip()
        if not line:
            continue
        items = line.split()
        if len(items) < 4:
            raise ValueError(f"line {number}: expected `image_name CAMERA_MODEL width height camera_params`")
        name, model_name = items[0], items[1]
        if model_name not in ids:
            raise UnknownCameraModel(f"Camera model {model_name} does not exist")
        try:
            width, height = int(items[2]), int(items[3])
            params = np.array([float(v) for v in items[4:]], np.float64)
        except ValueError:
            raise ValueError(f"line {number}: width, height and the camera parameters are numbers") from None
        if width <= 0 or height <= 0:
            raise ValueError(f"line {number}: width and height must be positive")
        want = MODELS[ids[model_name]].num_params
        if len(params) != want:  # Camera::VerifyParams
            raise ValueError(f"line {number}: Check failed: camera.VerifyParams() ({model_name} takes {want} parameters, "
                             f"got {len(params)})")
        out.append((name, W.SparseCamera(len(out) + 1, ids[model_name], width, height, params)))
    return out


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if not os.path.isdir(a.image_path):
        print(f"E `image_path` is not a directory: {a.image_path}", file=sys.stderr)
        return 1
    if not os.path.isfile(a.input_file):
        print(f"E `input_file` is not a file: {a.input_file}", file=sys.stderr)
        return 1
    copy_type = a.copy_policy.lower().replace("_", "-")
    if copy_type not in ("copy", "soft-link", "hard-link"):
        print("E Invalid `copy_policy` - supported values are {'copy', 'soft-link', 'hard-link'}.", file=sys.stderr)
        return 1
    try:
        with open(a.input_file) as f:
            entries = parse_image_names_and_cameras(f)
    except ValueError as e:   # UnknownCameraModel included: exe/image.cc:495-498 exits with failure
        print(f"E {e}", file=sys.stderr)
        return 1
    opt = U.UndistortCameraOptions(blank_pixels=a.blank_pixels, min_scale=a.min_scale, max_scale=a.max_scale,
                                   max_image_size=a.max_image_size, roi_min_x=a.roi_min_x, roi_min_y=a.roi_min_y,
                                   roi_max_x=a.roi_max_x, roi_max_y=a.roi_max_y)
    try:
        ctl = U.StandaloneImageUndistorter(
            U.StandaloneImageUndistorterOptions(image_names_and_cameras=entries, copy_type=copy_type,
                                                jpeg_quality=a.jpeg_quality, gpu_index=a.gpu_index),
            opt, a.image_path, a.output_path)
        ctl.Run()
    except U.UndistortError as e:
        print(f"E {e}", file=sys.stderr)
        return 1
    print(f"Undistorted {len(ctl.image_names_)} images into {a.output_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
