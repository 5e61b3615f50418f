"""`colmap image_rectifier` on MI355X (reference exe/image.cc:211-251, controllers/undistorters.cc:712-820):

    python -m colmap_amd image_rectifier --image_path IMAGES --input_path SPARSE --output_path OUT \\
        --stereo_pairs_list PAIRS.txt [--max_image_size 2000] [--blank_pixels 0] [--gpu_index 0]

reads the sparse model and a list of image-name pairs (two names per line) and writes, per pair, a directory
`<name1>-<name2>` with the two rectified, undistorted images and the disparity-to-depth matrix `Q.txt`.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Tuple

from . import undistortion as U
from . import workspace as W


def build_parser() -> argparse.ArgumentParser:
    d = U.UndistortCameraOptions()
    ap = argparse.ArgumentParser(prog="image_rectifier", description=__doc__.split("\n\n")[0])
    ap.add_argument("--image_path", required=True)
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--stereo_pairs_list", required=True, help="text file with two image names per line")
    ap.add_argument("--blank_pixels", type=float, default=d.blank_pixels)
    ap.add_argument("--min_scale", type=float, default=d.min_scale)
    ap.add_argument("--max_scale", type=float, default=d.max_scale)
    ap.add_argument("--max_image_size", type=int, default=d.max_image_size)
    ap.add_argument("--gpu_index", type=int, default=0, help="(MI355X) the device the images are rectified on")
    return ap


def read_stereo_image_pairs(path: str, model: W.SparseModel) -> List[Tuple[int, int]]:
    """ReadStereoImagePairs (exe/image.cc:58-79): two names per non-empty line, both in the model; else ValueError."""
    by_name = {img.name: iid for iid, img in model.images.items()}
    pairs = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):   # ReadTextFileLines skips empty lines and comments
                continue
            names = line.split(" ")
            if len(names) != 2:
                raise ValueError(f"{path}:{number}: Check failed: names.size() == 2 ({len(names)} vs. 2)")
            for name in names:
                if name not in by_name:
                    raise ValueError(f"{path}:{number}: image {name} does not exist in the reconstruction")
            pairs.append((by_name[names[0]], by_name[names[1]]))
    return pairs


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if not os.path.isdir(a.image_path):
        print(f"E `image_path` is not a directory: {a.image_path}", file=sys.stderr)
        return 1
    if not os.path.isdir(a.input_path):
        print(f"E `input_path` is not a directory: {a.input_path}", file=sys.stderr)
        return 1
    if not os.path.isfile(a.stereo_pairs_list):
        print(f"E `stereo_pairs_list` is not a file: {a.stereo_pairs_list}", file=sys.stderr)
        return 1
    model = W.read_sparse_model(a.input_path)
    try:
        pairs = read_stereo_image_pairs(a.stereo_pairs_list, model)
    except ValueError as e:
        print(f"E {e}", file=sys.stderr)
        return 1
    opt = U.UndistortCameraOptions(blank_pixels=a.blank_pixels, min_scale=a.min_scale, max_scale=a.max_scale,
                                   max_image_size=a.max_image_size)
    ctl = U.StereoImageRectifier(U.StereoImageRectifierOptions(stereo_pairs=pairs, gpu_index=a.gpu_index), opt, model,
                                 a.image_path, a.output_path)
    try:
        ctl.Run()
    except U.UndistortError as e:
        print(f"E {e}", file=sys.stderr)
        return 1
    print(f"Rectified {len(ctl.pair_names_)} image pairs into {a.output_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
