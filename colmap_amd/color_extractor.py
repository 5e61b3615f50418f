"""`colmap color_extractor` on MI355X (reference exe/sfm.cc:208-228, scene/reconstruction.cc:1122-1184):

    python -m colmap_amd color_extractor --image_path IMAGES --input_path SPARSE --output_path OUT [--gpu_index 0]

reads the sparse model, gives every 3D point the mean colour of its observations in the source images and writes the
model.
"""
from __future__ import annotations

import argparse
import os
import sys

from . import color_extraction as CE
from . import workspace as W


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="color_extractor", description=__doc__.split("\n\n")[0])
    ap.add_argument("--image_path", required=True)
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--gpu_index", type=int, default=0, help="(MI355X) the device the colours are computed on")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if not os.path.isdir(a.image_path):
        print(f"E `image_path` is not a directory: {a.image_path}", file=sys.stderr)
        return 1
    if not os.path.isdir(a.input_path):
        print(f"E `input_path` is not a directory: {a.input_path}", file=sys.stderr)
        return 1
    model = W.read_sparse_model(a.input_path)
    try:
        num_read = CE.ExtractColorsForAllImages(model, a.image_path, a.gpu_index)
    except CE.ColorError as e:
        print(f"E {e}", file=sys.stderr)
        return 1
    os.makedirs(a.output_path, exist_ok=True)
    W.write_model_binary(model, a.output_path)
    print(f"Extracted the colours of {len(model.points3D)} points from {num_read} images into {a.output_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
