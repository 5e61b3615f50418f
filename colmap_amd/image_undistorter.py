"""`colmap image_undistorter` on MI355X (reference exe/image.cc:325-430, controllers/undistorters.cc:150-313):

    python -m colmap_amd image_undistorter --image_path IMAGES --input_path SPARSE --output_path DENSE \\
        [--max_image_size 2000] [--blank_pixels 0] [--roi_min_x 0 ...] [--gpu_index 0]

reads the sparse model and the distorted images and writes the dense workspace `patch_match_stereo` and
`stereo_fusion` start from: `images/` undistorted on the GPU, `sparse/` as PINHOLE cameras with the observations moved,
`stereo/patch-match.cfg`, `stereo/fusion.cfg` and the two `run-colmap-*.sh` scripts.
"""
from __future__ import annotations

import argparse
import os
import sys

from . import undistortion as U
from . import workspace as W


def build_parser() -> argparse.ArgumentParser:
    d, c = U.UndistortCameraOptions(), U.COLMAPUndistorterOptions()
    ap = argparse.ArgumentParser(prog="image_undistorter", description=__doc__.split("\n\n")[0])
    ap.add_argument("--image_path", required=True)
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--output_type", default="COLMAP", help="{COLMAP}; PMVS and CMP-MVS are not part of this package")
    ap.add_argument("--image_list_path", default="")
    ap.add_argument("--copy_policy", default="copy", help="{copy, soft-link, hard-link}")
    ap.add_argument("--num_patch_match_src_images", type=int, default=c.num_patch_match_src_images)
    ap.add_argument("--jpeg_quality", type=int, default=c.jpeg_quality)
    ap.add_argument("--blank_pixels", type=float, default=d.blank_pixels)
    ap.add_argument("--min_scale", type=float, default=d.min_scale)
    ap.add_argument("--max_scale", type=float, default=d.max_scale)
    ap.add_argument("--max_image_size", type=int, default=d.max_image_size)
    for name in ("roi_min_x", "roi_min_y", "roi_max_x", "roi_max_y"):
        ap.add_argument(f"--{name}", type=float, default=getattr(d, name))
    ap.add_argument("--gpu_index", type=int, default=0, help="(MI355X) the device the images are undistorted on")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if not os.path.isdir(a.image_path):  # exe/image.cc:371-379
        print(f"E `image_path` is not a directory: {a.image_path}", file=sys.stderr)
        return 1
    if not os.path.isdir(a.input_path):
        print(f"E `input_path` is not a directory: {a.input_path}", file=sys.stderr)
        return 1
    os.makedirs(a.output_path, exist_ok=True)
    if a.copy_policy.lower() not in ("copy", "soft-link", "hard-link"):  # :381-395
        print(f"E Invalid `copy_policy` - supported values are {{'copy', 'soft-link', 'hard-link'}}.", file=sys.stderr)
        return 1
    if a.output_type != "COLMAP":  # :416-420; the PMVS and CMP-MVS undistorters are not part of this package
        print("E Invalid `output_type` - supported values are {'COLMAP', 'PMVS', 'CMP-MVS'}.", file=sys.stderr)
        return 1
    model = W.read_sparse_model(a.input_path)
    image_ids = []
    if a.image_list_path:  # :397-405
        names = {ln.strip() for ln in open(a.image_list_path) if ln.strip()}
        by_name = {img.name: iid for iid, img in model.images.items()}
        for n in sorted(names):
            if n in by_name:
                image_ids.append(by_name[n])
            else:
                print(f"W Cannot find image {n}", file=sys.stderr)
    opt = U.UndistortCameraOptions(blank_pixels=a.blank_pixels, min_scale=a.min_scale, max_scale=a.max_scale,
                                   max_image_size=a.max_image_size, roi_min_x=a.roi_min_x, roi_min_y=a.roi_min_y,
                                   roi_max_x=a.roi_max_x, roi_max_y=a.roi_max_y)
    copts = U.COLMAPUndistorterOptions(num_patch_match_src_images=a.num_patch_match_src_images,
                                       copy_type=a.copy_policy.lower(), jpeg_quality=a.jpeg_quality,
                                       image_ids=image_ids, gpu_index=a.gpu_index)
    ctl = U.COLMAPUndistorter(copts, opt, model, a.image_path, a.output_path)
    ctl.Run()
    print(f"Undistorted {len(ctl.image_names_)} images into {a.output_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
