"""`colmap feature_extractor` with the MI355X backend (reference exe/feature.cc:58-118 RunFeatureExtractor,
controllers/feature_extraction.cc, controllers/image_reader.cc):

    python -m colmap_amd feature_extractor --database_path DB --image_path IMAGES [--image_list_path LIST] \\
        [--ImageReader.camera_model SIMPLE_RADIAL] [--ImageReader.single_camera 0] [--ImageReader.camera_params f,cx,cy,k] \\
        [--FeatureExtraction.max_image_size 3200] [--SiftExtraction.max_num_features 8192] ...

reads the images of a folder as 8-bit grey, extracts SIFT keypoints and descriptors on the GPU with the arithmetic of the
reference's VLFeat route, and writes the `cameras`, `images`, `keypoints` and `descriptors` rows of the database, which is
created if absent. An image larger than max_image_size is scaled down first and its keypoints are scaled back
(ScaleKeypoints). Images that already have keypoints and descriptors are skipped. A new camera gets the focal length
default_focal_length_factor * max(width, height) and the principal point at the centre. With ImageReader.single_camera 1
the images ADDED BY ONE RUN share one camera, made for the first of them: as in the reference's ImageReader, which keeps
its previous camera for the length of a run only, a camera that an earlier run left in the database is not reused, so a
second run that adds images makes a second camera. Covariant / affine SIFT, domain
size pooling, ALIKED, masks, EXIF, per-folder cameras and the CPU extractor are not built and are refused by name.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional

import numpy as np

from . import camera as CAM
from . import database as DB
from . import feature_extraction as FE
from .matcher_cli import _flag

DEFAULT_MAX_IMAGE_SIZE = 3200  # FeatureExtractionOptions::EffMaxImageSize for SIFT
IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".tif", ".tiff", ".pgm", ".ppm", ".webp")


class FeatureExtractorError(RuntimeError):
    pass


def build_parser() -> argparse.ArgumentParser:
    """AddDatabaseOptions, AddImageOptions, AddFeatureExtractionOptions (controllers/option_manager.cc)."""
    ap = argparse.ArgumentParser(prog="feature_extractor", description=__doc__.split("\n\n")[0])
    d = FE.SiftExtractionOptions()
    ap.add_argument("--database_path", required=True)
    ap.add_argument("--image_path", required=True)
    ap.add_argument("--image_list_path", default="")
    ap.add_argument("--camera_mode", type=int, default=-1)
    ap.add_argument("--descriptor_normalization", default="l1_root", help="l1_root or l2")
    r = "--ImageReader."
    ap.add_argument(r + "mask_path", dest="mask_path", default="")
    ap.add_argument(r + "camera_mask_path", dest="camera_mask_path", default="")
    ap.add_argument(r + "camera_model", dest="camera_model", default="SIMPLE_RADIAL")
    ap.add_argument(r + "single_camera", dest="single_camera", type=_flag, default=False)
    ap.add_argument(r + "single_camera_per_folder", dest="single_camera_per_folder", type=_flag, default=False)
    ap.add_argument(r + "single_camera_per_image", dest="single_camera_per_image", type=_flag, default=False)
    ap.add_argument(r + "existing_camera_id", dest="existing_camera_id", type=int, default=-1)
    ap.add_argument(r + "camera_params", dest="camera_params", default="")
    ap.add_argument(r + "default_focal_length_factor", dest="default_focal_length_factor", type=float, default=1.2)
    f = "--FeatureExtraction."
    ap.add_argument(f + "type", dest="type", default="SIFT")
    ap.add_argument(f + "num_threads", dest="num_threads", type=int, default=-1, help="ignored")
    ap.add_argument(f + "use_gpu", dest="use_gpu", type=_flag, default=True)
    ap.add_argument(f + "gpu_index", dest="gpu_index", default="-1")
    ap.add_argument(f + "max_image_size", dest="max_image_size", type=int, default=-1)
    s = "--SiftExtraction."
    ap.add_argument(s + "max_num_features", dest="max_num_features", type=int, default=d.max_num_features)
    ap.add_argument(s + "first_octave", dest="first_octave", type=int, default=d.first_octave)
    ap.add_argument(s + "num_octaves", dest="num_octaves", type=int, default=d.num_octaves)
    ap.add_argument(s + "octave_resolution", dest="octave_resolution", type=int, default=d.octave_resolution)
    ap.add_argument(s + "peak_threshold", dest="peak_threshold", type=float, default=d.peak_threshold)
    ap.add_argument(s + "edge_threshold", dest="edge_threshold", type=float, default=d.edge_threshold)
    ap.add_argument(s + "max_num_orientations", dest="max_num_orientations", type=int, default=d.max_num_orientations)
    ap.add_argument(s + "upright", dest="upright", type=_flag, default=d.upright)
    ap.add_argument(s + "estimate_affine_shape", dest="estimate_affine_shape", type=_flag, default=False)
    ap.add_argument(s + "domain_size_pooling", dest="domain_size_pooling", type=_flag, default=False)
    ap.add_argument(s + "force_covariant_extractor", dest="force_covariant_extractor", type=_flag, default=False)
    ap.add_argument(s + "darkness_adaptivity", dest="darkness_adaptivity", type=_flag, default=False)
    return ap


def refusal(a: argparse.Namespace) -> str:
    """The message for a request that names something not built, or ''."""
    if a.estimate_affine_shape:
        return ("SiftExtraction.estimate_affine_shape is not built: it needs VLFeat's covariant detector and its affine "
                "shape adaptation")
    if a.domain_size_pooling:
        return "SiftExtraction.domain_size_pooling is not built: it needs the covariant extractor's descriptors over a range of scales"
    if a.force_covariant_extractor:
        return "SiftExtraction.force_covariant_extractor is not built: the covariant detector of VLFeat is missing"
    if a.darkness_adaptivity:
        return "SiftExtraction.darkness_adaptivity is not built: it exists only in SiftGPU's GLSL detector, whose arithmetic is not reproduced"
    if str(a.type).upper() != "SIFT":
        return f"FeatureExtraction.type {a.type} is not built: the ALIKED extractors need their networks; only SIFT is extracted"
    if not a.use_gpu:
        return "FeatureExtraction.use_gpu 0 is not built: there is no CPU extractor; the GPU extractor computes the CPU route's arithmetic"
    if a.mask_path or a.camera_mask_path:
        return "ImageReader.mask_path / camera_mask_path are not built: masked features (MaskFeatures) are missing"
    if a.single_camera_per_folder or a.single_camera_per_image:
        return ("ImageReader.single_camera_per_folder / single_camera_per_image are not built: every image gets its own "
                "camera, or all share one with ImageReader.single_camera 1")
    if a.existing_camera_id != -1:
        return "ImageReader.existing_camera_id is not built: cameras are always created by the command"
    if a.camera_mode >= 0:
        return "camera_mode is not built: use ImageReader.single_camera"
    if CAM_ID.get(a.camera_model) is None:
        return f"ImageReader.camera_model {a.camera_model} does not exist"
    if a.descriptor_normalization.upper() not in FE.NORMALIZATIONS:
        return f"descriptor_normalization {a.descriptor_normalization} does not exist: l1_root or l2"
    if not a.default_focal_length_factor > 0:
        return "ImageReader.default_focal_length_factor must be positive"
    if a.max_image_size == 0 or a.max_image_size < -1:
        return "FeatureExtraction.max_image_size must be positive (or -1 for the default of 3200)"
    return ""


CAM_ID = {m.name: i for i, m in enumerate(CAM.MODELS)}


def sift_options(a: argparse.Namespace) -> FE.SiftExtractionOptions:
    return FE.SiftExtractionOptions(max_num_features=a.max_num_features, first_octave=a.first_octave, num_octaves=a.num_octaves,
                                    octave_resolution=a.octave_resolution, peak_threshold=a.peak_threshold,
                                    edge_threshold=a.edge_threshold, max_num_orientations=a.max_num_orientations,
                                    upright=a.upright, normalization=FE.NORMALIZATIONS[a.descriptor_normalization.upper()])


def list_images(image_path: str, image_list_path: str = "") -> List[str]:
    """Names relative to image_path, sorted (GetRecursiveFileList + sort, image_reader.cc:60-80), or the lines of the list."""
    if image_list_path:
        with open(image_list_path) as f:
            return [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]
    names = []
    for root, _, files in os.walk(image_path):
        for fn in files:
            if fn.lower().endswith(IMAGE_EXTENSIONS):
                names.append(os.path.relpath(os.path.join(root, fn), image_path).replace(os.sep, "/"))
    return sorted(names)


def new_camera_params(model_id: int, width: int, height: int, focal_length: float) -> np.ndarray:
    """Camera::CreateFromModelId (scene/camera.cc): focal lengths, principal point at the centre, extras 0."""
    m = CAM.MODELS[model_id]
    p = np.zeros(m.num_params)
    if m.is_spherical:
        p[:] = [width, height]
        return p
    for i in m.focal_length_idxs:
        p[i] = focal_length
    p[m.principal_point_idxs[0]] = width / 2.0
    p[m.principal_point_idxs[1]] = height / 2.0
    return p


def thumbnail(grey: np.ndarray, max_image_size: int) -> np.ndarray:
    """Bitmap::Thumbnail (sensor/bitmap.cc:538-550): fits the longer side into max_image_size. The resampling filter is
    Pillow's bilinear one, not the reference's."""
    h, w = grey.shape
    if w <= max_image_size and h <= max_image_size:
        return grey
    from PIL import Image as PILImage
    scale = float(max_image_size) / max(w, h)
    nw, nh = int(np.floor(w * scale + 0.5)), int(np.floor(h * scale + 0.5))
    return np.ascontiguousarray(np.asarray(PILImage.fromarray(grey).resize((max(nw, 1), max(nh, 1)), PILImage.BILINEAR), np.uint8))


def scale_keypoints(kp6: np.ndarray, bitmap_width: int, bitmap_height: int, camera_width: int, camera_height: int) -> np.ndarray:
    """ScaleKeypoints (controllers/feature_extraction.cc:45-58)."""
    if bitmap_width == camera_width and bitmap_height == camera_height:
        return kp6
    scale_x = np.float32(camera_width) / np.float32(bitmap_width)
    scale_y = np.float32(camera_height) / np.float32(bitmap_height)
    return FE.rescale_keypoints(kp6, scale_x, scale_y)


def extract_into_database(database_path: str, image_path: str, image_names: Optional[List[str]] = None,
                          camera_model: str = "SIMPLE_RADIAL", single_camera: bool = False, camera_params: str = "",
                          options: Optional[FE.SiftExtractionOptions] = None, max_image_size: int = DEFAULT_MAX_IMAGE_SIZE,
                          default_focal_length_factor: float = 1.2, gpu_index: int = 0) -> Dict[str, int]:
    """FeatureExtractorController::Run over one GPU. Returns counts: extracted, skipped, features."""
    from . import workspace
    model_id = CAM_ID.get(camera_model)
    if model_id is None:
        raise FeatureExtractorError(f"camera model {camera_model} does not exist")
    params = None
    if camera_params:
        params = np.array([float(v) for v in camera_params.split(",")], np.float64)
        if len(params) != CAM.MODELS[model_id].num_params:
            raise FeatureExtractorError(f"ImageReader.camera_params has {len(params)} values, {camera_model} takes "
                                        f"{CAM.MODELS[model_id].num_params}")
    if not os.path.isdir(image_path):
        raise FeatureExtractorError(f"image_path {image_path} is not a directory")
    names = list_images(image_path) if image_names is None else list(image_names)
    stats = {"extracted": 0, "skipped": 0, "features": 0}
    with DB.Database(database_path, create=not os.path.isfile(database_path)) as db:
        db.create_verification_tables()   # a database made by the matchers' tests may lack cameras and keypoints
        known = {n: i for i, n in db.read_image_names().items()}
        cameras = db.read_cameras()
        shared_camera = None   # single_camera: the camera of this run's first new image (never one of an earlier run)
        with FE.SiftFeatureExtractor(options, gpu_index) as ex:
            for name in names:
                image_id = known.get(name)
                if image_id is not None and db.exists_keypoints(image_id) and db.exists_descriptors(image_id):
                    stats["skipped"] += 1
                    continue
                path = os.path.join(image_path, name)
                if not os.path.isfile(path):
                    raise FeatureExtractorError(f"image {path} does not exist")
                grey = workspace.read_bitmap_grey(path)
                h, w = grey.shape
                if image_id is None:
                    if single_camera and shared_camera is not None:
                        c = cameras[shared_camera]
                        if (c["width"], c["height"]) != (w, h):
                            raise FeatureExtractorError(f"image {name} is {w} x {h} but the single camera is {c['width']} x "
                                                        f"{c['height']}")
                        camera_id = shared_camera
                    else:
                        p = params if params is not None else new_camera_params(model_id, w, h, default_focal_length_factor * max(w, h))
                        camera_id = db.write_camera(model_id, w, h, p, prior_focal_length=params is not None)
                        cameras[camera_id] = {"model": model_id, "width": w, "height": h, "params": p,
                                              "prior_focal_length": params is not None}
                        if single_camera:
                            shared_camera = camera_id
                    image_id = db.write_image(name, camera_id)
                    known[name] = image_id
                small = thumbnail(grey, max_image_size)
                kp4, desc = ex.extract(small)
                kp6 = scale_keypoints(FE.keypoints_to_affine(kp4), small.shape[1], small.shape[0], w, h)
                if not db.exists_keypoints(image_id):
                    db.write_keypoints(image_id, kp6)
                if not db.exists_descriptors(image_id):
                    db.write_descriptors(image_id, desc.reshape(-1, 128))
                db.commit()
                stats["extracted"] += 1
                stats["features"] += len(kp6)
    return stats


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    why = refusal(a)
    if why:
        print(f"E {why}", file=sys.stderr)
        return 1
    try:
        opt = sift_options(a)
        first = str(a.gpu_index).split(",")[0].strip()
        names = list_images(a.image_path, a.image_list_path) if a.image_list_path else None
        stats = extract_into_database(a.database_path, a.image_path, names, a.camera_model, a.single_camera, a.camera_params, opt,
                                      DEFAULT_MAX_IMAGE_SIZE if a.max_image_size < 0 else a.max_image_size,
                                      a.default_focal_length_factor, max(int(first), 0))
    except (DB.DatabaseError, FE.FeatureExtractionError, FeatureExtractorError, OSError, ValueError) as e:
        print(f"E {e}", file=sys.stderr)
        return 1
    print(f"Extracted {stats['features']} features of {stats['extracted']} images, skipped {stats['skipped']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
