"""`colmap geometric_verifier` with the MI355X backend (reference exe/feature.cc, controllers/feature_matching_utils.cc:595-662):

    python -m colmap_amd geometric_verifier --database_path DB [--TwoViewGeometry.max_error 4] \\
        [--TwoViewGeometry.min_num_inliers 15] [--TwoViewGeometry.multiple_models 0] [--batch_size 256]

estimates the two-view geometry of every matched image pair of the database on the GPU and writes the
`two_view_geometries` table. Built are the routes of EstimateTwoViewGeometry that need only a fundamental matrix and a
homography; a pair on a route that needs an essential matrix or a focal solver (calibrated, shared focal, one-sided
focal, spherical) is left WITHOUT a row -- the state the matchers leave, which the reference's geometric_verifier picks
up -- and counted per route on stderr. Pairs that have matches and inlier matches are skipped; a geometry row without
inliers is deleted and recomputed.
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional

import numpy as np

from . import database as DB
from . import two_view_geometry as TV
from .matcher_cli import _flag

DEFAULT_BATCH_SIZE = 256  # pairs per batch of point sets


def build_parser() -> argparse.ArgumentParser:
    """AddTwoViewGeometryOptions (controllers/option_manager.cc:347-380)."""
    ap = argparse.ArgumentParser(prog="geometric_verifier", description=__doc__.split("\n\n")[0])
    d, r = TV.TwoViewGeometryOptions(), TV.RANSACOptions()
    ap.add_argument("--database_path", required=True)
    g = "--TwoViewGeometry."
    ap.add_argument(g + "min_num_inliers", dest="min_num_inliers", type=int, default=d.min_num_inliers)
    ap.add_argument(g + "multiple_models", dest="multiple_models", type=_flag, default=d.multiple_models)
    ap.add_argument(g + "compute_relative_pose", dest="compute_relative_pose", type=_flag, default=False)
    ap.add_argument(g + "detect_watermark", dest="detect_watermark", type=_flag, default=d.detect_watermark)
    ap.add_argument(g + "multiple_ignore_watermark", dest="multiple_ignore_watermark", type=_flag, default=d.multiple_ignore_watermark)
    ap.add_argument(g + "watermark_detection_max_error", dest="watermark_detection_max_error", type=float,
                    default=d.watermark_detection_max_error)
    ap.add_argument(g + "filter_stationary_matches", dest="filter_stationary_matches", type=_flag, default=d.filter_stationary_matches)
    ap.add_argument(g + "stationary_matches_max_error", dest="stationary_matches_max_error", type=float,
                    default=d.stationary_matches_max_error)
    ap.add_argument(g + "use_degensac", dest="use_degensac", type=_flag, default=False)
    ap.add_argument(g + "max_error", dest="max_error", type=float, default=r.max_error)
    ap.add_argument(g + "confidence", dest="confidence", type=float, default=r.confidence)
    ap.add_argument(g + "max_num_trials", dest="max_num_trials", type=int, default=r.max_num_trials)
    ap.add_argument(g + "min_inlier_ratio", dest="min_inlier_ratio", type=float, default=r.min_inlier_ratio)
    ap.add_argument(g + "random_seed", dest="random_seed", type=int, default=r.random_seed)
    ap.add_argument("--FeatureMatching.rig_verification", dest="rig_verification", type=_flag, default=False)
    ap.add_argument("--FeatureMatching.guided_matching", dest="guided_matching", type=_flag, default=False)
    ap.add_argument("--FeatureMatching.num_threads", "--num_threads", dest="num_threads", type=int, default=-1, help="ignored")
    ap.add_argument("--FeatureMatching.gpu_index", "--gpu_index", dest="gpu_index", default="-1")
    ap.add_argument("--batch_size", type=int, default=DEFAULT_BATCH_SIZE, help="image pairs per batch of point sets")
    return ap


def refusal(a: argparse.Namespace) -> str:
    """The message for a request that names something not built, or ''."""
    if a.use_degensac:
        return ("TwoViewGeometry.use_degensac is not built: DEGENSAC's plane-and-parallax step is missing; the fundamental "
                "matrix comes from plain LO-RANSAC")
    if a.compute_relative_pose:
        return ("TwoViewGeometry.compute_relative_pose is not built: it needs the essential matrix decomposition and "
                "triangulation of EstimateTwoViewGeometryPose")
    if a.rig_verification:
        return "FeatureMatching.rig_verification is not built: it needs rigs, frames and generalized two-view geometry"
    if a.guided_matching:
        return "FeatureMatching.guided_matching is not built: guided verification needs MatchGuided on the descriptors"
    if a.batch_size < 1:
        return "batch_size must be positive"
    return ""


def geometry_options(a: argparse.Namespace) -> TV.TwoViewGeometryOptions:
    r = TV.RANSACOptions(max_error=a.max_error, confidence=a.confidence, max_num_trials=a.max_num_trials,
                         min_inlier_ratio=a.min_inlier_ratio, random_seed=a.random_seed)
    r.min_num_trials = min(r.min_num_trials, r.max_num_trials)
    return TV.TwoViewGeometryOptions(min_num_inliers=a.min_num_inliers, multiple_models=a.multiple_models,
                                     detect_watermark=a.detect_watermark, multiple_ignore_watermark=a.multiple_ignore_watermark,
                                     watermark_detection_max_error=a.watermark_detection_max_error,
                                     filter_stationary_matches=a.filter_stationary_matches,
                                     stationary_matches_max_error=a.stationary_matches_max_error, ransac_options=r)


def verify_matches(db: DB.Database, options: Optional[TV.TwoViewGeometryOptions] = None, gpu_index: int = 0,
                   batch_size: int = DEFAULT_BATCH_SIZE) -> Dict[str, object]:
    """Verifies the matched pairs of an open database (feature_matching_utils.cc:595-662) in pair-id order. Returns
    counts: verified, skipped, inliers, and not_built: route name -> pairs left without a row."""
    options = options or TV.TwoViewGeometryOptions()
    cameras = db.read_cameras()
    image_camera = db.read_image_camera_ids()
    stats = {"verified": 0, "skipped": 0, "inliers": 0, "not_built": {}, "num_scored": 0, "num_launches": 0}
    keypoints: Dict[int, np.ndarray] = {}

    def info(image_id: int) -> TV.CameraInfo:
        cid = image_camera[image_id]
        c = cameras[cid]
        return TV.CameraInfo(c["model"], c["width"], c["height"], cid, c["prior_focal_length"])

    def xy(image_id: int) -> np.ndarray:
        if image_id not in keypoints:
            keypoints[image_id] = db.read_keypoints(image_id)[:, :2].astype(np.float64)
        return keypoints[image_id]

    todo: List[int] = []
    for pid in db.read_matched_pair_ids():
        i1, i2 = DB.pair_id_to_image_pair(pid)
        if db.exists_inlier_matches(i1, i2):
            stats["skipped"] += 1
            continue
        todo.append(pid)
    with TV.PointSets(gpu_index) as ps:
        for at in range(0, len(todo), batch_size):
            batch = todo[at:at + batch_size]
            pairs = [DB.pair_id_to_image_pair(pid) for pid in batch]
            matches = [db.read_matches(i1, i2) for i1, i2 in pairs]
            sets = []
            for (i1, i2), m in zip(pairs, matches):
                p1, p2 = xy(i1), xy(i2)
                if len(m) and (m[:, 0].max() >= len(p1) or m[:, 1].max() >= len(p2)):
                    raise DB.DatabaseError(f"pair ({i1}, {i2}): a match points past the keypoints of its image")
                sets.append(np.hstack([p1[m[:, 0]], p2[m[:, 1]]]) if len(m) else np.zeros((0, 4)))
            geoms, s = ps.verify_pairs([info(i1) for i1, _ in pairs], [info(i2) for _, i2 in pairs], sets, batch, options)
            stats["num_scored"] += s["num_scored"]
            stats["num_launches"] += s["num_launches"]
            for (i1, i2), m, g in zip(pairs, matches, geoms):
                if g.config == TV.NOT_BUILT:
                    name = TV.route_name(g.route)
                    stats["not_built"][name] = stats["not_built"].get(name, 0) + 1
                    continue
                inliers = m[g.inlier_mask]
                db.delete_two_view_geometry(i1, i2)
                if len(inliers) < options.min_num_inliers:   # :652-655: the default geometry
                    db.write_two_view_geometry(i1, i2, np.zeros((0, 2), np.uint32), TV.UNDEFINED)
                else:
                    db.write_two_view_geometry(i1, i2, inliers, g.config, g.F, g.H)
                    stats["inliers"] += len(inliers)
                stats["verified"] += 1
            db.commit()
    return stats


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    why = refusal(a)
    if why:
        print(f"E {why}", file=sys.stderr)
        return 1
    try:
        with DB.Database(a.database_path) as db:
            first = str(a.gpu_index).split(",")[0].strip()
            stats = verify_matches(db, geometry_options(a), max(int(first), 0), a.batch_size)
    except (DB.DatabaseError, TV.TwoViewGeometryError, OSError) as e:
        print(f"E {e}", file=sys.stderr)
        return 1
    for name, count in sorted(stats["not_built"].items()):
        print(f"W the {name} route of EstimateTwoViewGeometry is not built: {count} pair{'s' if count != 1 else ''} left "
              "without a two_view_geometries row", file=sys.stderr)
    print(f"Verified {stats['verified']} image pairs ({stats['inliers']} inlier matches), skipped {stats['skipped']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
