"""What `exhaustive_matcher`, `sequential_matcher` and `matches_importer` share (reference exe/feature.cc:120-268): the
reference's option names, the refusals of what is not built, and the run itself: read the database, generate pairs,
match them on the GPU in batched launches, write `matches`.

The commands behave like the reference's with `--FeatureMatching.skip_geometric_verification 1`, except that no
`two_view_geometries` row is written: the database is left with matches present and geometry absent, the state the
reference's `geometric_verifier` picks up.
"""
from __future__ import annotations

import argparse
import sys
from typing import Callable, Dict, Iterable, List, Tuple

from . import database as DB
from . import feature_matching as FM


def _flag(text: str) -> bool:
    if text.lower() in ("1", "true", "yes", "on"):
        return True
    if text.lower() in ("0", "false", "no", "off"):
        return False
    raise argparse.ArgumentTypeError(f"expected 0 or 1, got `{text}`")


def add_matching_options(ap: argparse.ArgumentParser):
    """AddFeatureMatchingOptions / AddTwoViewGeometryOptions (controllers/option_manager.cc), the options that apply."""
    ap.add_argument("--database_path", required=True)
    ap.add_argument("--FeatureMatching.type", dest="matcher_type", default="SIFT_BRUTEFORCE")
    ap.add_argument("--FeatureMatching.num_threads", dest="num_threads", type=int, default=-1, help="ignored")
    ap.add_argument("--FeatureMatching.use_gpu", dest="use_gpu", type=_flag, default=True)
    ap.add_argument("--FeatureMatching.gpu_index", dest="gpu_index", default="-1")
    ap.add_argument("--FeatureMatching.guided_matching", dest="guided_matching", type=_flag, default=False)
    ap.add_argument("--FeatureMatching.skip_geometric_verification", dest="skip_geometric_verification", type=_flag,
                    default=True, help="always on here: two-view geometry is not estimated")
    ap.add_argument("--FeatureMatching.rig_verification", dest="rig_verification", type=_flag, default=False)
    ap.add_argument("--FeatureMatching.skip_image_pairs_in_same_frame", dest="skip_same_frame", type=_flag, default=False)
    ap.add_argument("--FeatureMatching.max_num_matches", dest="max_num_matches", type=int, default=32768)
    ap.add_argument("--SiftMatching.max_ratio", dest="max_ratio", type=float, default=0.8)
    ap.add_argument("--SiftMatching.max_distance", dest="max_distance", type=float, default=0.7)
    ap.add_argument("--SiftMatching.cross_check", dest="cross_check", type=_flag, default=True)
    ap.add_argument("--SiftMatching.cpu_brute_force_matcher", dest="cpu_brute_force_matcher", type=_flag, default=False)
    ap.add_argument("--TwoViewGeometry.min_num_inliers", dest="min_num_inliers", type=int, default=15)
    ap.add_argument("--batch_pairs", type=int, default=FM.DEFAULT_BATCH_PAIRS, help="pairs per launch")
    ap.add_argument("--cache_bytes", type=int, default=0, help="device bytes for resident descriptor sets (0 = 4 GiB)")


def refusal(a: argparse.Namespace) -> str:
    """The message for a request that names something not built, or ''."""
    if a.matcher_type != "SIFT_BRUTEFORCE":
        return (f"FeatureMatching.type {a.matcher_type} is not built: ALIKED descriptors and the LightGlue matcher need "
                "their networks; only SIFT_BRUTEFORCE runs here")
    if not a.use_gpu or a.cpu_brute_force_matcher:
        return "FeatureMatching.use_gpu 0 / SiftMatching.cpu_brute_force_matcher 1: there is no CPU matcher, matching runs on the GPU"
    if a.guided_matching:
        return ("FeatureMatching.guided_matching is not built: it needs two-view geometry estimation and MatchGuided, "
                "run the reference's geometric_verifier on the written matches instead")
    if not a.skip_geometric_verification:
        return ("FeatureMatching.skip_geometric_verification 0 is not built: two-view geometry estimation is missing; "
                "the matches are written and geometric_verifier can pick them up")
    if a.rig_verification:
        return "FeatureMatching.rig_verification is not built: it needs rigs, frames and generalized two-view geometry"
    if a.skip_same_frame:
        return "FeatureMatching.skip_image_pairs_in_same_frame is not built: frames are not read from the database"
    return ""


def matching_options(a: argparse.Namespace) -> FM.SiftMatchingOptions:
    return FM.SiftMatchingOptions(max_ratio=a.max_ratio, max_distance=a.max_distance, cross_check=a.cross_check,
                                  max_num_matches=a.max_num_matches, min_num_inliers=a.min_num_inliers)


def gpu_index(a: argparse.Namespace) -> int:
    first = str(a.gpu_index).split(",")[0].strip()   # a list spreads pairs over devices in the reference; one device here
    return max(int(first), 0)


def run(a: argparse.Namespace, blocks_of: Callable[[DB.Database, Dict[int, str]], Iterable[List[Tuple[int, int]]]]) -> int:
    why = refusal(a)
    if why:
        print(f"E {why}", file=sys.stderr)
        return 1
    try:
        with DB.Database(a.database_path) as db:
            names = db.read_image_names()
            stats = FM.match_blocks(db, blocks_of(db, names), matching_options(a), gpu_index(a), a.cache_bytes, a.batch_pairs)
    except (DB.DatabaseError, FM.FeatureMatchingError, OSError) as e:
        print(f"E {e}", file=sys.stderr)
        return 1
    print(f"Matched {stats['matched']} image pairs ({stats['matches']} matches), skipped {stats['skipped']}")
    return 0
