"""`colmap matches_importer --match_type pairs` with the MI355X backend (reference exe/feature.cc:226-268):

    python -m colmap_amd matches_importer --database_path DB --match_list_path PAIRS.txt [--match_type pairs] \\
        [--ImagePairsMatching.block_size 1225] [the matching options of exhaustive_matcher]

matches the image pairs a text file lists, one `name1 name2` per line (ImportedPairGenerator). The `raw` and `inliers`
types, which import matches instead of computing them and verify them geometrically, are not built.
"""
from __future__ import annotations

import argparse
import os
import sys

from . import feature_matching as FM
from . import matcher_cli as CLI


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="matches_importer", description=__doc__.split("\n\n")[0])
    CLI.add_matching_options(ap)
    ap.add_argument("--match_list_path", required=True)
    ap.add_argument("--match_type", default="pairs", help="{pairs}")
    ap.add_argument("--ImagePairsMatching.block_size", dest="block_size", type=int, default=1225)
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if a.match_type in ("raw", "inliers"):
        print(f"E match_type {a.match_type} is not built: importing feature matches needs two-view geometry "
              "estimation (FeaturePairsFeatureMatcher), which is missing; only `pairs` runs here", file=sys.stderr)
        return 1
    if a.match_type != "pairs":
        print("E Invalid `match_type`", file=sys.stderr)
        return 1
    if not os.path.isfile(a.match_list_path):
        print(f"E match list {a.match_list_path} does not exist", file=sys.stderr)
        return 1
    return CLI.run(a, lambda db, names: FM.imported_pair_blocks(a.match_list_path, names, a.block_size))


if __name__ == "__main__":
    sys.exit(main())
