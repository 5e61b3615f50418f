"""`colmap exhaustive_matcher` with the MI355X backend (reference exe/feature.cc:120-143):

    python -m colmap_amd exhaustive_matcher --database_path DB [--ExhaustiveMatching.block_size 50] \\
        [--SiftMatching.max_ratio 0.8] [--SiftMatching.max_distance 0.7] [--SiftMatching.cross_check 1] \\
        [--FeatureMatching.max_num_matches 32768] [--TwoViewGeometry.min_num_inliers 15]

matches every pair of images of the database, block by block (ExhaustivePairGenerator), each block in batched launches,
and writes the `matches` table. Pairs that already have matches are skipped.
"""
from __future__ import annotations

import argparse
import sys

from . import feature_matching as FM
from . import matcher_cli as CLI


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="exhaustive_matcher", description=__doc__.split("\n\n")[0])
    CLI.add_matching_options(ap)
    ap.add_argument("--ExhaustiveMatching.block_size", dest="block_size", type=int, default=50)
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    return CLI.run(a, lambda db, names: FM.exhaustive_pair_blocks(sorted(names), a.block_size))


if __name__ == "__main__":
    sys.exit(main())
