"""`colmap sequential_matcher` with the MI355X backend (reference exe/feature.cc:270-297):

    python -m colmap_amd sequential_matcher --database_path DB [--SequentialMatching.overlap 10] \\
        [--SequentialMatching.quadratic_overlap 1] [the matching options of exhaustive_matcher]

matches every image, in the order of the image names, with its next `overlap` images -- or, with quadratic overlap, with
the images 1, 2, 4, ... 2^(overlap-1) places later (SequentialPairGenerator). Loop detection and rig expansion are not
built.
"""
from __future__ import annotations

import argparse
import sys

from . import feature_matching as FM
from . import matcher_cli as CLI


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="sequential_matcher", description=__doc__.split("\n\n")[0])
    CLI.add_matching_options(ap)
    ap.add_argument("--SequentialMatching.overlap", dest="overlap", type=int, default=10)
    ap.add_argument("--SequentialMatching.quadratic_overlap", dest="quadratic_overlap", type=CLI._flag, default=True)
    ap.add_argument("--SequentialMatching.expand_rig_images", dest="expand_rig_images", type=CLI._flag, default=False)
    ap.add_argument("--SequentialMatching.loop_detection", dest="loop_detection", type=CLI._flag, default=False)
    ap.add_argument("--SequentialMatching.vocab_tree_path", dest="vocab_tree_path", default="")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if a.loop_detection:
        print("E SequentialMatching.loop_detection is not built: it needs the vocabulary tree (visual index and its "
              "retrieval), which is missing", file=sys.stderr)
        return 1
    if a.expand_rig_images:
        print("E SequentialMatching.expand_rig_images is not built: rigs and frames are not read from the database",
              file=sys.stderr)
        return 1
    return CLI.run(a, lambda db, names: FM.sequential_pair_blocks(FM.order_by_name(names), a.overlap, a.quadratic_overlap))


if __name__ == "__main__":
    sys.exit(main())
