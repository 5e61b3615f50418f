"""`python -m colmap_amd <command> [options]`: the commands of the `colmap` executable that sit on the
two MI355X paths (exe/colmap.cc command table)."""
import sys

COMMANDS = {
    "patch_match_stereo": ("colmap_amd.patch_match_stereo", "dense stereo on an undistorted workspace (exe/mvs.cc:228-279)"),
    "stereo_fusion": ("colmap_amd.fusion", "fuse depth / normal maps into a point cloud (exe/mvs.cc:299-386)"),
    "bundle_adjuster": ("colmap_amd.bundle_adjuster", "global bundle adjustment of a sparse model (exe/sfm.cc:175-206)"),
    "point_filtering": ("colmap_amd.point_filtering", "filter outlier observations and points of a sparse model (exe/sfm.cc:556-587)"),
    "image_undistorter": ("colmap_amd.image_undistorter", "undistort images into a dense workspace (exe/image.cc:325-430)"),
    "image_undistorter_standalone": ("colmap_amd.image_undistorter_standalone",
                                     "undistort images whose cameras come from a text list (exe/image.cc:427-523)"),
    "image_rectifier": ("colmap_amd.image_rectifier", "rectify and undistort stereo pairs, write Q (exe/image.cc:211-251)"),
    "color_extractor": ("colmap_amd.color_extractor", "colour the 3D points of a sparse model from its images (exe/sfm.cc:208-228)"),
    "model_comparer": ("colmap_amd.model_comparer", "align two sparse models and report per-image pose errors (exe/model.cc:520-631)"),
    "model_aligner": ("colmap_amd.model_aligner", "move a sparse model onto reference camera positions (exe/model.cc:257-424)"),
    "model_transformer": ("colmap_amd.model_transformer", "apply a stored similarity to a sparse model or a PLY (exe/model.cc:1081-1129)"),
    "feature_extractor": ("colmap_amd.feature_extractor", "extract SIFT features of the images of a folder into a database (exe/feature.cc:58-118)"),
    "exhaustive_matcher": ("colmap_amd.exhaustive_matcher", "match the SIFT descriptors of all image pairs of a database (exe/feature.cc:120-143)"),
    "sequential_matcher": ("colmap_amd.sequential_matcher", "match every image with the next ones in name order (exe/feature.cc:270-297)"),
    "matches_importer": ("colmap_amd.matches_importer", "match the image pairs a text file lists (exe/feature.cc:226-268)"),
    "geometric_verifier": ("colmap_amd.geometric_verifier", "estimate the two-view geometry of the matched pairs of a database (exe/feature.cc)"),
}

# matcher commands of the reference whose pairing is not built: named so that the message says what is missing
NOT_BUILT = {
    "vocab_tree_matcher": "vocabulary-tree pairing needs the visual index and its retrieval, which are missing",
    "spatial_matcher": "spatial pairing needs pose priors and a nearest-neighbour search over positions, which are missing",
    "transitive_matcher": "transitive pairing needs the graph of existing two-view geometries, which are never written here",
}

# other commands of the reference that are named so that the message says what is missing
NOT_BUILT_OTHER = {
    "feature_importer": "importing keypoints and descriptors from text files is missing; feature_extractor extracts them on the GPU",
}


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help", "help"):
        print("usage: python -m colmap_amd <command> [options]\n\ncommands:")
        for name, (_, what) in COMMANDS.items():
            print(f"  {name:28s} {what}")
        return 0
    if argv[0] in NOT_BUILT:
        print(f"E Command `{argv[0]}` is not built: {NOT_BUILT[argv[0]]}. exhaustive_matcher, sequential_matcher and "
              "matches_importer --match_type pairs are.", file=sys.stderr)
        return 1
    if argv[0] in NOT_BUILT_OTHER:
        print(f"E Command `{argv[0]}` is not built: {NOT_BUILT_OTHER[argv[0]]}.", file=sys.stderr)
        return 1
    if argv[0] not in COMMANDS:
        print(f"E Command `{argv[0]}` not recognized. To list the available commands, run `python -m colmap_amd help`.",
              file=sys.stderr)
        return 1
    import importlib
    return importlib.import_module(COMMANDS[argv[0]][0]).main(argv[1:])


if __name__ == "__main__":
    sys.exit(main())
