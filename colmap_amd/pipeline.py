"""pycolmap-style pipeline functions on the MI355X paths: `from colmap_amd.pipeline import
patch_match_stereo, stereo_fusion, bundle_adjustment, filter_points, undistort_images, rectify_images,
undistort_images_standalone, extract_colors`."""
# ---------------------------------------------------------------------------------------------
# pycolmap-style pipeline functions (reference pycolmap/pipeline/mvs.cc:119-127,182-193,
# pycolmap/pipeline/sfm.cc:153-161,258-263): same names, argument order and defaults. Imports are
# deferred so that importing this module stays light.
# ---------------------------------------------------------------------------------------------

def patch_match_stereo(workspace_path, workspace_format="COLMAP", pmvs_option_name="option-all", options=None,
                       config_path=""):
    """pycolmap.patch_match_stereo: runs PatchMatch stereo on an undistorted workspace (needs an MI355X)."""
    from . import model_statistics, mvs
    opt = options or mvs.PatchMatchOptions()
    if opt.gpu_index == "-1":
        opt.gpu_index = "0"
    ctl = mvs.PatchMatchController.FromWorkspace(opt, str(workspace_path), workspace_format.lower(), pmvs_option_name,
                                                 str(config_path),
                                                 model_statistics=model_statistics.DeviceStatistics(int(str(opt.gpu_index).split(",")[0])))
    ctl.Run()
    return ctl


def stereo_fusion(output_path, workspace_path, workspace_format="COLMAP", pmvs_option_name="option-all",
                  input_type="geometric", options=None, output_type="bin"):
    """pycolmap.stereo_fusion: fuses the depth / normal maps of a workspace and writes a model (bin / txt)
    or a PLY file + visibility; returns the fused points."""
    from . import fusion
    argv = ["--workspace_path", str(workspace_path), "--workspace_format", workspace_format,
            "--pmvs_option_name", pmvs_option_name, "--input_type", input_type, "--output_type", output_type,
            "--output_path", str(output_path)]
    opt = options or fusion.StereoFusionOptions()
    for name in ("mask_path", "num_threads", "max_image_size", "min_num_pixels", "max_num_pixels", "max_traversal_depth",
                 "max_reproj_error", "max_depth_error", "max_normal_error", "check_num_images", "use_cache", "cache_size"):
        argv += [f"--StereoFusion.{name}", str(getattr(opt, name))]
    if fusion.main(argv) != 0:
        raise RuntimeError("stereo_fusion failed")
    if output_type.lower() == "ply":
        return fusion.read_binary_ply_points(str(output_path))
    return None


def bundle_adjustment(reconstruction, options=None):
    """pycolmap.bundle_adjustment: BundleAdjustmentController on a colmap_amd.scene.Reconstruction, in place."""
    from . import bundle_adjuster, estimators
    ctl = bundle_adjuster.BundleAdjustmentController(options or estimators.BundleAdjustmentOptions(), reconstruction)
    ctl.Run()
    return ctl.summary


def filter_points(reconstruction, max_reproj_error=4.0, min_tri_angle=1.5, min_track_len=2, gpu_index=0):
    """`colmap point_filtering` on a colmap_amd.scene.Reconstruction, in place (needs an MI355X):
    ObservationManager.FilterAllPoints3D, then FilterPoints3DWithShortTracks; returns the filtered-observation count."""
    from . import observation_manager
    om = observation_manager.ObservationManager(reconstruction, gpu_index=gpu_index)
    return om.FilterAllPoints3D(max_reproj_error, min_tri_angle) + om.FilterPoints3DWithShortTracks(min_track_len)


def estimate_ba_covariance(options, reconstruction, bundle_adjuster):
    """pycolmap.estimate_ba_covariance (pycolmap/estimators/covariance.cc): covariances of a solved bundle adjustment
    on the GPU; None when they are not estimable."""
    from . import estimators
    return estimators.EstimateBACovariance(options, reconstruction, bundle_adjuster)


def undistort_images(output_path, input_path, image_path, image_names=None, output_type="COLMAP", copy_policy="copy",
                     num_patch_match_src_images=20, undistort_options=None):
    """pycolmap.undistort_images (pycolmap/pipeline/images.cc): undistorts the images of the sparse model at input_path
    into a dense workspace at output_path (needs an MI355X). Only the COLMAP output type is part of this package."""
    import os
    from . import undistortion, workspace
    if output_type != "COLMAP":
        raise ValueError("Invalid `output_type` - supported value is 'COLMAP'.")
    model = workspace.read_sparse_model(str(input_path))
    ids = []
    if image_names:
        by_name = {img.name: iid for iid, img in model.images.items()}
        ids = [by_name[n] for n in image_names if n in by_name]
    os.makedirs(str(output_path), exist_ok=True)
    opts = undistortion.COLMAPUndistorterOptions(num_patch_match_src_images=num_patch_match_src_images,
                                                 copy_type=str(copy_policy).lower().replace("_", "-"), image_ids=ids)
    ctl = undistortion.COLMAPUndistorter(opts, undistort_options or undistortion.UndistortCameraOptions(), model,
                                         str(image_path), str(output_path))
    ctl.Run()
    return ctl


def rectify_images(output_path, input_path, image_path, stereo_pairs, undistort_options=None, gpu_index=0):
    """`colmap image_rectifier` (exe/image.cc:211-251): rectifies and undistorts the stereo pairs -- (name1, name2) image
    names of the sparse model at input_path -- into `<output_path>/<name1>-<name2>/` with `Q.txt` (needs an MI355X)."""
    from . import undistortion, workspace
    model = workspace.read_sparse_model(str(input_path))
    by_name = {img.name: iid for iid, img in model.images.items()}
    pairs = []
    for name1, name2 in stereo_pairs:
        if name1 not in by_name or name2 not in by_name:
            raise ValueError(f"image {name1 if name1 not in by_name else name2} does not exist in the reconstruction")
        pairs.append((by_name[name1], by_name[name2]))
    ctl = undistortion.StereoImageRectifier(undistortion.StereoImageRectifierOptions(stereo_pairs=pairs, gpu_index=gpu_index),
                                            undistort_options or undistortion.UndistortCameraOptions(), model,
                                            str(image_path), str(output_path))
    ctl.Run()
    return ctl


def undistort_images_standalone(output_path, image_path, image_names_and_cameras, copy_policy="copy",
                                undistort_options=None, gpu_index=0):
    """`colmap image_undistorter_standalone` (exe/image.cc:427-523): undistorts (image name, camera) entries with no
    model on disk (needs an MI355X)."""
    from . import undistortion
    opts = undistortion.StandaloneImageUndistorterOptions(image_names_and_cameras=list(image_names_and_cameras),
                                                          copy_type=str(copy_policy).lower().replace("_", "-"),
                                                          gpu_index=gpu_index)
    ctl = undistortion.StandaloneImageUndistorter(opts, undistort_options or undistortion.UndistortCameraOptions(),
                                                  str(image_path), str(output_path))
    ctl.Run()
    return ctl


def extract_colors(image_path, input_path, output_path, gpu_index=0):
    """`colmap color_extractor` (exe/sfm.cc:208-228): reads the sparse model at input_path, gives every 3D point the mean
    colour of its observations in the images under image_path, writes the model to output_path and returns it (needs an
    MI355X)."""
    import os
    from . import color_extraction, workspace
    model = workspace.read_sparse_model(str(input_path))
    color_extraction.ExtractColorsForAllImages(model, str(image_path), gpu_index)
    os.makedirs(str(output_path), exist_ok=True)
    workspace.write_model_binary(model, str(output_path))
    return model


def align_reconstructions_via_reprojections(src_reconstruction, tgt_reconstruction, min_inlier_observations=0.3,
                                            max_reproj_error=8.0, gpu_index=0):
    """pycolmap.align_reconstructions_via_reprojections (estimators/alignment.cc:301-342): tgt_from_src as an
    alignment.Sim3d, or None; the hypotheses are scored on the GPU (needs an MI355X)."""
    from . import alignment
    return alignment.AlignReconstructionsViaReprojections(src_reconstruction, tgt_reconstruction, min_inlier_observations,
                                                          max_reproj_error, gpu_index=gpu_index)


def align_reconstructions_via_proj_centers(src_reconstruction, tgt_reconstruction, max_proj_center_error, gpu_index=0):
    """pycolmap.align_reconstructions_via_proj_centers (alignment.cc:344-369): tgt_from_src or None."""
    from . import alignment
    return alignment.AlignReconstructionsViaProjCenters(src_reconstruction, tgt_reconstruction, max_proj_center_error,
                                                        gpu_index=gpu_index)


def align_reconstructions_via_points(src_reconstruction, tgt_reconstruction, min_common_observations=3, max_error=0.005,
                                     min_inlier_ratio=0.9, gpu_index=0):
    """pycolmap.align_reconstructions_via_points (alignment.cc:400-458): tgt_from_src or None."""
    from . import alignment
    return alignment.AlignReconstructionsViaPoints(src_reconstruction, tgt_reconstruction, min_common_observations, max_error,
                                                   min_inlier_ratio, gpu_index)


def align_reconstruction_to_locations(src, tgt_image_names, tgt_image_locations, min_common_images, ransac_options,
                                      src_names=None, gpu_index=0):
    """pycolmap.align_reconstruction_to_locations (alignment.cc:185-238): tgt_from_src or None. A scene.Reconstruction
    carries no image names: give them as `src_names` (image_id -> name), or use image ids as names."""
    from . import alignment
    return alignment.AlignReconstructionToLocations(src, tgt_image_names, tgt_image_locations, min_common_images,
                                                    ransac_options, src_names, gpu_index)


def compare_reconstructions(reconstruction1, reconstruction2, alignment_error="reprojection", min_inlier_observations=0.3,
                            max_reproj_error=8.0, max_proj_center_error=0.1, names1=None, names2=None, gpu_index=0):
    """pycolmap.compare_reconstructions (CompareModels, exe/model.cc:575-631): a dict with rec2_from_rec1 and the
    per-image errors, or None where the alignment fails."""
    from . import model_comparer
    result = model_comparer.compare_models(reconstruction1, reconstruction2, names1, names2, alignment_error,
                                           min_inlier_observations, max_reproj_error, max_proj_center_error, gpu_index)
    return None if result is None else {"rec2_from_rec1": result[1], "errors": result[0]}


def extract_features(database_path, image_path, image_names=None, camera_model="SIMPLE_RADIAL", single_camera=False,
                     camera_params="", sift_options=None, max_image_size=3200, default_focal_length_factor=1.2, gpu_index=0):
    """pycolmap.extract_features (FeatureExtractorController, controllers/feature_extraction.cc) with the GPU SIFT
    extractor (needs an MI355X): reads the images of image_path, writes cameras, images, keypoints and descriptors of
    database_path (created if absent) and skips images that already have both. sift_options: a
    feature_extraction.SiftExtractionOptions. Returns the counts of images extracted and skipped and of features."""
    from . import feature_extractor as fe
    return fe.extract_into_database(database_path, image_path, image_names, camera_model, single_camera, camera_params,
                                    sift_options, max_image_size, default_focal_length_factor, gpu_index)


def match_exhaustive(database_path, matching_options=None, block_size=50, gpu_index=0, cache_bytes=0, batch_pairs=None):
    """pycolmap.match_exhaustive (ExhaustiveFeatureMatcher, controllers/feature_matching.cc) without geometric
    verification: matches all image pairs of the database on the GPU (needs an MI355X) and writes the `matches` table;
    no `two_view_geometries` row is written. matching_options: a feature_matching.SiftMatchingOptions. Returns the
    counts of pairs matched and skipped."""
    from . import database, feature_matching as fm
    with database.Database(database_path) as db:
        blocks = fm.exhaustive_pair_blocks(db.read_image_ids(), block_size)
        return fm.match_blocks(db, blocks, matching_options, gpu_index, cache_bytes, batch_pairs or fm.DEFAULT_BATCH_PAIRS)


def match_sequential(database_path, matching_options=None, overlap=10, quadratic_overlap=True, gpu_index=0, cache_bytes=0,
                     batch_pairs=None):
    """pycolmap.match_sequential (SequentialFeatureMatcher) without loop detection and geometric verification: every
    image, in name order, with its next `overlap` images (or 1, 2, 4, ... places later)."""
    from . import database, feature_matching as fm
    with database.Database(database_path) as db:
        blocks = fm.sequential_pair_blocks(fm.order_by_name(db.read_image_names()), overlap, quadratic_overlap)
        return fm.match_blocks(db, blocks, matching_options, gpu_index, cache_bytes, batch_pairs or fm.DEFAULT_BATCH_PAIRS)


def verify_matches(database_path, options=None, gpu_index=0, batch_size=None):
    """pycolmap.verify_matches (the geometric verification of controllers/feature_matching_utils.cc:595-662): estimates
    the two-view geometry of every matched pair of the database on the GPU (needs an MI355X) and writes
    `two_view_geometries`. options: a two_view_geometry.TwoViewGeometryOptions. Pairs on a route of
    EstimateTwoViewGeometry that is not built (calibrated, shared focal, one-sided focal, spherical) are left without a
    row and counted in the returned `not_built`."""
    from . import database, geometric_verifier as gv
    with database.Database(database_path) as db:
        return gv.verify_matches(db, options, gpu_index, batch_size or gv.DEFAULT_BATCH_SIZE)


def estimate_two_view_geometry(camera1, points1, camera2, points2, matches, options=None, stream_id=0, gpu_index=0):
    """pycolmap.estimate_two_view_geometry (EstimateTwoViewGeometry, estimators/two_view_geometry.cc:552-640) on the
    routes that need only a fundamental matrix and a homography. camera1 / camera2: two_view_geometry.CameraInfo;
    points [.][2+]; matches uint32 [n][2]. Raises for a pair on a route that is not built."""
    from . import two_view_geometry as tv
    return tv.estimate_two_view_geometry(camera1, points1, camera2, points2, matches, options, stream_id, gpu_index)
