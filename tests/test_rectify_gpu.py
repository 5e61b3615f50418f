"""Stereo rectification on the GPU (undistort_rectify_images, undistort_warp_homography) against the numpy checker
tests/rectify_reference.py, and the two controllers that sit on it end to end.

Parity rule (the general rule): outputs are IDENTICAL, except that a pixel may differ by exactly 1
where (a) the checker's own double interpolant lies within 1e-4 of a half-integer, or (b) the source coordinate lies
within 1e-9 px of an integer (nearest: of a half-integer). Eligible pixels are counted from the checker alone and capped at
1 % per image. The rule applies to every model here: the homography puts one more rounding in front of the sample, so the
"no exception" class of plain undistortion is not claimed."""
import itertools
import os

import numpy as np
import pytest

import rectify_reference as RR
import test_undistort_gpu as G
import undistort_reference as R
from colmap_amd import undistortion as U
from colmap_amd import workspace as W

POSES = {"a": ((0.0, 0.05, 0.0), (0.1, 0.0, 0.0)),      # the reference's case (undistortion_test.cc:535-537)
         "b": ((0.1, 0.2, 0.3), (0.1, 0.2, 0.3))}       # large parts of the target fall outside the source
SIZES = [(61, 47), (64, 48)]
MODELS = [R.SIMPLE_RADIAL, R.OPENCV, R.OPENCV_FISHEYE]
PARITY_CASES = list(itertools.product(SIZES, (1, 3), ("bilinear", "nearest"), MODELS, sorted(POSES)))
PARITY_IDS = [f"{w}x{h}-{c}ch-{i}-{W.CAMERA_MODELS[m][0]}-pose_{p}" for (w, h), c, i, m, p in PARITY_CASES]


def source_camera(model, width, height, pp_shift=(0.0, 0.0)):
    if model == R.SIMPLE_RADIAL:  # k = 0.1
        cam = G.ba_camera(model, width, height, pp_shift)
        cam.params[3] = 0.1
        return cam
    return G.strong(G.ba_camera(model, width, height, pp_shift), 4.0)


def pose(name):
    euler, t = POSES[name]
    return RR.euler_to_rotation(*euler), np.array(t, np.float64)


def parity_inputs(size, channels, model, seed=5):
    w, h = size
    # pose (a) turns about the y axis only, so the row through the principal point maps to one source row: a principal
    # point on a whole or half pixel would put that whole row on a boundary of rule (b); hence the fractional shifts
    cam1, cam2 = source_camera(model, w, h, (0.37, -0.21)), source_camera(model, w, h, (1.3, -0.7))
    return cam1, cam2, R.noise_image(w, h, channels, seed), R.noise_image(w, h, channels, seed + 1)


def case_parity(size, channels, interp, model, pose_name):
    cam1, cam2, img1, img2 = parity_inputs(size, channels, model)
    Rm, t = pose(pose_name)
    opt = G._options(interp)
    got1, got2, out_cam, Q = U.RectifyAndUndistortStereoImages(opt, img1, img2, cam1, cam2, Rm, t)
    want_cam = U.UndistortCamera(opt, cam1)   # camera 1 only
    assert out_cam.model_id == U.PINHOLE and (out_cam.width, out_cam.height) == (want_cam.width, want_cam.height)
    assert np.array_equal(out_cam.params, want_cam.params)
    assert R.should_warp_directly(cam1, out_cam) and R.should_warp_directly(cam2, out_cam)
    want1, want2, want_Q = RR.rectify_pair(G._ref_cam(out_cam), cam1, cam2, img1, img2, Rm, t, interp)
    label = f"rectify {W.CAMERA_MODELS[model][0]} {size} {channels}ch {interp} pose {pose_name}"
    G.compare_under_parity_rule(got1, want1, None, label + " image 1")
    G.compare_under_parity_rule(got2, want2, None, label + " image 2")
    assert np.abs(Q - want_Q).max() <= 1e-10 * np.abs(want_Q).max()
    if pose_name == "b":
        # the baseline (0.1, 0.2, 0.3) is turned onto the x axis by 1.3 rad: at these focal lengths (nearly) the whole
        # target looks past the source, and what looks past it must be 0
        assert (want1.image == 0).mean() > 0.2 and (want2.image == 0).mean() > 0.2
    else:
        assert (want1.image != 0).mean() > 0.5 and (want2.image != 0).mean() > 0.5


ZERO_W_HINV = np.array([[1.0, 0.02, 0.3], [-0.01, 1.0, 0.2], [-0.125, 0.0, 1.3125]])   # w.z = 0 exactly at x = 10


def case_zero_w(interp, channels):
    """A homography whose third row is 0 at exact pixel centres: -0.125 (10 + 1/2) + 1.3125 == 0 in double."""
    cam = source_camera(R.OPENCV, 64, 48)
    target = R.Camera(R.PINHOLE, 61, 47, [80.0, 81.0, 30.2, 23.4])
    img = R.noise_image(64, 48, channels, 9)
    got = U.WarpImageWithHomographyBetweenCameras(U.WarpImageOptions(interpolation=interp), ZERO_W_HINV, cam, target, img)
    want = RR.warp_with_homography(ZERO_W_HINV, cam, target, img, interp)
    assert not got[:, 10].any() and not want.image[:, 10].any()
    assert (want.image[:, :9] != 0).mean() > 0.5   # left of the zero line the warp has content
    G.compare_under_parity_rule(got, want, None, f"w.z == 0 {interp} {channels}ch")


def case_indirect():
    """max_image_size = 20 on 61x47: ShouldWarpDirectly is false; the library's consistent indirect path."""
    cam1, cam2, img1, img2 = parity_inputs((61, 47), 3, R.OPENCV)
    Rm, t = pose("a")
    opt = G._options(max_image_size=20)
    got1, got2, out_cam, Q = U.RectifyAndUndistortStereoImages(opt, img1, img2, cam1, cam2, Rm, t)
    assert max(out_cam.width, out_cam.height) == 20 and not R.should_warp_directly(cam1, out_cam)
    ref_cam = G._ref_cam(out_cam)
    H1, H2, want_Q = RR.rectify_stereo_cameras(ref_cam, ref_cam, Rm, t)
    for got, cam, img, H in ((got1, cam1, img1, H1), (got2, cam2, img2, H2)):
        mid, want = RR.rectify_indirect(ref_cam, cam, img, H)
        assert mid.may_differ.sum() == 0 or mid.may_differ.mean() <= 0.01
        assert (mid.image != 0).mean() > 0.5
        G.compare_under_parity_rule(got, want, None, "indirect rectify OPENCV")
    assert np.abs(Q - want_Q).max() <= 1e-10 * np.abs(want_Q).max()


def case_reference_property():
    """undistortion_test.cc:515-560 with what the solid images imply: non-blank pixels are the colour, blank ones 0."""
    cam = R.Camera(R.SIMPLE_RADIAL, 100, 100, [100.0, 50.0, 50.0, 0.1])
    red = np.zeros((100, 100, 3), np.uint8)
    red[..., 0] = 255
    green = np.zeros((100, 100, 3), np.uint8)
    green[..., 1] = 255
    Rm, t = pose("a")
    o1, o2, out_cam, Q = U.RectifyAndUndistortStereoImages(U.UndistortCameraOptions(), red, green, cam, cam, Rm, t)
    assert W.CAMERA_MODELS[out_cam.model_id][0] == "PINHOLE"
    assert o1.shape == o2.shape == (out_cam.height, out_cam.width, 3)
    for o, colour in ((o1, (255, 0, 0)), (o2, (0, 255, 0))):
        blank = ~o.any(-1)
        assert (o[~blank] == np.array(colour, np.uint8)).all()
        assert 0 < (~blank).sum()
    assert Q.shape == (4, 4) and Q[3, 3] == 0.0


def case_batch():
    """Three pairs of different sizes in one call are bit-identical to three single calls."""
    pairs = []
    for k, (size, ch, model, pn) in enumerate([((61, 47), 1, R.SIMPLE_RADIAL, "a"), ((64, 48), 3, R.OPENCV, "b"),
                                               ((40, 30), 3, R.OPENCV_FISHEYE, "a")]):
        cam1, cam2, img1, img2 = parity_inputs(size, ch, model, seed=20 + k)
        pairs.append((img1, img2, cam1, cam2) + pose(pn))
    opt = G._options()
    together = U.RectifyAndUndistortStereoImagePairs(opt, pairs)
    assert len(together) == 3
    for p, (o1, o2, cam, Q) in zip(pairs, together):
        s1, s2, scam, sQ = U.RectifyAndUndistortStereoImages(opt, *p)
        assert np.array_equal(o1, s1) and np.array_equal(o2, s2) and np.array_equal(Q, sQ)
        assert (cam.width, cam.height) == (scam.width, scam.height) and np.array_equal(cam.params, scam.params)


def case_errors():
    """Every error is an argument the host refuses before a launch: a code plus undistort_last_error."""
    import ctypes as C
    cam1, cam2, img1, img2 = parity_inputs((64, 48), 1, R.SIMPLE_RADIAL)
    Rm, t = pose("a")
    opt = G._options()
    with pytest.raises(U.UndistortError, match="does not match"):      # size mismatch between camera and pixels
        U.RectifyAndUndistortStereoImages(opt, img1[:-1], img2, cam1, cam2, Rm, t)
    with pytest.raises(U.UndistortError, match="gpu_index"):
        U.RectifyAndUndistortStereoImages(opt, img1, img2, cam1, cam2, Rm, t, gpu_index=4096)
    with pytest.raises(U.UndistortError, match="blank_pixels"):
        U.RectifyAndUndistortStereoImages(G._options(blank_pixels=2.0), img1, img2, cam1, cam2, Rm, t)
    # the C ABI directly: a null buffer and an output buffer that is too small
    want = U.UndistortCamera(opt, cam1)
    out = np.empty((want.height, want.width), np.uint8)
    pair = U._StereoPair()
    U._fill_image(pair.image1, img1, cam1, out)
    U._fill_image(pair.image2, img2, cam2, out)
    pair.R[:] = list(Rm.reshape(9))
    pair.t[:] = list(t)
    copt = U._c_options(opt)
    lib = U.lib()
    pair.image2.out_capacity = out.nbytes - 1
    assert lib.undistort_rectify_images(C.byref(copt), 1, C.byref(pair), 0) != 0
    assert b"output buffer of" in lib.undistort_last_error() and b"needed" in lib.undistort_last_error()
    pair.image2.out_capacity = out.nbytes
    pair.image1.data = None
    assert lib.undistort_rectify_images(C.byref(copt), 1, C.byref(pair), 0) != 0
    assert b"null pixel buffer" in lib.undistort_last_error()


def two_image_model(tmp_path, model=R.OPENCV, size=(64, 48)):
    """A two-image sparse model with its images on disk (PNG, so that reading back is exact)."""
    w, h = size
    cam = source_camera(model, w, h)
    cams = {1: W.SparseCamera(1, cam.model_id, w, h, cam.params)}
    Rm, t = pose("a")
    # image 1 at the origin, image 2 = cam2_from_cam1
    tr = np.trace(Rm)
    qw = np.sqrt(1.0 + tr) / 2.0
    q2 = np.array([qw, (Rm[2, 1] - Rm[1, 2]) / (4 * qw), (Rm[0, 2] - Rm[2, 0]) / (4 * qw), (Rm[1, 0] - Rm[0, 1]) / (4 * qw)])
    images = {1: W.SparseImage(1, np.array([1.0, 0, 0, 0]), np.zeros(3), 1, "left/a.png"),
              2: W.SparseImage(2, q2, t, 1, "right/b.png")}
    image_dir = tmp_path / "images"
    from PIL import Image as PILImage
    bitmaps = {}
    for iid, img in images.items():
        os.makedirs(image_dir / os.path.dirname(img.name), exist_ok=True)
        bitmaps[iid] = R.noise_image(w, h, 3, 30 + iid)
        PILImage.fromarray(bitmaps[iid]).save(image_dir / img.name)
    return W.SparseModel(cameras=cams, images=images), str(image_dir), bitmaps


def case_rectifier_end_to_end(tmp_path):
    model, image_dir, bitmaps = two_image_model(tmp_path)
    out = tmp_path / "rectified"
    opt = U.UndistortCameraOptions()
    ctl = U.StereoImageRectifier(U.StereoImageRectifierOptions(stereo_pairs=[(1, 2)]), opt, model, image_dir, str(out))
    ctl.Run()
    pair_dir = out / "left-a.png-right-b.png"
    assert ctl.pair_names_ == ["left-a.png-right-b.png"] and pair_dir.is_dir()
    cam = model.cameras[1]
    Rm = model.images[2].RotationMatrix() @ model.images[1].RotationMatrix().T
    t = model.images[2].tvec - Rm @ model.images[1].tvec
    o1, o2, _, Q = U.RectifyAndUndistortStereoImages(opt, bitmaps[1], bitmaps[2], cam, cam, Rm, t)
    assert np.array_equal(U.read_bitmap(str(pair_dir / "left-a.png")), o1)
    assert np.array_equal(U.read_bitmap(str(pair_dir / "right-b.png")), o2)
    rows = [ln.split() for ln in open(pair_dir / "Q.txt").read().splitlines() if ln.strip()]
    assert len(rows) == 4 and all(len(r) == 4 for r in rows)
    assert np.abs(np.array(rows, np.float64) - Q).max() <= 1e-15 * np.abs(Q).max()   # repr() round-trips a double
    # an unreadable image logs an error and skips the pair
    os.remove(os.path.join(image_dir, "right", "b.png"))
    ctl = U.StereoImageRectifier(U.StereoImageRectifierOptions(stereo_pairs=[(1, 2)]), opt, model, image_dir,
                                 str(tmp_path / "again"))
    ctl.Run()
    assert ctl.pair_names_ == []


def case_standalone_end_to_end(tmp_path):
    model, image_dir, bitmaps = two_image_model(tmp_path, R.SIMPLE_RADIAL, (61, 47))
    cam = model.cameras[1]
    pinhole = W.SparseCamera(2, R.PINHOLE, 61, 47, np.array([70.0, 70.0, 30.5, 23.5]))
    entries = [("left/a.png", cam), ("right/b.png", pinhole), ("missing.png", cam)]
    out = tmp_path / "undistorted"
    opt = U.UndistortCameraOptions(blank_pixels=0.5)
    ctl = U.StandaloneImageUndistorter(U.StandaloneImageUndistorterOptions(image_names_and_cameras=entries), opt,
                                       image_dir, str(out))
    ctl.Run()
    assert sorted(ctl.image_names_) == ["left/a.png", "right/b.png"]
    want, _ = U.UndistortImage(opt, bitmaps[1], cam)
    assert np.array_equal(U.read_bitmap(str(out / "left" / "a.png")), want)
    # the copy branch copies the file byte for byte
    assert open(out / "right" / "b.png", "rb").read() == open(os.path.join(image_dir, "right", "b.png"), "rb").read()


# ---- the GPU runs ----------------------------------------------------------------------------------------------------

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", PARITY_CASES, ids=PARITY_IDS)
def test_rectify_parity(case):
    case_parity(*case)


@pytest.mark.parametrize("interp,channels", [("bilinear", 3), ("nearest", 1)])
def test_zero_third_coordinate_is_blank(interp, channels):
    case_zero_w(interp, channels)


def test_indirect_path():
    case_indirect()


def test_reference_property_solid_colours():
    case_reference_property()


def test_batch_is_bit_identical_to_single_calls():
    case_batch()


def test_errors():
    case_errors()


def test_stereo_image_rectifier_end_to_end(tmp_path):
    case_rectifier_end_to_end(tmp_path)


def test_standalone_image_undistorter_end_to_end(tmp_path):
    case_standalone_end_to_end(tmp_path)
