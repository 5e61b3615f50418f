"""Image undistortion on the GPU (include/colmap_amd_undistort.h) against the numpy checker tests/undistort_reference.py.

The case functions are shared with tests/test_undistort_emul.py, which runs them through the CPU stand-in build of the
same source (tests/hip_emul/build_undistort.sh).

Warp parity rule: outputs are IDENTICAL, except that a pixel may differ by exactly 1 where
  (a) the checker's own double-valued interpolant lies within 1e-4 of a half-integer (float resolves 1.5e-5 at 255), or
  (b) the pixel's source coordinate lies within 1e-9 px of an integer (nearest: of a half-integer), where the border
      validity test / the choice of texel may flip
-- the two places where device libm vs host libm can legitimately decide differently. The pixels eligible under (a) or
(b) are counted from the checker alone and may be at most 1 % of an image; models whose projection has no transcendental
function must show no difference at all."""
import numpy as np
import pytest

import undistort_reference as R
from colmap_amd import undistortion as U

# the intrinsics of the bundle-adjustment tests (tests/test_ba_gpu.py), for 1024x768 images
BA_INTRINSICS = {
    R.SIMPLE_PINHOLE: (1280.0, 512.0, 384.0),
    R.PINHOLE: (1280.0, 1280.0, 512.0, 384.0),
    R.SIMPLE_RADIAL: (1280.0, 512.0, 384.0, 0.05),
    R.RADIAL: (1280.0, 512.0, 384.0, 0.05, -0.01),
    R.OPENCV: (1280.0, 1290.0, 512.0, 384.0, 0.05, -0.01, 0.001, -0.002),
    R.SIMPLE_RADIAL_FISHEYE: (900.0, 512.0, 384.0, 0.03),
    R.RADIAL_FISHEYE: (900.0, 512.0, 384.0, 0.03, -0.004),
    R.OPENCV_FISHEYE: (900.0, 910.0, 512.0, 384.0, 0.03, -0.004, 0.001, -0.0002),
    R.FOV: (900.0, 910.0, 512.0, 384.0, 0.6),
    R.SIMPLE_DIVISION: (900.0, 512.0, 384.0, -0.05),
    R.DIVISION: (900.0, 910.0, 512.0, 384.0, -0.05),
    R.SIMPLE_FISHEYE: (900.0, 512.0, 384.0),
    R.FISHEYE: (900.0, 910.0, 512.0, 384.0),
    R.EUCM: (900.0, 910.0, 512.0, 384.0, 0.56, 0.87),
    R.FULL_OPENCV: (900.0, 910.0, 512.0, 384.0, -0.05, 0.02, -0.001, 0.001, 0.001, 0.02, -0.02, 0.001),
    R.THIN_PRISM_FISHEYE: (900.0, 910.0, 512.0, 384.0, -0.05, 0.02, -0.001, 0.001, 0.001, 0.02, -0.02, 0.001),
    R.RAD_TAN_THIN_PRISM_FISHEYE: (900.0, 910.0, 512.0, 384.0, -0.0232, 0.0924, -0.0591, 0.003, 0.0048, -0.0009,
                                   0.0002, 0.0005, -0.0009, -0.0001, 0.00007, -0.00017),
}
PERSPECTIVE_MODELS = sorted(BA_INTRINSICS)
assert len(PERSPECTIVE_MODELS) == 17


def ba_camera(model, width=1024, height=768, pp_shift=(0.0, 0.0)):
    """The BA test camera of `model`, scaled from 1024x768 to width x height (distortion coefficients are resolution
    independent), with its principal point moved by pp_shift pixels."""
    p = np.array(BA_INTRINSICS[model], np.float64)
    sx, sy = width / 1024.0, height / 768.0
    if model in R.ONE_FOCAL:
        p[0] *= 0.5 * (sx + sy)
        p[1] = p[1] * sx + pp_shift[0]
        p[2] = p[2] * sy + pp_shift[1]
    else:
        p[0] *= sx
        p[1] *= sy
        p[2] = p[2] * sx + pp_shift[0]
        p[3] = p[3] * sy + pp_shift[1]
    return R.Camera(model, width, height, p)


def strong(cam, factor):
    """The same camera with `factor` times the distortion (FOV / EUCM keep theirs: their parameters are not small)."""
    if cam.model_id in (R.FOV, R.EUCM):
        return cam
    n_intr = 3 if cam.model_id in R.ONE_FOCAL else 4
    p = cam.params.copy()
    p[n_intr:] *= factor
    return R.Camera(cam.model_id, cam.width, cam.height, p)


def make_image(kind, width, height, channels, seed):
    if kind == "gradient":
        img = R.gradient_image(width, height)
        return img if channels == 3 else img[..., 2].copy()
    return R.noise_image(width, height, channels, seed)


# (model, image kind, channels, interpolation, principal-point shift, option overrides). The gradient image is a linear
# ramp, so its interpolant IS the source coordinate: a principal point on a half pixel would put whole rows and columns
# exactly on a rounding boundary (case (a)); the gradient cases therefore shift it by a fraction.
WARP_CASES = [
    (R.SIMPLE_RADIAL, "noise", 1, "bilinear", (0, 0), {}),
    (R.SIMPLE_RADIAL, "gradient", 3, "bilinear", (2.3, -1.7), dict(blank_pixels=1.0)),
    (R.SIMPLE_RADIAL, "noise", 3, "nearest", (7.5, -4.25), dict(blank_pixels=0.5)),
    (R.OPENCV, "noise", 3, "bilinear", (9.0, -6.5), dict(blank_pixels=0.5)),
    (R.OPENCV, "gradient", 1, "nearest", (1.3, 0.6), {}),
    (R.FULL_OPENCV, "noise", 1, "bilinear", (0, 0), dict(blank_pixels=1.0, roi_min_x=0.1, roi_min_y=0.2, roi_max_x=0.9, roi_max_y=0.8)),
    (R.FULL_OPENCV, "gradient", 3, "bilinear", (-5.2, 3.4), {}),
    (R.OPENCV_FISHEYE, "noise", 3, "bilinear", (0, 0), dict(blank_pixels=0.5)),
    (R.OPENCV_FISHEYE, "noise", 1, "nearest", (4.2, 3.9), dict(max_image_size=100)),
    (R.THIN_PRISM_FISHEYE, "noise", 1, "bilinear", (6.0, -3.0), dict(blank_pixels=1.0)),
    (R.THIN_PRISM_FISHEYE, "gradient", 3, "bilinear", (0.7, 1.1), {}),
    (R.FOV, "noise", 3, "bilinear", (0, 0), dict(blank_pixels=1.0, max_image_size=120)),
    (R.FOV, "gradient", 1, "bilinear", (3.3, 2.1), {}),
    (R.DIVISION, "noise", 1, "bilinear", (0, 0), dict(blank_pixels=0.5, roi_min_x=0.05, roi_max_y=0.9)),
    (R.DIVISION, "noise", 3, "nearest", (-8.0, 5.0), {}),
    (R.EUCM, "noise", 3, "bilinear", (0, 0), dict(blank_pixels=1.0)),
    (R.EUCM, "gradient", 1, "bilinear", (5.3, -2.6), dict(max_image_size=110)),
    (R.RADIAL, "noise", 1, "bilinear", (0, 0), dict(blank_pixels=1.0)),
    (R.RAD_TAN_THIN_PRISM_FISHEYE, "noise", 1, "bilinear", (0, 0), dict(blank_pixels=0.5)),
]
WARP_IDS = [f"{U.W.CAMERA_MODELS[c[0]][0]}-{c[1]}-{c[2]}ch-{c[3]}-{i}" for i, c in enumerate(WARP_CASES)]
W0, H0 = 160, 120


def _options(interp="bilinear", **kw):
    o = U.UndistortCameraOptions(**kw)
    o.warp_options.interpolation = interp
    return o


def _ref_cam(c):
    return R.Camera(c.model_id, c.width, c.height, c.params)


def compare_under_parity_rule(got, want: R.WarpResult, model=None, label=""):
    """-> (pixels that differ, eligible pixels); asserts the rule of the module docstring."""
    assert got.shape == want.image.shape, (got.shape, want.image.shape)
    d = np.abs(got.astype(np.int32) - want.image.astype(np.int32))
    d = d if d.ndim == 2 else d.max(-1)
    eligible = want.may_differ
    share = eligible.mean()
    print(f"{label}: {got.shape}, differing pixels {int((d > 0).sum())}, max |d| {int(d.max())}, "
          f"eligible (a) {int(want.near_half.sum())} (b) {int(want.near_edge.sum())} = {share:.2e} of the image")
    assert share <= 0.01, f"{share:.3%} of the pixels are eligible for the exception: the test image proves too little"
    assert d.max() <= 1, f"a pixel differs by {d.max()}"
    bad = (d > 0) & ~eligible
    assert not bad.any(), f"{int(bad.sum())} pixels differ outside the exception, first at {np.argwhere(bad)[:5].tolist()}"
    if model is not None and model in R.NO_TRANSCENDENTAL:
        assert d.max() == 0, "a model without a transcendental function must match exactly"
    return int((d > 0).sum()), int(eligible.sum())


def case_warp(model, kind, channels, interp, pp_shift, overrides, seed=3):
    cam = strong(ba_camera(model, W0, H0, pp_shift), 4.0)  # visible distortion at this size
    img = make_image(kind, W0, H0, channels, seed)
    opt = _options(interp, **overrides)
    got, out_cam = U.UndistortImage(opt, img, cam)
    assert out_cam.model_id == U.PINHOLE
    assert (out_cam.width, out_cam.height) == (U.UndistortCamera(opt, cam).width, U.UndistortCamera(opt, cam).height)
    assert R.should_warp_directly(cam, out_cam), "these cases are direct warps"
    if "max_image_size" in overrides:
        assert max(out_cam.width, out_cam.height) <= overrides["max_image_size"]
    want = R.warp(cam, _ref_cam(out_cam), img, interp)
    compare_under_parity_rule(got, want, model, f"warp {U.W.CAMERA_MODELS[model][0]} {kind} {channels}ch {interp}")
    if overrides.get("blank_pixels", 0.0) == 0.0 and "roi_min_x" not in overrides:
        assert (got == 0).mean() < 0.02   # blank_pixels = 0: (nearly) every pixel has a source
    return got, out_cam


def case_points(model):
    cam = ba_camera(model)
    und = U.UndistortCamera(U.UndistortCameraOptions(), cam)
    xs, ys = np.meshgrid(np.linspace(0.5, cam.width - 0.5, 24), np.linspace(0.5, cam.height - 0.5, 18))
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    if model == R.EUCM:  # beyond the model's domain: CamFromImg has no value (sensor/models.h:2815-2826)
        far = np.array([[-4000.0, 384.0], [512.0, 5000.0], [6000.0, 6000.0], [-3500.0, -3500.0]])
        xy = np.concatenate([xy, far], 0)
    got = U.UndistortPoints(cam, und, xy)
    want = R.undistort_points(cam, _ref_cam(und), xy)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if model == R.EUCM:
        assert np.isnan(want[-4:]).all() and not np.isnan(want[:-4]).any()
    else:
        assert not np.isnan(want).any()
    err = np.nanmax(np.abs(got - want))
    print(f"points {U.W.CAMERA_MODELS[model][0]}: max |d| {err:.3e} px over {len(xy)} observations")
    assert err <= 1e-6
    assert np.abs(got - xy)[~np.isnan(got[:, 0])].max() > 1e-3 or model in (R.SIMPLE_PINHOLE, R.PINHOLE)


def case_points_spherical():
    cam = R.Camera(R.EQUIRECTANGULAR, 1000, 500, [1000.0, 500.0])
    und = R.Camera(R.EQUIRECTANGULAR, 250, 125, [250.0, 125.0])
    got = U.UndistortPoints(cam, und, np.array([[600.0, 200.0], [100.0, 400.0]]))
    np.testing.assert_allclose(got, [[150.0, 50.0], [25.0, 100.0]], atol=1e-9)   # undistortion_test.cc:470-480


def case_resize():
    for (w, h, ch, tw, th, seed) in [(160, 120, 1, 61, 47, 1), (160, 120, 3, 40, 30, 2), (97, 131, 3, 33, 70, 3),
                                     (100, 100, 1, 84, 84, 4), (64, 48, 3, 64, 48, 5)]:
        img = R.noise_image(w, h, ch, seed)
        got = U.ResizeBitmap(img, tw, th)
        compare_under_parity_rule(got, R.resize(img, tw, th), None, f"resize {w}x{h}x{ch} -> {tw}x{th}")
        if (w, h) == (tw, th):
            assert np.array_equal(got, img)


def case_indirect_property():
    """undistortion_test.cc:264-314: the gradient image through the direct and through the indirect path."""
    cam = R.Camera(R.SIMPLE_RADIAL, 100, 100, [100.0, 50.0, 50.0, 0.5])
    img = R.gradient_image(100, 100)
    opt = _options()
    direct, direct_cam = U.UndistortImage(opt, img, cam)
    assert min(direct_cam.width / 100, direct_cam.height / 100) >= opt.warp_options.direct_warp_min_scale
    opt.warp_options.direct_warp_min_scale = 1.0
    resized, resized_cam = U.UndistortImage(opt, img, cam)
    assert (resized_cam.width, resized_cam.height) == (direct_cam.width, direct_cam.height) == (84, 84)
    assert np.array_equal(resized_cam.params, direct_cam.params)
    assert resized.shape == direct.shape
    assert not np.array_equal(resized, direct)
    d = np.abs(resized.astype(np.int32) - direct.astype(np.int32))
    print(f"indirect vs direct: mean |d| {d.mean():.4f}, max |d| {d.max()}")
    assert d.mean() < 0.5
    assert d.max() <= 1
    # and the indirect result is what the checker's warp at source resolution + resize gives
    mid = R.warp(cam, R.rescaled(_ref_cam(direct_cam), 100, 100), img)
    assert mid.may_differ.mean() <= 0.01
    want = R.resize(mid.image, 84, 84)
    d2 = np.abs(resized.astype(np.int32) - want.image.astype(np.int32))
    assert d2.max() <= 1 and (d2 > 0).mean() <= 0.01   # a flip of an intermediate pixel may move a final rounding


def case_indirect_small_target():
    """min(target / source) < direct_warp_min_scale = 0.5: max_image_size forces the indirect path."""
    cam = strong(ba_camera(R.OPENCV, W0, H0), 4.0)
    img = R.noise_image(W0, H0, 3, 11)
    opt = _options(blank_pixels=1.0, max_image_size=64)
    got, out_cam = U.UndistortImage(opt, img, cam)
    assert max(out_cam.width, out_cam.height) == 64 and not R.should_warp_directly(cam, out_cam)
    mid = R.warp(cam, R.rescaled(_ref_cam(out_cam), W0, H0), img)
    assert mid.may_differ.sum() == 0 or mid.may_differ.mean() <= 0.01
    compare_under_parity_rule(got, R.resize(mid.image, out_cam.width, out_cam.height), None, "indirect OPENCV")


def case_blank_pixels():
    """undistortion_test.cc:181-262 on an all-255 image."""
    cam = R.Camera(R.SIMPLE_RADIAL, 100, 100, [100.0, 50.0, 50.0, 0.5])
    img = np.full((100, 100), 255, np.uint8)
    got, c = U.UndistortImage(_options(blank_pixels=0.0), img, cam)
    assert (c.width, c.height) == (84, 84) and tuple(c.params) == (100.0, 100.0, 42.0, 42.0)
    assert got.shape == (84, 84) and (got != 0).all()
    got, c = U.UndistortImage(_options(blank_pixels=1.0), img, cam)
    assert (c.width, c.height) == (90, 90) and tuple(c.params) == (100.0, 100.0, 45.0, 45.0)
    assert got.shape == (90, 90) and (got == 0).sum() > 0 and (got == 255).sum() > 0


def case_spherical_image():
    """image/undistortion.cc:274-290: a spherical image keeps its model; max_image_size shrinks it with the resize kernel."""
    cam = R.Camera(R.EQUIRECTANGULAR, 200, 100, [200.0, 100.0])
    img = R.noise_image(200, 100, 3, 21)
    got, c = U.UndistortImage(_options(), img, cam)
    assert c.model_id == R.EQUIRECTANGULAR and np.array_equal(got, img)
    got, c = U.UndistortImage(_options(max_image_size=50), img, cam)
    assert c.model_id == R.EQUIRECTANGULAR and (c.width, c.height) == (50, 25) and tuple(c.params) == (50.0, 25.0)
    compare_under_parity_rule(got, R.resize(img, 50, 25), None, "spherical resize")


def case_batch_and_errors():
    cams = [strong(ba_camera(R.SIMPLE_RADIAL, 64, 48), 4.0), strong(ba_camera(R.OPENCV, 80, 60), 4.0),
            ba_camera(R.PINHOLE, 32, 24)]
    imgs = [R.noise_image(64, 48, 1, 1), R.noise_image(80, 60, 3, 2), R.noise_image(32, 24, 1, 3)]
    res = U.UndistortImages(_options(), imgs, cams)
    for (got, oc), img, cam in list(zip(res, imgs, cams))[:2]:
        compare_under_parity_rule(got, R.warp(cam, _ref_cam(oc), img), cam.model_id, "batch")
    # a PINHOLE camera warps onto itself: every source coordinate is an integer (all of the image would be eligible under
    # (b), so it is compared exactly instead); the last row and column have no x1 / y1 and are blank (bitmap.cc:343)
    got, oc = res[2]
    assert oc.model_id == U.PINHOLE and (oc.width, oc.height) == (32, 24) and np.array_equal(oc.params, cams[2].params)
    assert np.array_equal(got[:-1, :-1], imgs[2][:-1, :-1]) and not got[-1].any() and not got[:, -1].any()
    with pytest.raises(U.UndistortError, match="does not match"):
        U.UndistortImage(_options(), imgs[0], cams[1])
    with pytest.raises(U.UndistortError, match="blank_pixels"):
        U.UndistortImage(_options(blank_pixels=2.0), imgs[0], cams[0])
    with pytest.raises(U.UndistortError, match="gpu_index"):
        U.UndistortImage(_options(), imgs[0], cams[0], gpu_index=4096)


def case_mixed_route_batch():
    """One call whose images take every route in turn -- indirect, direct, resize, clone, indirect again -- through one
    set of grow-only device buffers: the last image reuses buffers that grew for the first, after smaller images. Every
    output and output camera is byte-equal to the single-image call for the same input."""
    lens = strong(ba_camera(R.OPENCV, 61, 47, (0.37, -0.21)), 4.0)
    cams = [lens, ba_camera(R.PINHOLE, 24, 20), R.Camera(R.EQUIRECTANGULAR, 40, 20, [40.0, 20.0]),
            R.Camera(R.EQUIRECTANGULAR, 16, 8, [16.0, 8.0]), lens]
    imgs = [R.noise_image(61, 47, 3, 31), R.noise_image(24, 20, 1, 32), R.noise_image(40, 20, 3, 33),
            R.noise_image(16, 8, 1, 34), R.noise_image(61, 47, 1, 35)]
    routes = ["indirect", "direct", "resize", "clone", "indirect"]
    opt = _options(max_image_size=20)
    res = U.UndistortImages(opt, imgs, cams)
    assert len(res) == 5
    for k, ((got, oc), img, cam, route) in enumerate(zip(res, imgs, cams, routes)):
        if cam.model_id == R.EQUIRECTANGULAR:
            same_size = (oc.width, oc.height) == (cam.width, cam.height)
            took = "clone" if same_size else "resize"
            assert oc.model_id == R.EQUIRECTANGULAR and (not same_size or np.array_equal(got, img))
        else:
            took = "direct" if R.should_warp_directly(cam, oc) else "indirect"
            assert oc.model_id == U.PINHOLE
        assert took == route, (k, took, route)
        alone, alone_cam = U.UndistortImage(opt, img, cam)
        assert (oc.model_id, oc.width, oc.height) == (alone_cam.model_id, alone_cam.width, alone_cam.height), k
        assert np.array_equal(oc.params, alone_cam.params), k
        assert got.shape == alone.shape and got.dtype == alone.dtype and np.array_equal(got, alone), k
        assert got.any(), k
    assert (res[1][1].width, res[1][1].height) == (20, 17)
    assert (res[2][1].width, res[2][1].height) == (20, 10)
    assert max(res[0][1].width, res[0][1].height) == 20 and res[0][0].shape[2] == 3 and res[4][0].ndim == 2


# ---- the GPU runs ----------------------------------------------------------------------------------------------------

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", WARP_CASES, ids=WARP_IDS)
def test_warp_parity(case):
    case_warp(*case)


@pytest.mark.parametrize("model", PERSPECTIVE_MODELS, ids=[U.W.CAMERA_MODELS[m][0] for m in PERSPECTIVE_MODELS])
def test_points_match_checker(model):
    case_points(model)


def test_points_spherical():
    case_points_spherical()


def test_resize_kernel_matches_restated_filter():
    case_resize()


def test_indirect_path_property():
    case_indirect_property()


def test_indirect_path_small_target():
    case_indirect_small_target()


def test_blank_pixels_known_answers():
    case_blank_pixels()


def test_spherical_image():
    case_spherical_image()


def test_batch_and_errors():
    case_batch_and_errors()


def test_mixed_route_batch():
    case_mixed_route_batch()


def test_full_size_warp_parity():
    """One image at a real size (1024x768 OPENCV, RGB): grid tails, row pitch padding and many workgroups."""
    cam = ba_camera(R.OPENCV, 1022, 767, (3.0, -2.0))
    img = R.noise_image(1022, 767, 3, 5)
    got, oc = U.UndistortImage(_options(blank_pixels=0.5), img, cam)
    compare_under_parity_rule(got, R.warp(cam, _ref_cam(oc), img), R.OPENCV, "full size OPENCV")
