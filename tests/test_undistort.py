"""Image undistortion without a GPU: the host side of the hipcc-built library (undistort_camera, undistort_cam_from_img)
against the known answers of the reference's own tests (image/undistortion_test.cc:78-262, 361-468), the inverse camera
models against the existing, independent forward models of colmap_amd/scene.py, and the error paths."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_undistort_gpu as G
import undistort_reference as R
from colmap_amd import scene
from colmap_amd import undistortion as U
from colmap_amd import workspace as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from colmap_amd import build
    build.build()


def _cam(model, f, w, h):
    """Camera::CreateFromModelId (scene/camera.cc): InitializeParams(focal_length, width, height)."""
    n = W.CAMERA_MODELS[model][1]
    p = np.zeros(n)
    if model == R.EQUIRECTANGULAR:
        p[:] = [w, h]
    elif model in R.ONE_FOCAL:
        p[:3] = [f, w / 2.0, h / 2.0]
    else:
        p[:4] = [f, f, w / 2.0, h / 2.0]
    return W.SparseCamera(1, model, w, h, p)


def test_abi_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colmap_amd_undistort.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(undistort_[a-z0-9_]+)\s*\(", text)))
    assert len(names) >= 6 and {"undistort_options_init", "undistort_camera", "undistort_images", "undistort_points",
                                "undistort_last_error"} <= set(names)
    from colmap_amd import build
    lib = ctypes.CDLL(build.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_options_defaults_match_reference():
    """undistort_options_init == the member initialisers (image/undistortion.h:38-71, image/warp.h)."""
    o = U._Options()
    U.lib().undistort_options_init(ctypes.byref(o))
    d = U.UndistortCameraOptions()
    for name in ("blank_pixels", "min_scale", "max_scale", "max_image_size", "roi_min_x", "roi_min_y", "roi_max_x",
                 "roi_max_y", "max_cam_point_norm"):
        assert getattr(o, name) == getattr(d, name), name
    assert (o.blank_pixels, o.min_scale, o.max_scale, o.max_image_size) == (0.0, 0.2, 2.0, -1)
    assert (o.roi_min_x, o.roi_min_y, o.roi_max_x, o.roi_max_y, o.max_cam_point_norm) == (0.0, 0.0, 1.0, 1.0, -1.0)
    assert o.interpolation == 1 and o.direct_warp_min_scale == d.warp_options.direct_warp_min_scale == 0.5


def test_undistort_camera_nominal():
    """image/undistortion_test.cc:78-142."""
    opt = U.UndistortCameraOptions()
    for model in (R.SIMPLE_PINHOLE, R.SIMPLE_RADIAL):
        u = U.UndistortCamera(opt, _cam(model, 1, 1, 1))
        assert W.CAMERA_MODELS[u.model_id][0] == "PINHOLE"
        assert (u.params[0], u.params[1], u.width, u.height) == (1, 1, 1, 1)
    cam = _cam(R.SIMPLE_RADIAL, 100, 100, 100)
    cam.params[3] = 0.5
    u = U.UndistortCamera(opt, cam)
    assert W.CAMERA_MODELS[u.model_id][0] == "PINHOLE"
    assert (u.params[0], u.params[1], u.params[2], u.params[3], u.width, u.height) == (100, 100, 42.0, 42.0, 84, 84)
    opt.blank_pixels = 1
    u = U.UndistortCamera(opt, cam)
    assert (u.params[0], u.params[1], u.width, u.height) == (100, 100, 90, 90)
    assert (u.params[2], u.params[3]) == (45.0, 45.0)
    opt.max_scale = 0.75
    u = U.UndistortCamera(opt, cam)
    assert (u.params[0], u.params[1], u.width, u.height) == (100, 100, 75, 75)
    opt.max_scale = 1.0
    opt.roi_min_x, opt.roi_min_y, opt.roi_max_x, opt.roi_max_y = 0.1, 0.2, 0.9, 0.8
    u = U.UndistortCamera(opt, cam)
    assert W.CAMERA_MODELS[u.model_id][0] == "PINHOLE"
    assert (u.params[0], u.params[1], u.width, u.height) == (100, 100, 80, 60)
    assert (u.params[2], u.params[3]) == (40, 30)


def test_undistort_camera_max_cam_point_norm():
    """image/undistortion_test.cc:144-179."""
    cam = _cam(R.SIMPLE_FISHEYE, 130, 200, 100)
    cam.params[1], cam.params[2] = 10, 50
    opt = U.UndistortCameraOptions(blank_pixels=1.0)
    unbounded = U.UndistortCamera(opt, cam)
    assert unbounded.width == cam.width * opt.max_scale and unbounded.height == cam.height * opt.max_scale
    opt.max_cam_point_norm = 2.0
    bounded = U.UndistortCamera(opt, cam)
    assert bounded.width < unbounded.width and bounded.height < unbounded.height
    opt.max_cam_point_norm = 0
    with pytest.raises(U.UndistortError, match="max_cam_point_norm != 0"):
        U.UndistortCamera(opt, cam)


def test_undistorted_pinhole_with_max_image_size():
    """image/undistortion_test.cc:361-407."""
    u = U.UndistortCamera(U.UndistortCameraOptions(max_image_size=50), _cam(R.PINHOLE, 100, 100, 100))
    assert W.CAMERA_MODELS[u.model_id][0] == "PINHOLE" and (u.width, u.height) == (50, 50)
    np.testing.assert_allclose(u.params, [50, 50, 25, 25], atol=1e-6, rtol=0)


def test_spherical_camera_is_resized_not_undistorted():
    """image/undistortion_test.cc:419-468."""
    cam = _cam(R.EQUIRECTANGULAR, 0.0, 500, 250)
    assert U.IsSpherical(cam) and U.IsUndistorted(cam) and not U.IsPerspective(cam)
    u = U._predicted_camera(U.UndistortCameraOptions(max_image_size=250), cam)
    assert W.CAMERA_MODELS[u.model_id][0] == "EQUIRECTANGULAR" and (u.width, u.height) == (250, 125)
    assert tuple(u.params) == (250.0, 125.0)
    with pytest.raises(U.UndistortError, match="IsPerspective"):   # image/undistortion.cc:76
        U.UndistortCamera(U.UndistortCameraOptions(), cam)


@pytest.mark.parametrize("kw,what", [
    (dict(blank_pixels=-0.1), "blank_pixels >= 0"), (dict(blank_pixels=1.1), "blank_pixels <= 1"),
    (dict(min_scale=0.0), "min_scale > 0"), (dict(min_scale=3.0), "min_scale <= options.max_scale"),
    (dict(max_image_size=0), "max_image_size != 0"),
    (dict(roi_min_x=-0.1), "roi_min_x >= 0"), (dict(roi_min_y=-0.1), "roi_min_y >= 0"),
    (dict(roi_max_x=1.1), "roi_max_x <= 1"), (dict(roi_max_y=1.1), "roi_max_y <= 1"),
    (dict(roi_min_x=0.6, roi_max_x=0.5), "roi_min_x < options.roi_max_x"),
    (dict(roi_min_y=0.6, roi_max_y=0.6), "roi_min_y < options.roi_max_y")])
def test_every_reference_option_check_raises(kw, what):
    """image/undistortion.cc:60-70."""
    cam = _cam(R.SIMPLE_RADIAL, 100, 100, 100)
    with pytest.raises(U.UndistortError, match=re.escape(what)):
        U.UndistortCamera(U.UndistortCameraOptions(**kw), cam)


def test_is_undistorted():
    """scene/camera.cc:98-111."""
    assert U.IsUndistorted(_cam(R.PINHOLE, 100, 10, 10)) and U.IsUndistorted(_cam(R.OPENCV, 100, 10, 10))
    cam = _cam(R.OPENCV, 100, 10, 10)
    cam.params[6] = 2e-8
    assert not U.IsUndistorted(cam)
    cam.params[6] = 1e-9
    assert U.IsUndistorted(cam)


@pytest.mark.parametrize("model", G.PERSPECTIVE_MODELS, ids=[W.CAMERA_MODELS[m][0] for m in G.PERSPECTIVE_MODELS])
def test_cam_from_img_inverts_the_existing_forward_model(model):
    """ImgFromCam(CamFromImg(p)) == p within 1e-6 px, the reference's own tolerance for this round trip
    (sensor/models_test.cc:101-102), with the forward model of colmap_amd/scene.py (independent of the new header)."""
    cam = G.ba_camera(model)
    xs, ys = np.meshgrid(np.linspace(0.5, cam.width - 0.5, 33), np.linspace(0.5, cam.height - 0.5, 25))
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    uv = U.CamFromImg(cam, xy)
    assert not np.isnan(uv).any()
    back = scene.img_from_cam(model, cam.params, np.concatenate([uv, np.ones((len(uv), 1))], 1))
    err = np.abs(back - xy).max()
    print(f"{W.CAMERA_MODELS[model][0]}: round trip max |d| {err:.3e} px")
    assert err <= 1e-6
    # and the numpy checker inverts to the same rays
    np.testing.assert_allclose(R.cam_from_img(cam, xy), uv, atol=1e-6 / cam.params[0], rtol=0)


def test_cam_from_img_has_no_value_where_the_reference_has_none():
    cam = G.ba_camera(R.EUCM)   # sensor/models.h:2815-2826
    xy = np.array([[512.0, 384.0], [-4000.0, 384.0], [6000.0, 6000.0]])
    uv = U.CamFromImg(cam, xy)
    assert not np.isnan(uv[0]).any() and np.isnan(uv[1:]).all()
    assert np.array_equal(np.isnan(uv), np.isnan(R.cam_from_img(cam, xy)))
    sph = _cam(R.EQUIRECTANGULAR, 0.0, 1000, 500)   # back hemisphere (sensor/models.h:2896-2898)
    uv = U.CamFromImg(sph, np.array([[600.0, 200.0], [100.0, 400.0]]))
    assert not np.isnan(uv[0]).any() and np.isnan(uv[1]).all()


def test_no_gpu_fails_loudly():
    """Without a HIP device the pixel paths fail with an error; there is no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam = G.ba_camera(R.SIMPLE_RADIAL, 64, 48)
    with pytest.raises(U.UndistortError, match="no HIP device available"):
        U.UndistortImage(U.UndistortCameraOptions(), np.zeros((48, 64), np.uint8), cam)
    with pytest.raises(U.UndistortError, match="no HIP device available"):
        U.UndistortPoints(cam, U.UndistortCamera(U.UndistortCameraOptions(), cam), np.zeros((3, 2)))
    with pytest.raises(U.UndistortError, match="no HIP device available"):
        U.ResizeBitmap(np.zeros((48, 64), np.uint8), 32, 24)


def test_checker_eligibility_share_is_small():
    """The exception of the parity rule is rare by construction: counted from the checker alone on every warp case."""
    for (model, kind, ch, interp, shift, over) in G.WARP_CASES:
        cam = G.strong(G.ba_camera(model, G.W0, G.H0, shift), 4.0)
        opt = G._options(interp, **over)
        und = U.UndistortCamera(opt, cam)
        res = R.warp(cam, G._ref_cam(und), G.make_image(kind, G.W0, G.H0, ch, 3), interp)
        assert res.may_differ.mean() <= 0.01, (model, kind, res.may_differ.mean())
        assert (res.image != 0).mean() > 0.5
