"""Image undistortion on MI355X: distorted images + sparse model -> the pinhole dense workspace PatchMatch and fusion
start from (include/colmap_amd_undistort.h, colmap_amd/csrc/undistort.hip).

Mirrors (reference file:line in each docstring):
  image/undistortion.{h,cc}            UndistortCameraOptions, UndistortCamera, UndistortImage, UndistortReconstruction
  image/undistortion.{h,cc}            RectifyStereoCameras, RectifyAndUndistortStereoImages
  image/warp.{h,cc}                    WarpImageOptions, WarpImageWithHomographyBetweenCameras
  controllers/undistorters.cc:150-313  COLMAPUndistorter
  controllers/undistorters.cc:633-710  StandaloneImageUndistorter
  controllers/undistorters.cc:712-820  StereoImageRectifier
The camera arithmetic and every pixel run behind the C ABI (UndistortCamera on the host, the rest on the GPU); this
module does the file side. There is no CPU fallback: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import workspace as W
from .camera import model as camera_model

EQUIRECTANGULAR = W.CAMERA_MODEL_IDS["EQUIRECTANGULAR"]
PINHOLE = W.CAMERA_MODEL_IDS["PINHOLE"]


class _Cam(C.Structure):  # undistort_cam
    _fields_ = [("model_id", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32),
                ("params", C.c_double * 16)]


class _Options(C.Structure):  # undistort_options
    _fields_ = [("blank_pixels", C.c_double), ("min_scale", C.c_double), ("max_scale", C.c_double),
                ("max_image_size", C.c_int32), ("interpolation", C.c_int32),
                ("roi_min_x", C.c_double), ("roi_min_y", C.c_double), ("roi_max_x", C.c_double), ("roi_max_y", C.c_double),
                ("max_cam_point_norm", C.c_double), ("direct_warp_min_scale", C.c_double)]


class _Image(C.Structure):  # undistort_image
    _fields_ = [("camera", _Cam), ("data", C.c_void_p), ("channels", C.c_int32), ("reserved", C.c_int32),
                ("out", C.c_void_p), ("out_capacity", C.c_size_t), ("out_camera", _Cam)]


class _StereoPair(C.Structure):  # undistort_stereo_pair
    _fields_ = [("image1", _Image), ("image2", _Image), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("Q", C.c_double * 16)]


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "undistort_images"):
        raise _lib.LibraryMissingError("the loaded library has no undistort_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    L.undistort_last_error.restype = C.c_char_p
    return L


class UndistortError(RuntimeError):
    pass


def _check(rc: int):
    if rc != 0:
        raise UndistortError(lib().undistort_last_error().decode())


@dataclass
class WarpImageOptions:
    """colmap::WarpImageOptions (image/warp.h)."""
    interpolation: str = "bilinear"       # "bilinear" | "nearest"
    direct_warp_min_scale: float = 0.5


@dataclass
class UndistortCameraOptions:
    """colmap::UndistortCameraOptions (image/undistortion.h:38-71)."""
    blank_pixels: float = 0.0
    min_scale: float = 0.2
    max_scale: float = 2.0
    max_image_size: int = -1
    roi_min_x: float = 0.0
    roi_min_y: float = 0.0
    roi_max_x: float = 1.0
    roi_max_y: float = 1.0
    max_cam_point_norm: float = -1.0
    warp_options: WarpImageOptions = field(default_factory=WarpImageOptions)


def _c_options(o: UndistortCameraOptions) -> _Options:
    interp = {"nearest": 0, "bilinear": 1}.get(str(o.warp_options.interpolation).lower())
    if interp is None:
        raise UndistortError(f"Invalid warp image interpolation mode: {o.warp_options.interpolation}")
    return _Options(o.blank_pixels, o.min_scale, o.max_scale, int(o.max_image_size), interp, o.roi_min_x, o.roi_min_y,
                    o.roi_max_x, o.roi_max_y, o.max_cam_point_norm, o.warp_options.direct_warp_min_scale)


def _c_cam(cam) -> _Cam:
    n = W.CAMERA_MODELS[cam.model_id][1]
    p = np.asarray(cam.params, np.float64)
    if p.shape != (n,):
        raise UndistortError(f"{W.CAMERA_MODELS[cam.model_id][0]} takes {n} parameters, got {p.shape}")
    c = _Cam(int(cam.model_id), int(cam.width), int(cam.height), 0)
    for i, v in enumerate(p):
        c.params[i] = float(v)
    return c


def _py_cam(c: _Cam, camera_id: int = 0) -> W.SparseCamera:
    n = W.CAMERA_MODELS[c.model_id][1]
    return W.SparseCamera(camera_id, c.model_id, c.width, c.height, np.array(c.params[:n], np.float64))


def IsSpherical(cam) -> bool:
    return cam.model_id == EQUIRECTANGULAR


def IsPerspective(cam) -> bool:
    return cam.model_id != EQUIRECTANGULAR


def IsUndistorted(cam) -> bool:
    """Camera::IsUndistorted (scene/camera.cc:98-111): spherical, or every extra parameter within 1e-8 of zero."""
    if IsSpherical(cam):
        return True
    m = camera_model(cam.model_id)
    if m is None:
        raise KeyError(cam.model_id)
    first_extra = len(m.focal_length_idxs) + len(m.principal_point_idxs)
    return not np.any(np.abs(np.asarray(cam.params, np.float64)[first_extra:]) > 1e-8)


def _rescale_to_max_image_size(options: UndistortCameraOptions, cam) -> W.SparseCamera:
    """RescaleToMaxImageSize (image/undistortion.cc:43-54) for a spherical camera: Camera::Rescale(scale)
    (scene/camera.cc:113-121), whose parameters (width, height) follow the image (sensor/models.h:399-405)."""
    out = W.SparseCamera(cam.camera_id, cam.model_id, cam.width, cam.height, np.array(cam.params, np.float64))
    if options.max_image_size < 0:
        return out
    scale = min(options.max_image_size / cam.width, options.max_image_size / cam.height)
    if scale < 1.0:
        w, h = int(np.floor(scale * cam.width + 0.5)), int(np.floor(scale * cam.height + 0.5))
        out.params = out.params * np.array([w / cam.width, h / cam.height])
        out.width, out.height = w, h
    return out


def UndistortCamera(options: UndistortCameraOptions, camera) -> W.SparseCamera:
    """UndistortCamera (image/undistortion.cc:58-264) on the host side of the library: callable without a GPU."""
    out = _Cam()
    opt, cam = _c_options(options), _c_cam(camera)
    _check(lib().undistort_camera(C.byref(opt), C.byref(cam), C.byref(out)))
    return _py_cam(out, getattr(camera, "camera_id", 0))


def CamFromImg(camera, xy: np.ndarray) -> np.ndarray:
    """Camera::CamFromImg for (N,2) pixels; NaN rows where the reference returns no value (host side of the library)."""
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    uv = np.empty_like(xy)
    cam = _c_cam(camera)
    _check(lib().undistort_cam_from_img(C.byref(cam), xy.ctypes.data_as(C.c_void_p), C.c_int64(len(xy)),
                                        uv.ctypes.data_as(C.c_void_p)))
    return uv


def _predicted_camera(options: UndistortCameraOptions, camera) -> W.SparseCamera:
    if IsSpherical(camera):
        return _rescale_to_max_image_size(options, camera)
    return UndistortCamera(options, camera)


def UndistortImages(options: UndistortCameraOptions, bitmaps: Sequence[np.ndarray], cameras: Sequence,
                    gpu_index: int = 0) -> List[Tuple[np.ndarray, W.SparseCamera]]:
    """UndistortImage (image/undistortion.cc:266-301) for a batch: bitmaps are (H,W) grey or (H,W,3) RGB uint8."""
    n = len(bitmaps)
    imgs = (_Image * max(n, 1))()
    keep, outs = [], []
    for i, (bmp, cam) in enumerate(zip(bitmaps, cameras)):
        bmp = np.ascontiguousarray(bmp, np.uint8)
        ch = 1 if bmp.ndim == 2 else bmp.shape[2]
        if bmp.shape[:2] != (cam.height, cam.width):  # THROW_CHECK_EQ (:271-272)
            raise UndistortError(f"bitmap {bmp.shape[1]}x{bmp.shape[0]} does not match its camera {cam.width}x{cam.height}")
        want = _predicted_camera(options, cam)
        out = np.empty((want.height, want.width) + (() if bmp.ndim == 2 else (ch,)), np.uint8)
        keep.append(bmp)
        outs.append(out)
        imgs[i].camera = _c_cam(cam)
        imgs[i].data = bmp.ctypes.data
        imgs[i].channels = ch
        imgs[i].out = out.ctypes.data
        imgs[i].out_capacity = out.nbytes
    opt = _c_options(options)
    _check(lib().undistort_images(C.byref(opt), C.c_int32(n), imgs, C.c_int32(gpu_index)))
    res = []
    for i in range(n):
        oc = _py_cam(imgs[i].out_camera, getattr(cameras[i], "camera_id", 0))
        assert (oc.height, oc.width) == outs[i].shape[:2]
        res.append((outs[i], oc))
    return res


def UndistortImage(options: UndistortCameraOptions, distorted_bitmap: np.ndarray, distorted_camera,
                   gpu_index: int = 0) -> Tuple[np.ndarray, W.SparseCamera]:
    """UndistortImage (image/undistortion.cc:266-301): (undistorted bitmap, undistorted camera)."""
    return UndistortImages(options, [distorted_bitmap], [distorted_camera], gpu_index)[0]


def _fill_image(slot: _Image, bmp: np.ndarray, cam, out: np.ndarray):
    slot.camera = _c_cam(cam)
    slot.data = bmp.ctypes.data
    slot.channels = 1 if bmp.ndim == 2 else bmp.shape[2]
    slot.out = out.ctypes.data
    slot.out_capacity = out.nbytes


def _checked_bitmap(bmp, cam) -> np.ndarray:
    bmp = np.ascontiguousarray(bmp, np.uint8)
    if bmp.shape[:2] != (cam.height, cam.width):  # THROW_CHECK_EQ (image/undistortion.cc:271-272, :457-460)
        raise UndistortError(f"bitmap {bmp.shape[1]}x{bmp.shape[0]} does not match its camera {cam.width}x{cam.height}")
    return bmp


def RectifyStereoCameras(camera1, camera2, R, t) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """RectifyStereoCameras (image/undistortion.cc:384-445) on the host side of the library: callable without a GPU.
    cam2_from_cam1 as a 3x3 rotation R and a translation t; -> (H1, H2, Q)."""
    R = np.ascontiguousarray(R, np.float64).reshape(3, 3)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    H1, H2, Q = np.empty((3, 3)), np.empty((3, 3)), np.empty((4, 4))
    c1, c2 = _c_cam(camera1), _c_cam(camera2)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib().undistort_rectify_cameras(C.byref(c1), C.byref(c2), vp(R), vp(t), vp(H1), vp(H2), vp(Q)))
    return H1, H2, Q


def RectifyAndUndistortStereoImagePairs(options: UndistortCameraOptions, pairs: Sequence, gpu_index: int = 0) -> List:
    """RectifyAndUndistortStereoImages for a batch in ONE undistort_rectify_images call: pairs holds
    (bitmap1, bitmap2, camera1, camera2, R, t); -> [(undistorted1, undistorted2, undistorted_camera, Q)]."""
    n = len(pairs)
    arr = (_StereoPair * max(n, 1))()
    keep = []
    for i, (b1, b2, cam1, cam2, R, t) in enumerate(pairs):
        b1, b2 = _checked_bitmap(b1, cam1), _checked_bitmap(b2, cam2)
        want = UndistortCamera(options, cam1)  # camera 1 only (:462)
        o1 = np.empty((want.height, want.width) + b1.shape[2:], np.uint8)
        o2 = np.empty((want.height, want.width) + b2.shape[2:], np.uint8)
        _fill_image(arr[i].image1, b1, cam1, o1)
        _fill_image(arr[i].image2, b2, cam2, o2)
        arr[i].R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
        arr[i].t[:] = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
        keep.append((b1, b2, o1, o2))
    opt = _c_options(options)
    _check(lib().undistort_rectify_images(C.byref(opt), C.c_int32(n), arr, C.c_int32(gpu_index)))
    res = []
    for i, (_, _, o1, o2) in enumerate(keep):
        oc = _py_cam(arr[i].image1.out_camera, getattr(pairs[i][2], "camera_id", 0))
        assert (oc.height, oc.width) == o1.shape[:2] == o2.shape[:2]
        res.append((o1, o2, oc, np.array(arr[i].Q[:], np.float64).reshape(4, 4)))
    return res


def RectifyAndUndistortStereoImages(options: UndistortCameraOptions, distorted_image1: np.ndarray,
                                    distorted_image2: np.ndarray, distorted_camera1, distorted_camera2, R, t,
                                    gpu_index: int = 0):
    """RectifyAndUndistortStereoImages (image/undistortion.cc:447-490) on the GPU:
    -> (undistorted_image1, undistorted_image2, undistorted_camera, Q). When ShouldWarpDirectly is false the warp runs at
    source size with the rescaled camera and the conjugated homography, then shrinks (include/colmap_amd_undistort.h)."""
    return RectifyAndUndistortStereoImagePairs(options, [(distorted_image1, distorted_image2, distorted_camera1,
                                                          distorted_camera2, R, t)], gpu_index)[0]


def WarpImageWithHomographyBetweenCameras(options: WarpImageOptions, Hinv, source_camera, target_camera,
                                          source_image: np.ndarray, gpu_index: int = 0) -> np.ndarray:
    """WarpImageWithHomographyBetweenCameras (image/warp.cc:196-272), direct path, on the GPU: target pixel p takes the
    source at ImgFromCam(source, CamFromImg(target, hnormalized(Hinv p))); 0 where the third coordinate is 0."""
    bmp = _checked_bitmap(source_image, source_camera)
    out = np.empty((target_camera.height, target_camera.width) + bmp.shape[2:], np.uint8)
    im = _Image()
    _fill_image(im, bmp, source_camera, out)
    opt = _c_options(UndistortCameraOptions(warp_options=options))
    H = np.ascontiguousarray(Hinv, np.float64).reshape(3, 3)
    tgt = _c_cam(target_camera)
    _check(lib().undistort_warp_homography(C.byref(opt), H.ctypes.data_as(C.c_void_p), C.byref(tgt), C.byref(im),
                                           C.c_int32(gpu_index)))
    return out


def UndistortPoints(distorted_camera, undistorted_camera, xy: np.ndarray, gpu_index: int = 0) -> np.ndarray:
    """The observation loop of UndistortReconstruction (image/undistortion.cc:334-381) for one camera, on the GPU."""
    out = np.array(xy, np.float64).reshape(-1, 2)
    out = np.ascontiguousarray(out)
    d, u = _c_cam(distorted_camera), _c_cam(undistorted_camera)
    _check(lib().undistort_points(C.byref(d), C.byref(u), out.ctypes.data_as(C.c_void_p), C.c_int64(len(out)),
                                  C.c_int32(gpu_index)))
    return out


def ResizeBitmap(bitmap: np.ndarray, width: int, height: int, gpu_index: int = 0) -> np.ndarray:
    """Bitmap::Rescale with the library's triangle filter (colmap_amd/csrc/undistort.hip), on the GPU."""
    bmp = np.ascontiguousarray(bitmap, np.uint8)
    ch = 1 if bmp.ndim == 2 else bmp.shape[2]
    out = np.empty((height, width) + (() if bmp.ndim == 2 else (ch,)), np.uint8)
    _check(lib().undistort_resize(bmp.ctypes.data_as(C.c_void_p), C.c_int32(bmp.shape[1]), C.c_int32(bmp.shape[0]),
                                  C.c_int32(ch), out.ctypes.data_as(C.c_void_p), C.c_int32(width), C.c_int32(height),
                                  C.c_int32(gpu_index)))
    return out


def LastTiming() -> Tuple[float, float]:
    """(kernel ms, whole-call ms) of the last UndistortImages."""
    k, t = C.c_double(), C.c_double()
    lib().undistort_last_timing(C.byref(k), C.byref(t))
    return k.value, t.value


def UndistortReconstruction(options: UndistortCameraOptions, model: W.SparseModel, gpu_index: int = 0) -> None:
    """UndistortReconstruction (image/undistortion.cc:303-382) on a workspace.SparseModel, in place: cameras become
    PINHOLE (spherical ones are only resized), every observation goes through undistort_points on the GPU."""
    def keep_unchanged(cam):  # :316-318
        return IsUndistorted(cam) and options.max_image_size < 0

    distorted = {cid: replace(c, params=np.array(c.params, np.float64)) for cid, c in model.cameras.items()}
    for cid, cam in distorted.items():
        if keep_unchanged(cam):
            continue
        new = _predicted_camera(options, cam)
        new.camera_id = cam.camera_id
        model.cameras[cid] = new
    # one launch per camera: the observations of all its images together
    by_cam: Dict[int, List[W.SparseImage]] = {}
    for img in model.images.values():
        if not keep_unchanged(distorted[img.camera_id]) and len(img.xys):
            by_cam.setdefault(img.camera_id, []).append(img)
    for cid, imgs in by_cam.items():
        xy = np.concatenate([np.asarray(i.xys, np.float64).reshape(-1, 2) for i in imgs], 0)
        xy = UndistortPoints(distorted[cid], model.cameras[cid], xy, gpu_index)
        at = 0
        for i in imgs:
            n = len(i.xys)
            i.xys = xy[at:at + n].copy()
            at += n


# ------------------------------------------------------------------------------------------------
# bitmaps (sensor/bitmap.cc) with PIL, like workspace.py
# ------------------------------------------------------------------------------------------------

def read_bitmap(path: str) -> Optional[np.ndarray]:
    """Bitmap::Read(path, as_rgb=true) (sensor/bitmap.cc): (H,W,3) uint8, or (H,W) for a grey file; None if unreadable."""
    from PIL import Image as PILImage
    try:
        with PILImage.open(path) as im:
            if im.mode in ("L", "1"):
                return np.ascontiguousarray(np.asarray(im.convert("L"), np.uint8))
            return np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))
    except Exception:
        return None


def write_bitmap(path: str, bitmap: np.ndarray, jpeg_quality: int = -1) -> bool:
    """Bitmap::Write with MaybeSetJpegQuality (controllers/undistorters.cc:41-52): the quality applies to .jpg / .jpeg."""
    from PIL import Image as PILImage
    kw = {}
    if jpeg_quality > 0 and os.path.splitext(path)[1].lower() in (".jpg", ".jpeg"):
        kw["quality"] = int(jpeg_quality)
    try:
        PILImage.fromarray(bitmap).save(path, **kw)
        return True
    except Exception:
        return False


def _file_copy(src: str, dst: str, copy_type: str):
    """FileCopy (util/file.cc): copy | hard-link | soft-link."""
    if os.path.lexists(dst):
        os.remove(dst)
    if copy_type == "copy":
        shutil.copyfile(src, dst)
    elif copy_type == "hard-link":
        os.link(src, dst)
    elif copy_type == "soft-link":
        os.symlink(os.path.abspath(src), dst)
    else:
        raise UndistortError(f"Invalid `copy_policy` - supported values are {{'copy', 'soft-link', 'hard-link'}}.")


@dataclass
class COLMAPUndistorterOptions:
    """COLMAPUndistorter::Options (controllers/undistorters.h)."""
    num_patch_match_src_images: int = 20
    copy_type: str = "copy"
    jpeg_quality: int = -1
    image_ids: List[int] = field(default_factory=list)
    gpu_index: int = 0
    batch_size: int = 8  # (MI355X) images handed to one undistort_images call


class COLMAPUndistorter:
    """COLMAPUndistorter (controllers/undistorters.cc:150-313): writes the dense workspace
    `<out>/{images,sparse,stereo/{depth_maps,normal_maps,consistency_graphs,patch-match.cfg,fusion.cfg}}` plus the two
    run-colmap-*.sh scripts."""

    def __init__(self, options: COLMAPUndistorterOptions, camera_options: UndistortCameraOptions, model: W.SparseModel,
                 image_path: str, output_path: str):
        if options.num_patch_match_src_images < 1:
            raise UndistortError("Check failed: options_.num_patch_match_src_images >= 1")
        if not -1 <= options.jpeg_quality <= 100:
            raise UndistortError("Check failed: jpeg_quality in [-1, 100]")
        self.options_, self.camera_options_, self.model_ = options, camera_options, model
        self.image_path_, self.output_path_ = image_path, output_path
        self.image_names_: List[str] = []

    def Run(self):
        out = self.output_path_
        stereo = ("depth_maps", "normal_maps", "consistency_graphs")
        for d in ("images", "sparse", "stereo") + tuple(os.path.join("stereo", s) for s in stereo):
            os.makedirs(os.path.join(out, d), exist_ok=True)
        ids = list(self.options_.image_ids) or sorted(self.model_.images)
        # Reconstruction::CreateImageDirs: the sub-folders of the image names
        for iid in ids:
            sub = os.path.dirname(self.model_.images[iid].name)
            if sub:
                for d in ("images",) + tuple(os.path.join("stereo", s) for s in stereo):
                    os.makedirs(os.path.join(out, d, sub), exist_ok=True)
        ok = self._undistort(ids)
        self.image_names_ = [self.model_.images[i].name for i in ids if ok[i]]
        import copy
        undistorted = copy.deepcopy(self.model_)
        UndistortReconstruction(self.camera_options_, undistorted, self.options_.gpu_index)
        W.write_model_binary(undistorted, os.path.join(out, "sparse"))
        W.write_patch_match_config(os.path.join(out, "stereo", "patch-match.cfg"), self.image_names_,
                                   f"__auto__, {self.options_.num_patch_match_src_images}")
        with open(os.path.join(out, "stereo", "fusion.cfg"), "w") as f:
            f.writelines(n + "\n" for n in self.image_names_)
        self._write_script(False)
        self._write_script(True)

    def _undistort(self, ids: Sequence[int]) -> Dict[int, bool]:
        """COLMAPUndistorter::Undistort (:230-280) per image; the images that go through the GPU are batched."""
        ok: Dict[int, bool] = {}
        batch: List[Tuple[int, np.ndarray]] = []

        def flush():
            if not batch:
                return
            cams = [self.model_.cameras[self.model_.images[i].camera_id] for i, _ in batch]
            res = UndistortImages(self.camera_options_, [b for _, b in batch], cams, self.options_.gpu_index)
            for (iid, _), (bmp, _) in zip(batch, res):
                dst = os.path.join(self.output_path_, "images", self.model_.images[iid].name)
                ok[iid] = write_bitmap(dst, bmp, self.options_.jpeg_quality)
            batch.clear()

        for iid in ids:
            img = self.model_.images[iid]
            cam = self.model_.cameras[img.camera_id]
            src = os.path.join(self.image_path_, img.name)
            dst = os.path.join(self.output_path_, "images", img.name)
            if (not IsPerspective(cam) or IsUndistorted(cam)) and self.camera_options_.max_image_size < 0 \
                    and os.path.isfile(src):  # :242-260
                _file_copy(src, dst, self.options_.copy_type)
                ok[iid] = True
                continue
            bmp = read_bitmap(src)
            if bmp is None:
                print(f"E Cannot read image at path: {src}")
                ok[iid] = False
                continue
            if bmp.shape[:2] != (cam.height, cam.width):
                raise UndistortError(f"image {img.name} is {bmp.shape[1]}x{bmp.shape[0]}, its camera {cam.width}x{cam.height}")
            batch.append((iid, bmp))
            if len(batch) >= self.options_.batch_size:
                flush()
        flush()
        return ok

    def _write_script(self, geometric: bool):
        """WriteScript / WriteCOLMAPCommands (:93-146, :304-313) with this package's commands; the meshers are not part of it."""
        name = "run-colmap-geometric.sh" if geometric else "run-colmap-photometric.sh"
        g = "true" if geometric else "false"
        with open(os.path.join(self.output_path_, name), "w") as f:
            f.write("# Run from this directory, with the colmap_amd package importable.\n")
            f.write("python -m colmap_amd patch_match_stereo \\\n  --workspace_path . \\\n  --workspace_format COLMAP \\\n"
                    f"  --PatchMatchStereo.max_image_size 2000 \\\n  --PatchMatchStereo.geom_consistency {g}\n")
            f.write("python -m colmap_amd stereo_fusion \\\n  --workspace_path . \\\n  --workspace_format COLMAP \\\n"
                    f"  --input_type {'geometric' if geometric else 'photometric'} \\\n  --output_path ./fused.ply\n")


@dataclass
class StereoImageRectifierOptions:
    """StereoImageRectifier::Options (controllers/undistorters.h)."""
    stereo_pairs: List[Tuple[int, int]] = field(default_factory=list)   # (image_id1, image_id2)
    jpeg_quality: int = -1
    gpu_index: int = 0
    batch_size: int = 4  # (MI355X) pairs handed to one undistort_rectify_images call


class StereoImageRectifier:
    """StereoImageRectifier (controllers/undistorters.cc:712-820): per pair a directory `<name1>-<name2>` (`/` in names
    replaced by `-`) with the two rectified, undistorted images and `Q.txt`."""

    def __init__(self, options: StereoImageRectifierOptions, camera_options: UndistortCameraOptions, model: W.SparseModel,
                 image_path: str, output_path: str):
        if not -1 <= options.jpeg_quality <= 100:
            raise UndistortError("Check failed: jpeg_quality in [-1, 100]")
        self.options_, self.camera_options_, self.model_ = options, camera_options, model
        self.image_path_, self.output_path_ = image_path, output_path
        self.pair_names_: List[str] = []   # the pairs written

    def Run(self):
        os.makedirs(self.output_path_, exist_ok=True)
        batch = []

        def flush():
            if not batch:
                return
            res = RectifyAndUndistortStereoImagePairs(self.camera_options_, [b[1] for b in batch], self.options_.gpu_index)
            for (names, _), (o1, o2, _, Q) in zip(batch, res):
                pair_name, n1, n2 = names
                write_bitmap(os.path.join(self.output_path_, pair_name, n1), o1, self.options_.jpeg_quality)
                write_bitmap(os.path.join(self.output_path_, pair_name, n2), o2, self.options_.jpeg_quality)
                with open(os.path.join(self.output_path_, pair_name, "Q.txt"), "w") as f:   # WriteMatrix
                    for row in Q:
                        f.write(" ".join(repr(float(v)) for v in row) + "\n")
                self.pair_names_.append(pair_name)
            batch.clear()

        for id1, id2 in self.options_.stereo_pairs:
            image1, image2 = self.model_.images[id1], self.model_.images[id2]
            cam1, cam2 = self.model_.cameras[image1.camera_id], self.model_.cameras[image2.camera_id]
            n1, n2 = image1.name.replace("/", "-"), image2.name.replace("/", "-")
            pair_name = f"{n1}-{n2}"
            os.makedirs(os.path.join(self.output_path_, pair_name), exist_ok=True)
            bitmaps = []
            for img in (image1, image2):
                src = os.path.join(self.image_path_, img.name)
                bmp = read_bitmap(src)
                if bmp is None:
                    print(f"E Cannot read image at path {src}")
                    break
                bitmaps.append(bmp)
            if len(bitmaps) != 2:
                continue
            # cam2_from_cam1 = image2.CamFromWorld() * Inverse(image1.CamFromWorld()) (:789-790)
            R1, R2 = image1.RotationMatrix(), image2.RotationMatrix()
            R = R2 @ R1.T
            t = np.asarray(image2.tvec, np.float64) - R @ np.asarray(image1.tvec, np.float64)
            batch.append(((pair_name, n1, n2), (bitmaps[0], bitmaps[1], cam1, cam2, R, t)))
            if len(batch) >= self.options_.batch_size:
                flush()
        flush()


@dataclass
class StandaloneImageUndistorterOptions:
    """StandaloneImageUndistorter::Options (controllers/undistorters.h)."""
    image_names_and_cameras: List[Tuple[str, W.SparseCamera]] = field(default_factory=list)
    copy_type: str = "copy"
    jpeg_quality: int = -1
    gpu_index: int = 0
    batch_size: int = 8  # (MI355X) images handed to one undistort_images call


class StandaloneImageUndistorter:
    """StandaloneImageUndistorter (controllers/undistorters.cc:633-710): undistorts images whose cameras come from a
    list, with no model on disk."""

    def __init__(self, options: StandaloneImageUndistorterOptions, camera_options: UndistortCameraOptions, image_path: str,
                 output_path: str):
        if not -1 <= options.jpeg_quality <= 100:
            raise UndistortError("Check failed: jpeg_quality in [-1, 100]")
        self.options_, self.camera_options_ = options, camera_options
        self.image_path_, self.output_path_ = image_path, output_path
        self.image_names_: List[str] = []   # the images written

    def Run(self):
        os.makedirs(self.output_path_, exist_ok=True)
        batch: List[Tuple[str, np.ndarray, W.SparseCamera]] = []

        def flush():
            if not batch:
                return
            res = UndistortImages(self.camera_options_, [b for _, b, _ in batch], [c for _, _, c in batch],
                                  self.options_.gpu_index)
            for (name, _, _), (bmp, _) in zip(batch, res):
                if write_bitmap(os.path.join(self.output_path_, name), bmp, self.options_.jpeg_quality):
                    self.image_names_.append(name)
            batch.clear()

        for name, cam in self.options_.image_names_and_cameras:
            src, dst = os.path.join(self.image_path_, name), os.path.join(self.output_path_, name)
            if os.path.dirname(name):
                os.makedirs(os.path.dirname(dst), exist_ok=True)
            if IsUndistorted(cam) and self.camera_options_.max_image_size < 0 and os.path.isfile(src):  # :684-690
                _file_copy(src, dst, self.options_.copy_type)
                self.image_names_.append(name)
                continue
            bmp = read_bitmap(src)
            if bmp is None:
                print(f"E Cannot read image at path {src}")
                continue
            if bmp.shape[:2] != (cam.height, cam.width):
                raise UndistortError(f"image {name} is {bmp.shape[1]}x{bmp.shape[0]}, its camera {cam.width}x{cam.height}")
            batch.append((name, bmp, cam))
            if len(batch) >= self.options_.batch_size:
                flush()
        flush()
