"""`python -m colmap_amd image_undistorter` (reference exe/image.cc:325-430, controllers/undistorters.cc:150-313):
distorted images + sparse model in -> the dense workspace `patch_match_stereo` starts from. The copy-through and error
paths run without a GPU; the end-to-end run (undistort on the GPU, then PatchMatch on the result) is a GPU test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pm_common
import undistort_reference as R
from colmap_amd import image_undistorter as cli
from colmap_amd import mvs, scene
from colmap_amd import workspace as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_DIRS = ("images", "sparse", "stereo", "stereo/depth_maps", "stereo/normal_maps", "stereo/consistency_graphs")
LAYOUT_FILES = ("sparse/cameras.bin", "sparse/images.bin", "sparse/points3D.bin", "stereo/patch-match.cfg",
                "stereo/fusion.cfg", "run-colmap-photometric.sh", "run-colmap-geometric.sh")


def _pinhole_input(tmp_path, n=4, w=96, h=72):
    """A pinhole scene on disk: (images dir, sparse dir, names)."""
    views = pm_common.scene(n, w, h)
    ws = tmp_path / "pinhole"
    names = pm_common.write_dense_workspace(str(ws), views, num_points=300)
    return str(ws / "images"), str(ws / "sparse"), names, views


def _run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "colmap_amd", *args], capture_output=True, text=True, env=env, cwd=ROOT)


def _assert_layout(out):
    for d in LAYOUT_DIRS:
        assert os.path.isdir(os.path.join(out, d)), d
    for f in LAYOUT_FILES:
        assert os.path.isfile(os.path.join(out, f)), f


def _cfg_names(out):
    pm = open(os.path.join(out, "stereo", "patch-match.cfg")).read().splitlines()
    fu = open(os.path.join(out, "stereo", "fusion.cfg")).read().splitlines()
    return pm, fu


def test_copy_through_cli_without_a_gpu(tmp_path):
    """PINHOLE input, no max_image_size (controllers/undistorters.cc:251-260): files are copied byte for byte, the model
    is unchanged (image/undistortion.cc:316-322), nothing touches the GPU."""
    images, sparse, names, _ = _pinhole_input(tmp_path)
    out = str(tmp_path / "dense")
    assert cli.main(["--image_path", images, "--input_path", sparse, "--output_path", out,
                     "--num_patch_match_src_images", "7"]) == 0
    _assert_layout(out)
    for n in names:
        assert open(os.path.join(out, "images", n), "rb").read() == open(os.path.join(images, n), "rb").read()
    a, b = W.read_sparse_model(sparse), W.read_sparse_model(os.path.join(out, "sparse"))
    for cid in a.cameras:
        assert b.cameras[cid].model_id == a.cameras[cid].model_id and np.array_equal(b.cameras[cid].params, a.cameras[cid].params)
    for iid in a.images:
        assert np.array_equal(a.images[iid].xys, b.images[iid].xys)
    pm, fu = _cfg_names(out)
    assert pm[0::2] == names and set(pm[1::2]) == {"__auto__, 7"} and fu == names
    script = open(os.path.join(out, "run-colmap-geometric.sh")).read()
    assert "python -m colmap_amd patch_match_stereo" in script and "geom_consistency true" in script
    assert "python -m colmap_amd stereo_fusion" in script and "--input_type geometric" in script
    assert "geom_consistency false" in open(os.path.join(out, "run-colmap-photometric.sh")).read()


def test_unreadable_images_are_left_out_of_the_configs(tmp_path):
    """controllers/undistorters.cc:197-212, 262-266: a missing image is skipped; with soft links the rest are linked."""
    images, sparse, names, _ = _pinhole_input(tmp_path)
    partial = tmp_path / "partial"
    os.makedirs(partial)
    for n in names[1:]:
        os.link(os.path.join(images, n), partial / n)
    out = str(tmp_path / "dense")
    # the missing PINHOLE image falls through to the read and fails there: nothing reaches the GPU
    assert cli.main(["--image_path", str(partial), "--input_path", sparse, "--output_path", out,
                     "--copy_policy", "soft-link"]) == 0
    pm, fu = _cfg_names(out)
    assert pm[0::2] == names[1:] and fu == names[1:]
    assert os.path.islink(os.path.join(out, "images", names[1]))
    assert not os.path.exists(os.path.join(out, "images", names[0]))


def test_cli_error_paths(tmp_path, capsys):
    images, sparse, names, _ = _pinhole_input(tmp_path)
    out = str(tmp_path / "dense")
    base = ["--image_path", images, "--input_path", sparse, "--output_path", out]
    assert cli.main(["--image_path", str(tmp_path / "nope"), "--input_path", sparse, "--output_path", out]) == 1
    assert cli.main(["--image_path", images, "--input_path", str(tmp_path / "nope"), "--output_path", out]) == 1
    assert cli.main(base + ["--output_type", "PMVS"]) == 1
    assert cli.main(base + ["--output_type", "nonsense"]) == 1
    assert "Invalid `output_type` - supported values are {'COLMAP', 'PMVS', 'CMP-MVS'}." in capsys.readouterr().err
    assert cli.main(base + ["--copy_policy", "move"]) == 1
    from colmap_amd import undistortion as U
    with pytest.raises(U.UndistortError):
        cli.main(base + ["--num_patch_match_src_images", "0"])
    with pytest.raises(U.UndistortError):
        cli.main(base + ["--jpeg_quality", "101"])
    # the command table knows the command
    from colmap_amd import __main__ as entry
    assert entry.COMMANDS["image_undistorter"][0] == "colmap_amd.image_undistorter"


def _distorted_input(tmp_path, k=-0.12):
    """The pinhole scene seen through SIMPLE_RADIAL lenses: distorted images (the checker's inverse warp), distorted
    observations (the existing forward model of colmap_amd/scene.py), SIMPLE_RADIAL cameras."""
    from PIL import Image as PILImage
    images, sparse, names, views = _pinhole_input(tmp_path)
    sm = W.read_sparse_model(sparse)
    src = tmp_path / "distorted" / "images" / "sub"
    os.makedirs(src)
    originals = {}
    for iid, img in sm.images.items():
        cam = sm.cameras[img.camera_id]
        fx, fy, cx, cy = cam.params
        f = 0.5 * (fx + fy)
        pin = R.Camera(R.PINHOLE, cam.width, cam.height, [f, f, cx, cy])
        dist = R.Camera(R.SIMPLE_RADIAL, cam.width, cam.height, [f, cx, cy, k])
        grey = np.asarray(PILImage.open(os.path.join(images, img.name)))
        PILImage.fromarray(R.distort_image(pin, dist, grey)).save(src / img.name)
        originals[iid] = (img.xys.copy(), pin)
        uvw = np.concatenate([(img.xys - [cx, cy]) / f, np.ones((len(img.xys), 1))], 1)
        img.xys = scene.img_from_cam(R.SIMPLE_RADIAL, dist.params, uvw)
        img.name = "sub/" + img.name   # a per-image subdirectory (Reconstruction::CreateImageDirs)
        sm.cameras[img.camera_id] = W.SparseCamera(cam.camera_id, R.SIMPLE_RADIAL, cam.width, cam.height, dist.params)
    W.write_model_binary(sm, str(tmp_path / "distorted" / "sparse"))
    return str(tmp_path / "distorted" / "images"), str(tmp_path / "distorted" / "sparse"), sm, originals


@pytest.mark.gpu
def test_image_undistorter_cli_end_to_end(tmp_path):
    images, sparse, sm, originals = _distorted_input(tmp_path)
    out = str(tmp_path / "dense")
    r = _run_cli("image_undistorter", "--image_path", images, "--input_path", sparse, "--output_path", out,
                 "--num_patch_match_src_images", "3", "--gpu_index", "0")
    assert r.returncode == 0, r.stderr
    _assert_layout(out)
    names = [sm.images[i].name for i in sorted(sm.images)]
    for sub in ("images", "stereo/depth_maps", "stereo/normal_maps", "stereo/consistency_graphs"):
        assert os.path.isdir(os.path.join(out, sub, "sub"))
    pm, fu = _cfg_names(out)
    assert pm[0::2] == names and set(pm[1::2]) == {"__auto__, 3"} and fu == names
    assert sorted(os.listdir(os.path.join(out, "images", "sub"))) == sorted(os.path.basename(n) for n in names)
    # sparse/ is PINHOLE, the observations are back where the pinhole scene had them
    und = W.read_sparse_model(os.path.join(out, "sparse"))
    for iid, img in und.images.items():
        cam = und.cameras[img.camera_id]
        assert W.CAMERA_MODELS[cam.model_id][0] == "PINHOLE"
        xys0, pin = originals[iid]
        assert np.abs(img.xys - sm.images[iid].xys).max() > 0.05            # moved
        rays = (img.xys - cam.params[2:4]) / cam.params[0:2]
        rays0 = (xys0 - pin.params[2:4]) / pin.params[0:2]
        assert np.abs(rays - rays0).max() * cam.params[0] <= 1e-6           # ... to the same rays
        from PIL import Image as PILImage
        bmp = np.asarray(PILImage.open(os.path.join(out, "images", img.name)))
        assert bmp.shape == (cam.height, cam.width)
        # the image itself is the checker's warp of the distorted file
        dist = sm.cameras[img.camera_id]
        src = np.asarray(PILImage.open(os.path.join(images, img.name)))
        want = R.warp(R.Camera(dist.model_id, dist.width, dist.height, dist.params),
                      R.Camera(cam.model_id, cam.width, cam.height, cam.params), src)
        assert np.array_equal(bmp, want.image)                              # SIMPLE_RADIAL: no transcendental
    # ... and the workspace is what patch_match_stereo starts from, unchanged
    ws = W.Workspace(out)
    assert len(ws.GetModel().images) == len(names)
    r = _run_cli("patch_match_stereo", "--workspace_path", out, "--PatchMatchStereo.geom_consistency", "0",
                 "--PatchMatchStereo.num_iterations", "2", "--PatchMatchStereo.gpu_index", "0")
    assert r.returncode == 0, r.stderr
    for i, n in enumerate(names):
        depth = mvs.read_mat(os.path.join(out, "stereo", "depth_maps", n + ".photometric.bin"))
        assert depth.ndim >= 2 and (depth > 0).mean() > 0.2, (n, (depth > 0).mean())
        assert os.path.isfile(os.path.join(out, "stereo", "normal_maps", n + ".photometric.bin"))


@pytest.mark.gpu
def test_pipeline_undistort_images_cli_equivalent(tmp_path):
    """pipeline.undistort_images (the pycolmap signature) writes what the command writes, with max_image_size applied."""
    from colmap_amd import pipeline
    from colmap_amd import undistortion as U
    images, sparse, sm, _ = _distorted_input(tmp_path)
    out = str(tmp_path / "dense")
    ctl = pipeline.undistort_images(out, sparse, images, num_patch_match_src_images=2,
                                    undistort_options=U.UndistortCameraOptions(max_image_size=64))
    _assert_layout(out)
    assert len(ctl.image_names_) == len(sm.images)
    und = W.read_sparse_model(os.path.join(out, "sparse"))
    assert all(max(c.width, c.height) == 64 and c.model_id == U.PINHOLE for c in und.cameras.values())
