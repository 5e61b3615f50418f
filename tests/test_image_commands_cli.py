"""The command lines of image_rectifier, image_undistorter_standalone and color_extractor without a GPU: registration,
the argument checks, the two list-file parsers, and the loud failure without a device."""
import os

import numpy as np
import pytest

import test_color_extraction_gpu as TC
import test_rectify_gpu as TR
import undistort_reference as R
from colmap_amd import __main__ as M
from colmap_amd import color_extractor, image_rectifier, image_undistorter_standalone, pipeline
from colmap_amd import workspace as W

NEW_COMMANDS = ("image_rectifier", "image_undistorter_standalone", "color_extractor")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from colmap_amd import build
    build.build()


def test_commands_are_registered():
    import importlib
    for name in NEW_COMMANDS:
        assert name in M.COMMANDS
        assert callable(importlib.import_module(M.COMMANDS[name][0]).main)
    for name in ("rectify_images", "undistort_images_standalone", "extract_colors"):
        assert callable(getattr(pipeline, name))


def _args(command, tmp_path, **override):
    base = {"image_rectifier": dict(image_path=tmp_path, input_path=tmp_path, output_path=tmp_path / "out",
                                    stereo_pairs_list=tmp_path / "pairs.txt"),
            "image_undistorter_standalone": dict(image_path=tmp_path, input_file=tmp_path / "cameras.txt",
                                                 output_path=tmp_path / "out"),
            "color_extractor": dict(image_path=tmp_path, input_path=tmp_path, output_path=tmp_path / "out")}[command]
    base.update(override)
    return [command] + [s for k, v in base.items() for s in (f"--{k}", str(v))]


@pytest.mark.parametrize("command", NEW_COMMANDS)
def test_bad_image_path_exits_1(command, tmp_path, capsys):
    (tmp_path / "pairs.txt").write_text("")
    (tmp_path / "cameras.txt").write_text("")
    assert M.main(_args(command, tmp_path, image_path=tmp_path / "nowhere")) == 1
    assert "`image_path` is not a directory" in capsys.readouterr().err


@pytest.mark.parametrize("command", ("image_rectifier", "color_extractor"))
def test_bad_input_path_exits_1(command, tmp_path, capsys):
    (tmp_path / "pairs.txt").write_text("")
    assert M.main(_args(command, tmp_path, input_path=tmp_path / "nowhere")) == 1
    assert "`input_path` is not a directory" in capsys.readouterr().err


def test_standalone_bad_input_file_exits_1(tmp_path, capsys):
    assert M.main(_args("image_undistorter_standalone", tmp_path)) == 1
    assert "`input_file` is not a file" in capsys.readouterr().err


def test_standalone_parser_accepts_the_documented_format():
    lines = ["a.jpg SIMPLE_RADIAL 640 480 500.5 320 240 0.1\n", "\n", "   \n",
             "  sub/b.png   PINHOLE 100 80 90 91 50 40  \n", "c.png OPENCV_FISHEYE 64 48 50 51 32 24 1e-2 -2e-3 0 0"]
    out = image_undistorter_standalone.parse_image_names_and_cameras(lines)
    assert [n for n, _ in out] == ["a.jpg", "sub/b.png", "c.png"]
    a, b, c = (cam for _, cam in out)
    assert (a.model_id, a.width, a.height) == (R.SIMPLE_RADIAL, 640, 480) and a.params.tolist() == [500.5, 320, 240, 0.1]
    assert (b.model_id, b.width, b.height) == (R.PINHOLE, 100, 80) and b.params.tolist() == [90, 91, 50, 40]
    assert c.model_id == R.OPENCV_FISHEYE and c.params.tolist() == [50, 51, 32, 24, 0.01, -0.002, 0, 0]
    assert a.params.dtype == np.float64


def test_standalone_parser_refusals(tmp_path, capsys):
    P = image_undistorter_standalone.parse_image_names_and_cameras
    with pytest.raises(image_undistorter_standalone.UnknownCameraModel, match="Camera model NOT_A_MODEL does not exist"):
        P(["a.jpg NOT_A_MODEL 640 480 1 2 3"])
    with pytest.raises(ValueError, match=r"VerifyParams\(\).*SIMPLE_RADIAL takes 4 parameters, got 3"):
        P(["a.jpg SIMPLE_RADIAL 640 480 500 320 240"])
    with pytest.raises(ValueError, match=r"VerifyParams\(\).*PINHOLE takes 4 parameters, got 5"):
        P(["a.jpg PINHOLE 640 480 500 500 320 240 0"])
    with pytest.raises(ValueError, match="expected `image_name CAMERA_MODEL width height"):
        P(["a.jpg PINHOLE 640"])
    with pytest.raises(ValueError, match="are numbers"):
        P(["a.jpg PINHOLE wide 480 1 1 1 1"])
    # through the command: an unknown model exits 1 with the reference's message
    (tmp_path / "cameras.txt").write_text("a.jpg NOT_A_MODEL 640 480 1 2 3\n")
    assert M.main(_args("image_undistorter_standalone", tmp_path)) == 1
    assert "Camera model NOT_A_MODEL does not exist" in capsys.readouterr().err
    (tmp_path / "cameras.txt").write_text("a.jpg RADIAL 640 480 1 2 3\n")
    assert M.main(_args("image_undistorter_standalone", tmp_path)) == 1
    assert "VerifyParams" in capsys.readouterr().err
    (tmp_path / "cameras.txt").write_text("")
    assert M.main(_args("image_undistorter_standalone", tmp_path, copy_policy="move")) == 1
    assert "Invalid `copy_policy`" in capsys.readouterr().err


def test_rectifier_pair_list(tmp_path, capsys):
    model, image_dir, _ = TR.two_image_model(tmp_path)
    lst = tmp_path / "pairs.txt"
    lst.write_text("left/a.png right/b.png\n\nright/b.png left/a.png\n")
    assert image_rectifier.read_stereo_image_pairs(str(lst), model) == [(1, 2), (2, 1)]
    lst.write_text("left/a.png nowhere.png\n")
    with pytest.raises(ValueError, match="image nowhere.png does not exist in the reconstruction"):
        image_rectifier.read_stereo_image_pairs(str(lst), model)
    for bad in ("left/a.png\n", "left/a.png right/b.png left/a.png\n"):
        lst.write_text(bad)
        with pytest.raises(ValueError, match=r"names.size\(\) == 2"):
            image_rectifier.read_stereo_image_pairs(str(lst), model)
    # through the command
    os.makedirs(tmp_path / "sparse")
    W.write_model_binary(model, str(tmp_path / "sparse"))
    lst.write_text("left/a.png nowhere.png\n")
    assert M.main(_args("image_rectifier", tmp_path, image_path=image_dir, input_path=tmp_path / "sparse")) == 1
    assert "nowhere.png does not exist" in capsys.readouterr().err


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")


def test_rectifier_without_a_device_fails_loudly(tmp_path, capsys):
    _no_gpu()
    model, image_dir, _ = TR.two_image_model(tmp_path)
    os.makedirs(tmp_path / "sparse")
    W.write_model_binary(model, str(tmp_path / "sparse"))
    (tmp_path / "pairs.txt").write_text("left/a.png right/b.png\n")
    assert M.main(_args("image_rectifier", tmp_path, image_path=image_dir, input_path=tmp_path / "sparse")) == 1
    assert "no HIP device available" in capsys.readouterr().err


def test_standalone_without_a_device_fails_loudly(tmp_path, capsys):
    _no_gpu()
    model, image_dir, _ = TR.two_image_model(tmp_path)
    cam = model.cameras[1]
    (tmp_path / "cameras.txt").write_text(f"left/a.png OPENCV {cam.width} {cam.height} " +
                                          " ".join(repr(float(p)) for p in cam.params) + "\n")
    assert M.main(_args("image_undistorter_standalone", tmp_path, image_path=image_dir)) == 1
    assert "no HIP device available" in capsys.readouterr().err


def test_color_extractor_without_a_device_fails_loudly(tmp_path, capsys):
    _no_gpu()
    model, bitmaps = TC.solid_model({1: (20, 40, 220), 2: (20, 40, 220)})
    TC.write_images(bitmaps, str(tmp_path / "images"))
    os.makedirs(tmp_path / "sparse")
    W.write_model_binary(model, str(tmp_path / "sparse"))
    assert M.main(_args("color_extractor", tmp_path, image_path=tmp_path / "images", input_path=tmp_path / "sparse")) == 1
    assert "no HIP device available" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
