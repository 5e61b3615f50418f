"""`python -m colmap_amd feature_extractor` without a GPU: the command table entry, the refusals by name, the database
additions, the image list, the camera a new image gets and the scale-back of keypoints."""
import contextlib
import importlib
import io
import os

import numpy as np
import pytest

from colmap_amd import __main__ as M
from colmap_amd import database as DB
from colmap_amd import feature_extraction as FE
from colmap_amd import feature_extractor as FX


def main(argv):
    err = io.StringIO()
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        rc = M.main(argv)
    return rc, err.getvalue()


def test_command_table_entry():
    assert M.COMMANDS["feature_extractor"][0] == "colmap_amd.feature_extractor"
    assert callable(importlib.import_module(M.COMMANDS["feature_extractor"][0]).main)
    rc, err = main(["feature_importer", "--database_path", "x"])
    assert rc == 1 and "feature_importer" in err and "not built" in err


REFUSALS = [
    (["--SiftExtraction.estimate_affine_shape", "1"], "estimate_affine_shape"),
    (["--SiftExtraction.domain_size_pooling", "1"], "domain_size_pooling"),
    (["--SiftExtraction.force_covariant_extractor", "1"], "force_covariant_extractor"),
    (["--SiftExtraction.darkness_adaptivity", "1"], "darkness_adaptivity"),
    (["--FeatureExtraction.type", "ALIKED_N16ROT"], "ALIKED"),
    (["--FeatureExtraction.use_gpu", "0"], "use_gpu"),
    (["--ImageReader.mask_path", "masks"], "mask_path"),
    (["--ImageReader.camera_mask_path", "mask.png"], "camera_mask_path"),
    (["--ImageReader.single_camera_per_folder", "1"], "single_camera_per_folder"),
    (["--ImageReader.single_camera_per_image", "1"], "single_camera_per_image"),
    (["--ImageReader.existing_camera_id", "3"], "existing_camera_id"),
    (["--ImageReader.camera_model", "NO_SUCH_MODEL"], "NO_SUCH_MODEL"),
    (["--descriptor_normalization", "l3"], "descriptor_normalization"),
    (["--FeatureExtraction.max_image_size", "0"], "max_image_size"),
]


@pytest.mark.parametrize("extra,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals_name_what_is_missing(tmp_path, extra, word):
    db = str(tmp_path / "database.db")
    rc, err = main(["feature_extractor", "--database_path", db, "--image_path", str(tmp_path)] + extra)
    assert rc == 1 and err.startswith("E ") and word in err
    assert not os.path.exists(db)   # refused before anything is written


def test_parser_defaults_and_options():
    a = FX.build_parser().parse_args(["--database_path", "d", "--image_path", "i"])
    assert FX.refusal(a) == ""
    o = FX.sift_options(a)
    assert o == FE.SiftExtractionOptions()
    assert a.camera_model == "SIMPLE_RADIAL" and not a.single_camera and a.default_focal_length_factor == 1.2
    a = FX.build_parser().parse_args(["--database_path", "d", "--image_path", "i", "--SiftExtraction.max_num_features", "100",
                                      "--SiftExtraction.first_octave", "0", "--SiftExtraction.upright", "1",
                                      "--descriptor_normalization", "L2", "--SiftExtraction.peak_threshold", "0.01"])
    o = FX.sift_options(a)
    assert (o.max_num_features, o.first_octave, o.upright, o.normalization, o.peak_threshold) == (100, 0, True, FE.L2, 0.01)


def test_database_additions(tmp_path):
    path = str(tmp_path / "database.db")
    kp = np.arange(18, dtype=np.float32).reshape(3, 6)
    with DB.Database(path, create=True) as db:
        cid = db.write_camera(2, 640, 480, [768.0, 320.0, 240.0, 0.0])
        cid2 = db.write_camera(1, 64, 48, [70.0, 71.0, 32.0, 24.0], prior_focal_length=True)
        iid = db.write_image("a.png", cid)
        assert not db.exists_keypoints(iid) and not db.exists_descriptors(iid)
        db.write_keypoints(iid, kp)
        db.write_descriptors(iid, np.zeros((3, 128), np.uint8))
        assert db.exists_keypoints(iid) and db.exists_descriptors(iid)
        with pytest.raises(DB.DatabaseError):
            db.write_keypoints(iid + 1, np.zeros((2, 5), np.float32))
    with DB.Database(path) as db:
        assert np.array_equal(db.read_keypoints(iid), kp)
        cams = db.read_cameras()
        assert cams[cid]["model"] == 2 and cams[cid]["params"].tolist() == [768.0, 320.0, 240.0, 0.0] and not cams[cid]["prior_focal_length"]
        assert cams[cid2]["prior_focal_length"] and (cams[cid2]["width"], cams[cid2]["height"]) == (64, 48)
        assert db.read_image_camera_ids() == {iid: cid}


def test_image_list_and_new_camera(tmp_path):
    (tmp_path / "sub").mkdir()
    for n in ("b.png", "a.JPG", "sub/c.tif", "notes.txt"):
        (tmp_path / n).write_bytes(b"")
    assert FX.list_images(str(tmp_path)) == ["a.JPG", "b.png", "sub/c.tif"]
    lst = tmp_path / "list.txt"
    lst.write_text("b.png\n\n# comment\nsub/c.tif\n")
    assert FX.list_images(str(tmp_path), str(lst)) == ["b.png", "sub/c.tif"]
    assert FX.new_camera_params(2, 640, 480, 1.2 * 640).tolist() == [768.0, 320.0, 240.0, 0.0]        # SIMPLE_RADIAL
    assert FX.new_camera_params(1, 101, 51, 100.0).tolist() == [100.0, 100.0, 50.5, 25.5]              # PINHOLE
    assert FX.new_camera_params(4, 10, 20, 5.0).tolist() == [5.0, 5.0, 5.0, 10.0, 0.0, 0.0, 0.0, 0.0]  # OPENCV


def test_scale_keypoints_and_thumbnail():
    kp = np.array([[10.0, 20.0, 1.0, -2.0, 2.0, 1.0]], np.float32)
    assert FX.scale_keypoints(kp, 80, 60, 80, 60) is kp
    out = FX.scale_keypoints(kp, 80, 60, 160, 180)   # ScaleKeypoints: x, a11, a21 by 2; y, a12, a22 by 3
    assert out.tolist() == [[20.0, 60.0, 2.0, -6.0, 4.0, 3.0]]
    with pytest.raises(ValueError):
        FE.rescale_keypoints(kp, 0.0, 1.0)
    img = np.zeros((120, 160), np.uint8)
    assert FX.thumbnail(img, 160) is img and FX.thumbnail(img, 80).shape == (60, 80) and FX.thumbnail(img.T, 80).shape == (80, 60)


def test_keypoints_to_affine():
    kp4 = np.array([[1.5, 2.5, 2.0, 0.0], [3.0, 4.0, 1.5, np.pi / 2]], np.float32)
    a = FE.keypoints_to_affine(kp4)
    assert a.dtype == np.float32 and a.shape == (2, 6)
    assert a[0].tolist() == [1.5, 2.5, 2.0, -0.0, 0.0, 2.0]
    assert abs(a[1, 2]) < 1e-6 and a[1, 4] == np.float32(1.5) and a[1, 3] == -a[1, 4] and a[1, 5] == a[1, 2]
    assert FE.keypoints_to_affine(np.zeros((0, 4), np.float32)).shape == (0, 6)


def test_missing_image_path_is_an_error(tmp_path):
    rc, err = main(["feature_extractor", "--database_path", str(tmp_path / "d.db"), "--image_path", str(tmp_path / "nowhere")])
    assert rc == 1 and "nowhere" in err
