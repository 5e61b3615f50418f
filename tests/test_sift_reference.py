"""Condition 1 of SIFT extraction: the numpy checker (tests/sift_reference.py) against what VLFeat itself gave for the
cases (tests/golden/sift_vlfeat.npz, made as tests/golden/sift_vlfeat.md says): the same detections in the same order, and
x, y, s, sigma, the angles, the float descriptors and the final keypoints and bytes equal bit for bit -- no field needed
a bound. Then: the cases contain what they are meant to test."""
import numpy as np
import pytest

import sift_cases as SC
import sift_reference as R
from test_sift_extraction_gpu import checker, same

CASES = SC.case_names()


def test_fixture_holds_every_case():
    assert set(CASES) == set(SC.make_cases())
    for name, made in SC.make_cases().items():
        assert SC.fixture()[name]["options"] == made["options"]
        have = SC.fixture()[name]["image"]
        assert have.shape == made["image"].shape and have.dtype == made["image"].dtype == np.uint8
        # the generator is the record of how the committed images were made: it may differ from them by one grey level
        # (numpy's exp in the last bit, then the quantisation), not by more
        assert np.abs(have.astype(np.int32) - made["image"].astype(np.int32)).max() <= 1, name
    assert SC.fixture()["blobs96"]["bounds"] == {}   # every field is equal bit for bit: no bound is stored


@pytest.mark.parametrize("name", CASES)
def test_checker_equals_vlfeat(name):
    want, got = SC.fixture()[name], checker(name)
    assert len(got["octaves"]) == len(want["octaves"])
    for k, (a, b) in enumerate(zip(got["octaves"], want["octaves"])):
        assert (a["o"], a["w"], a["h"]) == (b["o"], b["w"], b["h"])
        same(a["det_i"], b["det_i"], f"{name}: octave {k} detections (o, ix, iy, is)")
        same(a["det_f"], b["det_f"], f"{name}: octave {k} detections (x, y, s, sigma)")
        same(a["counts"], b["counts"], f"{name}: octave {k} orientation counts")
        same(a["angles"], b["angles"], f"{name}: octave {k} angles")
        same(a["float_desc"], b["float_desc"], f"{name}: octave {k} float descriptors")
    for key in ("level_num_features", "level_num_rows", "keypoints", "descriptors"):
        same(got[key], want[key], f"{name}: {key}")
    assert (got["skip"], got["num_out"]) == (want["skip"], want["num_out"])


def _stats(name):
    total = {}
    for oc in checker(name)["octaves"]:
        for k, v in oc["stats"].items():
            total[k] = total.get(k, 0) + v
    return total


def test_cases_contain_what_they_test():
    det = lambda name: [len(oc["det_i"]) for oc in checker(name)["octaves"]]
    counts = lambda name: np.concatenate([oc["counts"] for oc in checker(name)["octaves"]])
    assert det("blobs160")[:3] == [38, 73, 16] and det("odd67")[:3] == [9, 20, 1] and sum(det("constant")) == 0
    # one, two, three and four orientations: the cut to max_num_orientations is exercised, and so is the stop at four
    assert {1, 2, 3} <= set(counts("blobs160").tolist()) and 4 in counts("seam")
    assert (counts("upright") == 1).all() and (checker("upright")["keypoints"][:, 3] == 0).all()
    assert len(checker("one_orientation")["keypoints"]) == sum(det("one_orientation")) < len(checker("blobs96")["keypoints"])
    # every refinement test rejects somewhere, and candidates move
    total = {}
    for name in ("blobs160", "first0", "res2"):
        for k, v in _stats(name).items():
            total[k] = total.get(k, 0) + v
    for k in ("moved", "rejected_peak", "rejected_edge", "rejected_offset", "rejected_xy_range", "rejected_s_range"):
        assert total[k] > 0, k
    assert det("coarse")[3] > 0 and det("coarse")[0] == 0          # detections in the last octave
    assert det("first0")[0] > 0 and checker("first0")["octaves"][0]["o"] == 0
    assert checker("res2")["octaves"][0]["levels"].shape[0] == 5
    # the cut falls between levels and keeps the level that crosses the limit whole
    c = checker("cut")
    assert 0 < c["skip"] and c["num_out"] > 25 and c["skip"] + c["num_out"] == len(c["keypoints"])
    # border: detections within 8 octave pixels of an edge, so that windows are cut and gradients one-sided
    b = checker("border")["octaves"][0]
    edge = np.minimum(np.minimum(b["det_i"][:, 1], b["w"] - 1 - b["det_i"][:, 1]), np.minimum(b["det_i"][:, 2], b["h"] - 1 - b["det_i"][:, 2]))
    assert (edge <= 8).any()
    # seam: a detection within 2 pixels of the corner (64, 32) of four column-pass tiles of octave -1
    s = checker("seam")["octaves"][0]["det_i"]
    assert ((np.abs(s[:, 1] - 64) <= 2) & (np.abs(s[:, 2] - 32) <= 2)).any()
    # sizes: octave -1 of odd67 is 134 x 90, a multiple of none of 64, 32, 128, 8; blobs160 spans several tiles each way
    o = checker("odd67")["octaves"][0]
    assert all(o["w"] % t and o["h"] % t for t in (64, 32, 128, 8))
    assert checker("blobs160")["octaves"][0]["w"] > 2 * 128 and checker("blobs160")["octaves"][0]["h"] > 2 * 32
    # L2 and L1_ROOT differ in the bytes and agree in everything before
    same(checker("l2")["float_desc"], checker("blobs96")["float_desc"], "float descriptors under L2")
    assert not np.array_equal(checker("l2")["descriptors"], checker("blobs96")["descriptors"])


def test_pointwise_restatements():
    """The approximations against what they approximate, over their domains."""
    x = np.float32(10.0) ** np.linspace(-6, 6, 2001).astype(np.float32)
    assert np.max(np.abs(R.fast_sqrt_f(x) / np.sqrt(x) - 1)) < 1e-5
    a = np.linspace(-np.pi, np.pi, 4001)
    got = R.fast_atan2_f(np.sin(a).astype(np.float32), np.cos(a).astype(np.float32))
    assert np.max(np.abs(np.angle(np.exp(1j * (got - a))))) < 0.0062   # mathop.h: maximum error 0.0061 rad
    t = np.linspace(0, 25, 3001)
    assert np.max(np.abs(R.fast_expn(t) - np.exp(-t))) < 2e-3
    assert R.fast_expn(np.array([25.1]))[0] == 0.0
    assert R.floor_to_int(np.array([-1.5, -1.0, -0.0, 0.5, 2.0], np.float32)).tolist() == [-2, -1, 0, 0, 2]
    assert R.mod_2pi_f(np.array([-0.1, 7.0], np.float32)).tolist() == [np.float32(-0.1) + np.float32(2 * np.pi), np.float32(7.0) - np.float32(2 * np.pi)]
