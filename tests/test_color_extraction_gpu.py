"""Colour extraction on the GPU (include/colmap_amd_color.h) against the numpy checker tests/color_reference.py.

Samples: `valid` is identical to the checker's; values agree within 2^-16, one float ulp below 256 -- a fused
multiply-add on the device may differ from numpy by that much and no more.
Colours: identical, except +-1 in a channel where the checker's double mean lies within 1e-4 of a half-integer (the
project's half_tol); the eligible channels are counted from the checker alone and capped at 1 %. Observation coordinates
have generic fractional parts (seeded uniform), for which the expected share is about 2e-4. The solid-colour cases allow
no exception."""
import os

import numpy as np
import pytest

import color_reference as CR
import undistort_reference as R
from colmap_amd import color_extraction as CE
from colmap_amd import workspace as W

SAMPLE_TOL = 2.0 ** -16
IMAGES = {1: (37, 29, 3), 2: (64, 48, 1), 3: (9, 7, 3)}     # id -> width, height, channels
LONG_IDS = list(range(10, 80))                               # 70 images of 9x7: one point is seen in each of them
LONG_POINT, BLANK_POINT = 1000, 1001


def image_name(iid):
    return f"img_{iid:03d}.png"


def make_model(seed=11):
    """-> (SparseModel, {image id: bitmap}). 40 points with tracks of length 1 to 3 over three images of different
    shapes, observations on and beyond the x1 >= W / y1 >= H border and at negative coordinates, one point without a
    valid sample, one point observed in each of 70 small images."""
    rng = np.random.default_rng(seed)
    bitmaps = {iid: R.noise_image(w, h, c, seed + iid) for iid, (w, h, c) in IMAGES.items()}
    sizes = dict(IMAGES)
    for iid in LONG_IDS:
        bitmaps[iid] = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
        sizes[iid] = (9, 7, 3)
    obs = {iid: [] for iid in sizes}   # image id -> [(x, y, point id)]
    points = {}
    for pid in range(1, 41):
        length = 1 + (pid % 3)
        for iid in rng.permutation(list(IMAGES))[:length]:
            w, h, _ = sizes[int(iid)]
            obs[int(iid)].append((rng.uniform(0.5, w - 0.5), rng.uniform(0.5, h - 0.5), pid))
        points[pid] = None
    # the border of InterpolateBilinear: x - 1/2 = W - 1 has x1 = W (invalid); just inside is valid; negative is invalid
    w, h, _ = sizes[1]
    for k, (x, y) in enumerate([(w - 0.5, 10.3), (w - 0.5 - 1e-9, 10.3), (12.7, h - 0.5), (12.7, h - 0.5 - 1e-9),
                                (-3.2, 5.1), (4.4, -0.75), (0.5, 0.5), (0.5 - 1e-9, 3.3), (w + 40.0, h + 40.0),
                                (float("nan"), 2.0)]):
        obs[1].append((x, y, 1 + k))   # further observations of points 1..10, in the same image
    for iid in (1, 2, 3):              # BLANK_POINT: observed three times, never inside
        w, h, _ = sizes[iid]
        obs[iid].append((w + 5.0, h / 2.0, BLANK_POINT))
    for iid in LONG_IDS:
        obs[iid].append((rng.uniform(0.5, 8.5), rng.uniform(0.5, 6.5), LONG_POINT))
    obs[2].append((10.25, 11.75, LONG_POINT))
    points[LONG_POINT] = points[BLANK_POINT] = None

    model = W.SparseModel()
    model.cameras[1] = W.SparseCamera(1, R.SIMPLE_PINHOLE, 64, 48, np.array([50.0, 32.0, 24.0]))
    for iid in sorted(sizes):
        rows = obs[iid]
        rng.shuffle(rows)
        xys = np.array([[r[0], r[1]] for r in rows] + [[1.5, 1.5]], np.float64)      # the last point2D has no 3D point
        ids = np.array([r[2] for r in rows] + [-1], np.int64)
        model.images[iid] = W.SparseImage(iid, np.array([1.0, 0, 0, 0]), np.zeros(3), 1, image_name(iid), xys, ids)
    for pid in points:
        track = [(iid, k) for iid in sorted(model.images) for k, q in enumerate(model.images[iid].point3D_ids) if q == pid]
        model.points3D[pid] = W.SparsePoint3D(pid, np.zeros(3), (7, 7, 7), 0.0, track)
    return model, bitmaps


def checker_layout(model):
    """The slot layout from the checker alone -> (point ids, ptr, {image id: (point2D indices, slots)})."""
    pids = sorted(model.points3D)
    index = {pid: k for k, pid in enumerate(pids)}
    op, oi, o2 = [], [], []
    for iid in sorted(model.images):
        for k, q in enumerate(model.images[iid].point3D_ids):
            if q != -1:
                op.append(index[int(q)])
                oi.append(iid)
                o2.append(k)
    ptr, slot = CR.slot_layout(op, oi, o2, len(pids))
    per_image, at = {}, 0
    for iid in sorted(model.images):
        n = int((np.asarray(model.images[iid].point3D_ids) != -1).sum())
        per_image[iid] = (np.array(o2[at:at + n], np.int64), slot[at:at + n])
        at += n
    return pids, ptr, per_image


_EXPECTED = {}


def expected(seed=11):
    """The checker's answer for make_model(seed), computed once and shared."""
    if seed not in _EXPECTED:
        model, bitmaps = make_model(seed)
        pids, ptr, per_image = checker_layout(model)
        rgb, valid = np.zeros((ptr[-1], 3), np.float32), np.zeros(ptr[-1], bool)
        for iid, (idx, slot) in per_image.items():
            rgb[slot], valid[slot] = CR.sample(bitmaps[iid], model.images[iid].xys[idx])
        colours, count, near_half = CR.point_colours(rgb, valid, ptr)
        _EXPECTED[seed] = dict(model=model, bitmaps=bitmaps, pids=pids, ptr=ptr, per_image=per_image, rgb=rgb, valid=valid,
                               colours=colours, count=count, near_half=near_half)
    return _EXPECTED[seed]


def run_device(e, order=None):
    """Streams the model's images through a handle in `order` -> (samples, valid, colours, count)."""
    with CE.ColorExtractor(int(e["ptr"][-1])) as ex:
        for iid in (order or sorted(e["per_image"])):
            idx, slot = e["per_image"][iid]
            ex.AddImage(e["bitmaps"][iid], e["model"].images[iid].xys[idx], slot)
        colours, count = ex.Finish(e["ptr"])
        rgb, valid = ex.Samples()
    return rgb, valid, colours, count


def case_layout_matches_checker():
    e = expected()
    slots = CE.ModelSlots(e["model"])
    assert list(slots.point_ids) == e["pids"] and np.array_equal(slots.ptr, e["ptr"])
    for iid, (idx, slot) in e["per_image"].items():
        assert np.array_equal(slots.per_image[iid][0], idx) and np.array_equal(slots.per_image[iid][1], slot)
    lengths = np.diff(e["ptr"])
    assert lengths.max() == 71 > 64 and (lengths <= 64).sum() == 41   # the long-range path and the serial path both run


def case_samples():
    e = expected()
    rgb, valid, _, _ = run_device(e)
    assert np.array_equal(valid, e["valid"])
    err = np.abs(rgb.astype(np.float64) - e["rgb"].astype(np.float64)).max()
    print(f"samples: {int(valid.sum())} valid of {len(valid)}, max |d| {err:.3e}")
    assert 0 < (~valid).sum() < len(valid)
    assert err <= SAMPLE_TOL
    assert not rgb[~valid].any()
    # the border cases of image 1, by construction: x - 1/2 == W - 1 is outside, a hair inside is inside
    img = e["model"].images[1]
    idx, slot = e["per_image"][1]
    by_xy = {(float(x), float(y)): bool(valid[s]) for (x, y), s in zip(img.xys[idx], slot) if not np.isnan(x)}
    assert by_xy[(36.5, 10.3)] is False and by_xy[(36.5 - 1e-9, 10.3)] is True
    assert by_xy[(12.7, 28.5)] is False and by_xy[(12.7, 28.5 - 1e-9)] is True
    assert by_xy[(-3.2, 5.1)] is False and by_xy[(4.4, -0.75)] is False and by_xy[(0.5, 0.5)] is True


def compare_colours(colours, count, e):
    assert np.array_equal(count, e["count"])
    d = np.abs(colours.astype(np.int32) - e["colours"].astype(np.int32))
    share = e["near_half"].mean()
    print(f"colours: {len(colours)} points, differing channels {int((d > 0).sum())}, eligible {int(e['near_half'].sum())} "
          f"= {share:.2e}")
    assert share <= 0.01
    assert d.max() <= 1
    assert not ((d > 0) & ~e["near_half"]).any()


def case_colours():
    e = expected()
    _, _, colours, count = run_device(e)
    compare_colours(colours, count, e)
    k = e["pids"].index(BLANK_POINT)
    assert count[k] == 0 and tuple(colours[k]) == (0, 0, 0)
    k = e["pids"].index(LONG_POINT)
    assert count[k] == 71
    assert (count > 0).sum() == 41


def case_determinism():
    e = expected()
    a = run_device(e)
    b = run_device(e)
    c = run_device(e, order=sorted(e["per_image"], reverse=True))   # the order of the images does not matter either
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def case_all_images_on_a_model(tmp_path):
    e = expected()
    import copy
    from PIL import Image as PILImage
    model = copy.deepcopy(e["model"])
    for iid, bmp in e["bitmaps"].items():
        PILImage.fromarray(bmp).save(tmp_path / image_name(iid))
    assert CE.ExtractColorsForAllImages(model, str(tmp_path)) == len(model.images)
    colours = np.array([model.points3D[pid].rgb for pid in e["pids"]], np.uint8)
    compare_colours(colours, e["count"], e)
    assert model.points3D[BLANK_POINT].rgb == (0, 0, 0)   # was (7, 7, 7): every point of the model is rewritten


def solid_model(colours_by_image, num_points=10, size=(16, 12)):
    """Images 1..n, every point observed at a pixel centre of every image, two point2Ds without a 3D point per image."""
    w, h = size
    model = W.SparseModel()
    model.cameras[1] = W.SparseCamera(1, R.SIMPLE_PINHOLE, w, h, np.array([20.0, w / 2.0, h / 2.0]))
    bitmaps = {}
    for iid, colour in colours_by_image.items():
        bitmaps[iid] = np.broadcast_to(np.array(colour, np.uint8), (h, w, 3)).copy()
        xys = np.array([[1.5 + (p % 12), 1.5 + (p // 12) + (iid % 3)] for p in range(num_points)] + [[3.0, 3.0], [5.0, 5.0]])
        ids = np.array(list(range(1, num_points + 1)) + [-1, -1], np.int64)
        model.images[iid] = W.SparseImage(iid, np.array([1.0, 0, 0, 0]), np.zeros(3), 1, image_name(iid), xys, ids)
    for pid in range(1, num_points + 1):
        model.points3D[pid] = W.SparsePoint3D(pid, np.zeros(3), (0, 0, 0), 0.0, [(iid, pid - 1) for iid in colours_by_image])
    return model, bitmaps


def write_images(bitmaps, path):
    from PIL import Image as PILImage
    os.makedirs(path, exist_ok=True)
    for iid, bmp in bitmaps.items():
        PILImage.fromarray(bmp).save(os.path.join(path, image_name(iid)))


def case_reference_known_answer(tmp_path):
    """reconstruction_test.cc:1418-1444: solid (20, 40, 220), one file deleted, every point exactly that colour."""
    model, bitmaps = solid_model({1: (20, 40, 220), 2: (20, 40, 220), 3: (20, 40, 220)})
    write_images(bitmaps, str(tmp_path))
    os.remove(tmp_path / image_name(1))
    assert CE.ExtractColorsForAllImages(model, str(tmp_path)) == 2
    assert all(p.rgb == (20, 40, 220) for p in model.points3D.values())


def case_half_rounds_away_from_zero(tmp_path):
    model, bitmaps = solid_model({1: (21, 40, 220), 2: (20, 41, 221)})
    write_images(bitmaps, str(tmp_path))
    CE.ExtractColorsForAllImages(model, str(tmp_path))
    assert all(p.rgb == (21, 41, 221) for p in model.points3D.values())   # means 20.5, 40.5, 220.5


def case_for_image(tmp_path):
    model, bitmaps = solid_model({1: (10, 20, 30), 2: (40, 50, 60)}, num_points=4)
    # a second observation of point 1 in image 1, on a different colour: it must not overwrite the first
    bitmaps[1][8:, :] = (200, 100, 50)
    img = model.images[1]
    img.xys = np.concatenate([img.xys, [[4.5, 10.5]]])
    img.point3D_ids = np.concatenate([img.point3D_ids, [1]])
    write_images(bitmaps, str(tmp_path))
    model.points3D[2].rgb = (1, 2, 3)   # not black: stays
    assert CE.ExtractColorsForImage(model, 1, str(tmp_path)) is True
    assert model.points3D[1].rgb == (10, 20, 30) and model.points3D[2].rgb == (1, 2, 3)
    assert model.points3D[3].rgb == model.points3D[4].rgb == (10, 20, 30)
    assert CE.ExtractColorsForImage(model, 2, str(tmp_path)) is True    # nothing is black any more
    assert [model.points3D[p].rgb for p in (1, 2, 3, 4)] == [(10, 20, 30), (1, 2, 3), (10, 20, 30), (10, 20, 30)]
    os.remove(tmp_path / image_name(2))
    assert CE.ExtractColorsForImage(model, 2, str(tmp_path)) is False
    # a fractional sample goes through Cast<uint8_t>: halfway between the two colours of image 1 -> round(105.0) etc.
    model.points3D[1].rgb = (0, 0, 0)
    img.xys[0] = [4.5, 8.0]   # rows 7 and 8 in equal parts
    assert CE.ExtractColorsForImage(model, 1, str(tmp_path)) is True
    assert model.points3D[1].rgb == (105, 60, 40)


def case_command(tmp_path):
    from colmap_amd import color_extractor
    model, bitmaps = solid_model({1: (21, 40, 220), 2: (20, 41, 221)})
    write_images(bitmaps, str(tmp_path / "images"))
    os.makedirs(tmp_path / "in")
    W.write_model_binary(model, str(tmp_path / "in"))
    assert color_extractor.main(["--image_path", str(tmp_path / "images"), "--input_path", str(tmp_path / "in"),
                                 "--output_path", str(tmp_path / "out")]) == 0
    back = W.read_sparse_model(str(tmp_path / "out"))
    assert sorted(back.points3D) == sorted(model.points3D)
    assert all(tuple(int(c) for c in p.rgb) == (21, 41, 221) for p in back.points3D.values())
    assert all(np.array_equal(back.images[i].xys, model.images[i].xys) for i in model.images)


def case_errors():
    """Every error is an argument the host refuses before a launch; a refused call stores nothing."""
    bmp = np.full((6, 8, 3), 90, np.uint8)
    xy = np.array([[2.5, 2.5], [3.5, 3.5]])
    with CE.ColorExtractor(3) as ex:
        with pytest.raises(CE.ColorError, match="slot 3 out of range"):
            ex.AddImage(bmp, xy, [0, 3])
        with pytest.raises(CE.ColorError, match="slot 1 given twice"):
            ex.AddImage(bmp, xy, [1, 1])
        ex.AddImage(bmp, xy, [0, 1])        # the refused calls took nothing
        with pytest.raises(CE.ColorError, match="slot 0 given twice"):
            ex.AddImage(bmp, xy[:1], [0])
        with pytest.raises(CE.ColorError, match="channels"):
            ex.AddImage(np.zeros((6, 8, 2), np.uint8), xy[:1], [2])
        with pytest.raises(CE.ColorError, match="ptr decreases at point 1"):
            ex.Finish([0, 2, 1, 3])
        with pytest.raises(CE.ColorError, match="beyond the 3 slots"):
            ex.Finish([0, 2, 4])
        colours, count = ex.Finish([0, 2, 3])
        assert colours.tolist() == [[90, 90, 90], [0, 0, 0]] and count.tolist() == [2, 0]
    with pytest.raises(CE.ColorError, match="gpu_index"):
        CE.ColorExtractor(3, gpu_index=4096)


# ---- the GPU runs ----------------------------------------------------------------------------------------------------

pytestmark = pytest.mark.gpu


def test_model_slots_match_checker_layout():
    case_layout_matches_checker()


def test_samples_match_checker():
    case_samples()


def test_colours_match_checker():
    case_colours()


def test_two_runs_are_byte_identical():
    case_determinism()


def test_extract_colors_for_all_images(tmp_path):
    case_all_images_on_a_model(tmp_path)


def test_reference_known_answer(tmp_path):
    case_reference_known_answer(tmp_path)


def test_half_rounds_away_from_zero(tmp_path):
    case_half_rounds_away_from_zero(tmp_path)


def test_extract_colors_for_image(tmp_path):
    case_for_image(tmp_path)


def test_color_extractor_command(tmp_path):
    case_command(tmp_path)


def test_errors():
    case_errors()
