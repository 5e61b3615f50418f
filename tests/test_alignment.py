"""Host side of model alignment (colmap_amd/alignment.py and the commands model_comparer, model_aligner,
model_transformer) without a GPU: known answers of the stopping rule, Sim3d files, ComputeImageAlignmentError and the
association step by hand, and the three commands end to end with the CPU build of the unmodified kernels standing in for
the library (tests/test_alignment_emul.py)."""
import importlib
import os

import numpy as np
import pytest

import align_reference as A
import test_alignment_emul as E
import test_alignment_gpu as G
from colmap_amd import __main__ as cli_main
from colmap_amd import alignment as AL
from colmap_amd import bundle_adjuster as BA
from colmap_amd import fusion, scene
from colmap_amd import workspace as W

COMMANDS = ("model_comparer", "model_aligner", "model_transformer")


def test_commands_are_registered():
    for name in COMMANDS:
        assert name in cli_main.COMMANDS
        assert callable(importlib.import_module(cli_main.COMMANDS[name][0]).main)


def test_compute_num_trials_known_answers():
    """optim/ransac.h:179-210, the values tests/cpp/test_align_plan.cc asserts of the product's ComputeNumTrials."""
    assert A.compute_num_trials(50, 100, 1.0, 3.0) == A.SIZE_MAX   # prob_failure <= 0
    assert A.compute_num_trials(100, 100, 0.99, 3.0) == 1          # prob_outlier <= 0
    assert A.compute_num_trials(0, 100, 0.99, 3.0) == A.SIZE_MAX   # prob_outlier == 1
    assert A.compute_num_trials(2, 100, 0.99, 3.0) == A.SIZE_MAX   # num_inliers - 2 = 0
    assert A.compute_num_trials(50, 100, 0.99, 0.0) == 0
    # 50 of 100: p = 50/100 * 49/99 * 48/98 = 4/33; log(0.01) / log(29/33) = 35.64...; times 3, rounded up
    assert A.compute_num_trials(50, 100, 0.99, 3.0) == 107
    assert A.compute_num_trials(90, 100, 0.99, 1.0) == 4
    assert A.compute_num_trials(20000, 100000, 0.99, 3.0) == 1721  # the constructor's clamp for min_inlier_ratio = 0.2


def test_sim3d_file_round_trip(tmp_path):
    sim = AL.Sim3d(1.0 / 3.0, np.array([0.9, 0.1, -0.2, 0.3]) / np.linalg.norm([0.9, 0.1, -0.2, 0.3]), np.array([np.pi, -1e-17, 2e300]))
    path = str(tmp_path / "sim.txt")
    sim.ToFile(path)
    text = open(path).read()
    assert text.endswith("\n") and len(text.split()) == 8 and text.split()[0] == "0.33333333333333331"  # 17 digits
    back = AL.Sim3d.FromFile(path)
    assert np.array_equal(back.params(), sim.params())
    sane = AL.Sim3d(sim.scale, sim.rotation, np.array([np.pi, -2.5, 7.0]))
    inv = AL.Inverse(sane)
    assert inv.scale == 3.0 and np.allclose(AL.Inverse(inv).params(), sane.params(), rtol=0, atol=1e-14)
    x = np.array([0.3, -0.7, 1.1])
    assert np.allclose(AL.Inverse(AL.Sim3d.from_params(G.TRUE_SIM)) * (AL.Sim3d.from_params(G.TRUE_SIM) * x), x, atol=1e-15)
    with open(path, "w") as f:
        f.write("1 2 3\n")
    with pytest.raises(AL.AlignmentError):
        AL.Sim3d.FromFile(path)


def _one_image(pose):
    rec = scene.Reconstruction()
    rec.cameras[1] = scene.Camera(1, scene.PINHOLE, 640, 480, np.array([500.0, 500.0, 320.0, 240.0]))
    rec.images[2] = scene.Image(2, 1, np.asarray(pose, np.float64))
    return rec


def test_image_alignment_error_by_hand():
    # identity similarity; the tgt camera is turned by 90 degrees about z and its centre -R^T t sits at (3, 4, 0)
    a = _one_image([0, 0, 0, 1, 0, 0, 0])
    b = _one_image([0, 0, np.sqrt(0.5), np.sqrt(0.5), -4, 3, 0])
    (e,) = AL.ComputeImageAlignmentError(a, b, AL.Sim3d())
    assert e.image_name == 2 and abs(e.rotation_error_deg - 90.0) < 1e-12 and abs(e.proj_center_error - 5.0) < 1e-14
    # scale 2 and a shift: the src centre (1, 0, 0) lands on 2 * (1, 0, 0) + (0, 0, 1) = (2, 0, 1); tgt centre at the origin
    a = _one_image([0, 0, 0, 1, -1, 0, 0])
    b = _one_image([0, 0, 0, 1, 0, 0, 0])
    (e,) = AL.ComputeImageAlignmentError(a, b, AL.Sim3d(2.0, np.array([1.0, 0, 0, 0]), np.array([0.0, 0.0, 1.0])))
    assert e.rotation_error_deg == 0.0 and abs(e.proj_center_error - np.sqrt(5.0)) < 1e-15
    # names decide which images are common
    assert AL.ComputeImageAlignmentError(a, b, AL.Sim3d(), {2: "a.png"}, {2: "b.png"}) == []
    (e,) = AL.ComputeImageAlignmentError(a, b, AL.Sim3d(), {2: "a.png"}, {2: "a.png"})
    assert e.image_name == "a.png"
    # against the checker on the search pair
    src, tgt = G.search_pair()
    got = AL.ComputeImageAlignmentError(src, tgt, AL.Sim3d.from_params(G.TRUE_SIM))
    want = A.image_alignment_errors(src, tgt, G.TRUE_SIM)
    assert np.allclose([(e.rotation_error_deg, e.proj_center_error) for e in got], want, rtol=0, atol=1e-9)


def test_point_association_by_hand():
    """alignment.cc:411-447: the count of a tgt point starts at 0."""
    def model(assign):
        rec = scene.Reconstruction()
        for i in (1, 2, 3, 4):
            rec.images[i] = scene.Image(i, 1, np.array([0, 0, 0, 1, 0, 0, 0.0]), [scene.Point2D(np.zeros(2), -1) for _ in range(2)])
        for pid, (xyz, track) in assign.items():
            rec.points3D[pid] = scene.Point3D(np.array(xyz, np.float64), list(track))
            for (i, k) in track:
                rec.images[i].points2D[k].point3D_id = pid
        return rec
    src = model({10: ([1, 0, 0], [(1, 0), (2, 0), (3, 0), (4, 0)]), 11: ([2, 0, 0], [(1, 1), (2, 1)]), 12: ([3, 0, 0], [(3, 1)])})
    # tgt: point 20 under three of the four observations of src 10, point 21 under the fourth; 22 under both of src 11
    tgt = model({20: ([0, 1, 0], [(1, 0), (2, 0), (3, 0)]), 21: ([0, 2, 0], [(4, 0)]), 22: ([0, 3, 0], [(1, 1), (2, 1)])})
    a, b = AL.associate_points(src, tgt, 1)
    assert a.tolist() == [[1, 0, 0], [2, 0, 0]] and b.tolist() == [[0, 1, 0], [0, 3, 0]]  # counts 2 and 1; src 12 has none
    a, b = AL.associate_points(src, tgt, 2)
    assert a.tolist() == [[1, 0, 0]] and b.tolist() == [[0, 1, 0]]                        # three votes count 2
    a, b = AL.associate_points(src, tgt, 3)
    assert len(a) == 0 and a.shape == (0, 3)
    del tgt.images[4]                                                                      # an image tgt does not hold
    assert len(AL.associate_points(src, tgt, 2)[0]) == 1


# ----------------------------------------------------------------------------------------------------------------------
# the commands, through the stand-in library
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def emulated_library(monkeypatch):
    if not E.have_host_compiler():
        pytest.skip("the stand-in is built with ROCm's clang++ as host compiler")
    monkeypatch.setattr(AL, "lib", E.emul_lib)


def _write(rec, path, names=None):
    os.makedirs(path, exist_ok=True)
    W.write_model_binary(BA.sparse_model_from_reconstruction(rec, names), path)
    return path


def _run(command, *args):
    return importlib.import_module(cli_main.COMMANDS[command][0]).main([str(a) for a in args])


def _centres(path):
    sm = W.read_sparse_model(path)
    rec = BA.reconstruction_from_sparse_model(sm)
    return {sm.images[i].name: rec.ProjectionCenter(i) for i in sorted(rec.images)}, sm


def test_model_comparer_end_to_end(emulated_library, tmp_path, capsys):
    src, tgt = G.search_pair()
    p1, p2, out = _write(src, str(tmp_path / "m1")), _write(tgt, str(tmp_path / "m2")), tmp_path / "out"
    assert _run("model_comparer", "--input_path1", p1, "--input_path2", p2, "--output_path", out) == 1  # no directory
    out.mkdir()
    for mode in ("reprojection", "proj_center"):
        assert _run("model_comparer", "--input_path1", p1, "--input_path2", p2, "--output_path", out, "--alignment_error", mode,
                    "--max_proj_center_error", 0.05) == 0
        from colmap_amd import model_comparer
        errors = model_comparer.read_comparison_errors_csv(str(out / "errors.csv"))
        assert errors.shape == (len(G.SEARCH_COUNTS), 2)
        good = np.array([i + 1 not in G.SEARCH_OUTLIER_IMAGES for i in range(len(errors))])
        assert errors[good, 1].max() <= 4.0 * G.TRUE_SIM[0] * G.CENTER_NOISE and errors[~good, 1].min() > 0.5
        text = open(out / "errors.csv").read().splitlines()
        assert text[0].startswith("# Model comparison pose errors") and text[1] == "# <rotation error (deg)>, <proj center error>"
        summary = open(out / "errors_summary.txt").read()
        assert summary.startswith("\nRotation errors (degrees)\nMin:    ") and "\nProjection center errors\nMin:    " in summary
        assert [l.split(":")[0] for l in summary.splitlines()[2:8]] == ["Min", "Max", "Mean", "Median", "P90", "P99"]
        assert abs(float(summary.splitlines()[-4].split()[1]) - errors[:, 1].mean()) <= 1e-5 * errors[:, 1].mean()
    assert "Common images: 20" in capsys.readouterr().out
    assert _run("model_comparer", "--input_path1", p1, "--input_path2", p2, "--alignment_error", "nonsense") == 1
    few = G.build_pair([5, 6], seed=2)
    assert _run("model_comparer", "--input_path1", _write(few[0], str(tmp_path / "f1")), "--input_path2",
                _write(few[1], str(tmp_path / "f2"))) == 1  # fewer than 3 common images: the alignment fails


def test_model_transformer_round_trip(emulated_library, tmp_path):
    src, _ = G.search_pair()
    p0 = _write(src, str(tmp_path / "m0"))
    sim_path = str(tmp_path / "sim.txt")
    AL.Sim3d.from_params(G.TRUE_SIM).ToFile(sim_path)
    p1, p2 = str(tmp_path / "m1"), str(tmp_path / "m2")
    assert _run("model_transformer", "--input_path", p0, "--output_path", p1, "--transform_path", sim_path) == 0
    assert _run("model_transformer", "--input_path", p1, "--output_path", p2, "--transform_path", sim_path, "--is_inverse", 1) == 0
    c0, m0 = _centres(p0)
    c1, m1 = _centres(p1)
    c2, m2 = _centres(p2)
    for name in c0:
        assert np.allclose(c1[name], A.sim_apply(G.TRUE_SIM, c0[name]), rtol=0, atol=1e-12)
        assert np.allclose(c2[name], c0[name], rtol=0, atol=1e-12)
    for pid, p in m0.points3D.items():
        assert np.allclose(m1.points3D[pid].xyz, A.sim_apply(G.TRUE_SIM, p.xyz), rtol=0, atol=1e-12)
        assert np.allclose(m2.points3D[pid].xyz, p.xyz, rtol=0, atol=1e-12)
        assert m2.points3D[pid].track == p.track
    for i, im in m0.images.items():
        assert np.array_equal(m2.images[i].point3D_ids, im.point3D_ids) and np.array_equal(m2.images[i].xys, im.xys)
    # a point cloud: positions move, colours stay, normals are dropped
    rng = np.random.default_rng(0)
    cloud = fusion.FusedPoints(rng.uniform(-2, 2, (300, 3)).astype(np.float32), rng.normal(size=(300, 3)).astype(np.float32),
                               rng.integers(0, 256, (300, 3)).astype(np.uint8))
    ply0, ply1, ply2 = (str(tmp_path / f"c{k}.ply") for k in range(3))
    fusion.write_binary_ply_points(ply0, cloud)
    assert _run("model_transformer", "--input_path", ply0, "--output_path", ply1, "--transform_path", sim_path) == 0
    head, body = open(ply1, "rb").read().split(b"end_header\n", 1)
    assert b"property float nx" not in head and b"element vertex 300" in head and len(body) == 300 * 15
    rec = np.frombuffer(body, np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))]))
    want = np.array([A.sim_apply(G.TRUE_SIM, x) for x in cloud.xyz.astype(np.float64)])
    assert np.array_equal(rec["rgb"], cloud.rgb) and np.array_equal(rec["xyz"], want.astype(np.float32))
    assert _run("model_transformer", "--input_path", str(tmp_path / "nothing"), "--output_path", p2, "--transform_path", sim_path) == 1


def test_model_aligner_end_to_end(emulated_library, tmp_path, capsys):
    src, tgt = G.search_pair()
    names = {i: f"img{i:03d}.jpg" for i in src.images}
    p_src, p_ref = _write(src, str(tmp_path / "src"), names), _write(tgt, str(tmp_path / "ref"), names)
    ref_txt, sim_path = str(tmp_path / "ref.txt"), str(tmp_path / "sim.txt")
    with open(ref_txt, "w") as f:
        f.write("unknown.jpg 1 2 3\n")
        for i in sorted(tgt.images):
            f.write(names[i] + " " + " ".join(f"{v:.17g}" for v in tgt.ProjectionCenter(i)) + "\n")
    for k, ref_args in enumerate((["--ref_images_path", ref_txt, "--ref_is_gps", 0], ["--ref_model_path", p_ref])):
        out = str(tmp_path / f"out{k}")
        assert _run("model_aligner", "--input_path", p_src, "--output_path", out, "--alignment_max_error", 0.05,
                    "--transform_path", sim_path, *ref_args) == 0
        assert A.sim_distance(AL.Sim3d.FromFile(sim_path).params(), G.TRUE_SIM) <= 10 * G.CENTER_NOISE
        centres, _ = _centres(out)
        d = np.array([np.linalg.norm(centres[names[i]] - tgt.ProjectionCenter(i)) for i in sorted(tgt.images)
                      if i not in G.SEARCH_OUTLIER_IMAGES])
        assert d.max() <= 4.0 * G.TRUE_SIM[0] * G.CENTER_NOISE
        text = capsys.readouterr().out
        assert "=> Alignment error: " in text and "(mean)" in text and "(median)" in text and "=> Alignment succeeded" in text
    out = str(tmp_path / "merged")
    assert _run("model_aligner", "--input_path", p_src, "--output_path", out, "--alignment_max_error", 0.05,
                "--ref_model_path", p_ref, "--merge_image_and_ref_origins", 1, "--transform_path", sim_path) == 0
    centres, _ = _centres(out)
    assert np.allclose(centres[names[1]], tgt.ProjectionCenter(1), rtol=0, atol=1e-12)  # the first reference is met exactly
    moved = AL.Sim3d.FromFile(sim_path)
    assert np.allclose(moved * src.ProjectionCenter(1), tgt.ProjectionCenter(1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("args,message", [
    (["--alignment_type", "plane"], "alignment_type `plane` is not built"),
    (["--alignment_type", "enu", "--ref_images_path", "x.txt"], "alignment_type `enu` is not built"),
    (["--alignment_type", "ecef", "--ref_images_path", "x.txt"], "is not built"),
    (["--alignment_type", "enu-plane-unscaled", "--ref_images_path", "x.txt"], "is not built"),
    (["--database_path", "db.db"], "--database_path is not built"),
    (["--ref_images_path", "x.txt"], "GPS reference positions are not built"),
    (["--ref_images_path", "x.txt", "--ref_is_gps", "1"], "GPS reference positions are not built"),
    (["--alignment_type", "sideways", "--ref_images_path", "x.txt"], "Invalid `alignment_type`"),
    ([], "One of the following arguments must be specified"),
])
def test_model_aligner_says_what_is_not_built(tmp_path, capsys, args, message):
    assert _run("model_aligner", "--input_path", tmp_path, "--output_path", tmp_path, "--alignment_max_error", 0.1, *args) == 1
    assert message in capsys.readouterr().err


def test_model_aligner_reference_checks(tmp_path, capsys):
    assert _run("model_aligner", "--input_path", tmp_path, "--output_path", tmp_path, "--ref_images_path", "x.txt") == 1
    assert "You must provide a maximum alignment error > 0" in capsys.readouterr().err
    ref = tmp_path / "ref.txt"
    ref.write_text("a.jpg 0 0 0\nb.jpg 1 0 0\n")
    assert _run("model_aligner", "--input_path", tmp_path, "--output_path", tmp_path, "--ref_images_path", ref, "--ref_is_gps", 0,
                "--alignment_max_error", 0.1) == 1
    assert "Cannot align with insufficient reference locations." in capsys.readouterr().err
