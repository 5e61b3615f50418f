"""Descriptor matching without a GPU: the numpy checker against a literal triple loop, the three pair generators
against hand-written lists, the database round trip, the refusals, and the commands' registration and the options they
decline."""
import importlib
import sqlite3

import numpy as np
import pytest

import match_reference as R
from colmap_amd import __main__ as cli_main
from colmap_amd import database as DB
from colmap_amd import feature_matching as FM

COMMANDS = ("exhaustive_matcher", "sequential_matcher", "matches_importer")


# ---- the checker ------------------------------------------------------------------------------------------------------

def test_checker_against_a_literal_triple_loop():
    rng = np.random.default_rng(0)
    A, B = rng.integers(0, 256, (5, 128), dtype=np.uint8), rng.integers(0, 256, (7, 128), dtype=np.uint8)
    B[3] = B[5] = A[2]            # a doubled maximum
    A[4] = 0                      # an all-zero row
    D = R.dots(A, B)
    expect = []
    for i in range(5):
        best, second, idx = 0, 0, -1
        for j in range(7):
            dot = 0
            for k in range(128):
                dot += int(A[i, k]) * int(B[j, k])
            assert D[i, j] == dot
            if dot > best:
                idx, second, best = j, best, dot
            elif dot > second:
                second = dot
        expect.append([idx, best, second])
    sel = R.select(D)
    assert sel.tolist() == expect
    assert sel[2].tolist() == [3, int(D[2, 3]), int(D[2, 3])] and sel[4].tolist() == [-1, 0, 0]
    assert R.dots(np.full((1, 128), 255, np.uint8), np.full((1, 128), 255, np.uint8))[0, 0] == 8323200


def test_checker_decisions():
    def dot_at(angle):
        return int(round(262144 * np.cos(angle)))
    sel = np.array([[3, dot_at(0.3), dot_at(0.9)],     # accept
                    [3, dot_at(0.3), dot_at(0.3)],     # doubled maximum
                    [3, dot_at(0.9), 0],               # beyond max_distance
                    [3, dot_at(0.65), dot_at(0.7)],    # ratio
                    [-1, 0, 0],
                    [0, 128 * 255 * 255, 0]], np.int32)
    assert R.decide(sel).tolist() == [3, -1, -1, -1, -1, 0]
    assert R.decide(sel, 1.5, 2.0).tolist() == [3, 3, 3, 3, -1, 0]
    m12, m21 = np.array([1, 1, -1, 0], np.int32), np.array([3, 0, -1], np.int32)
    assert R.cross(m12, m21, True, 0).tolist() == [[0, 1], [3, 0]]
    assert R.cross(m12, m21, False, 0).tolist() == [[0, 1], [1, 1], [3, 0]]
    assert R.cross(m12, m21, True, 3).shape == (0, 2)


def test_generator_is_not_vacuous():
    for n1, n2 in ((1000, 1100), (193, 4097)):
        A, B, r12, r21 = R.case(n1, n2)
        assert A.shape == (n1, 128) and B.shape == (n2, 128) and A.dtype == np.uint8
        m = R.cross(R.decide(r12), R.decide(r21))
        assert 0.2 * n1 <= len(m) <= 0.8 * n1
        assert (R.decide(r12) >= 0).sum() > len(m)                     # the cross check rejects some
        assert ((r12[:, 1] == r12[:, 2]) & (r12[:, 0] >= 0)).sum() > 0    # doubled maxima occur
    with pytest.raises(ValueError):
        R.case(5, 5)[0][0, 0] = 1                                        # shared, read-only


# ---- pair generators ---------------------------------------------------------------------------------------------------

def test_exhaustive_pairs_block_edges():
    ids = [10, 20, 30, 40, 50]
    blocks = list(FM.exhaustive_pair_blocks(ids, 2))
    # block ids are index % 2; cells (block1, block2) in row-major order. idx1 < idx2 needs block_id1 < block_id2,
    # idx1 > idx2 needs block_id1 <= block_id2
    assert blocks == [
        [(10, 20)], [(10, 40)], [],
        [(30, 10), (30, 20), (40, 20)], [(30, 40)], [],
        [(50, 10), (50, 20)], [(50, 30), (50, 40)], [],
    ]
    pairs = [p for b in blocks for p in b]
    # the rule by hand: idx1, idx2 in the same block grid cell; block ids are idx % 2
    expect = []
    for s1 in (0, 2, 4):
        for s2 in (0, 2, 4):
            for i1 in range(s1, min(5, s1 + 2)):
                for i2 in range(s2, min(5, s2 + 2)):
                    if (i1 > i2 and i1 % 2 <= i2 % 2) or (i1 < i2 and i1 % 2 < i2 % 2):
                        expect.append((ids[i1], ids[i2]))
    assert pairs == expect
    # every unordered pair exactly once
    assert sorted(tuple(sorted(p)) for p in pairs) == [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]]
    with pytest.raises(FM.FeatureMatchingError):
        list(FM.exhaustive_pair_blocks(ids, 1))


def test_sequential_pairs():
    ids = [5, 3, 9, 1, 7, 2]     # already in name order
    plain = [p for b in FM.sequential_pair_blocks(ids, 3, False) for p in b]
    assert plain == [(5, 3), (5, 9), (5, 1), (3, 9), (3, 1), (3, 7), (9, 1), (9, 7), (9, 2), (1, 7), (1, 2), (7, 2)]
    quadratic = [p for b in FM.sequential_pair_blocks(ids, 3, True) for p in b]
    assert quadratic == [(5, 3), (5, 9), (5, 7), (3, 9), (3, 1), (3, 2), (9, 1), (9, 7), (1, 7), (1, 2), (7, 2)]
    assert [len(b) for b in FM.sequential_pair_blocks(ids, 3, True)] == [3, 3, 2, 2, 1, 0]
    assert FM.order_by_name({1: "b.jpg", 2: "a.jpg", 3: "c/a.jpg", 4: "B.jpg"}) == [4, 2, 1, 3]


def test_imported_pairs(tmp_path, capsys):
    names = {1: "a.jpg", 2: "b.jpg", 3: "sub/c.jpg"}
    path = tmp_path / "pairs.txt"
    path.write_text("# comment\na.jpg b.jpg\n\nsub/c.jpg a.jpg\nb.jpg missing.jpg\nb.jpg sub/c.jpg\n")
    blocks = list(FM.imported_pair_blocks(str(path), names, block_size=2))
    assert blocks == [[(1, 2), (3, 1)], [(2, 3)]]
    assert "missing.jpg does not exist" in capsys.readouterr().err
    path.write_text("a.jpg\n")
    with pytest.raises(FM.FeatureMatchingError, match="name1 name2"):
        list(FM.imported_pair_blocks(str(path), names))


# ---- database ----------------------------------------------------------------------------------------------------------

def test_pair_ids():
    assert DB.image_pair_to_pair_id(1, 2) == 2147483647 + 2 == DB.image_pair_to_pair_id(2, 1)
    assert DB.pair_id_to_image_pair(DB.image_pair_to_pair_id(7, 3)) == (3, 7)
    assert DB.swap_image_pair(7, 3) and not DB.swap_image_pair(3, 7)
    with pytest.raises(DB.DatabaseError):
        DB.image_pair_to_pair_id(1, 2147483647)


def test_database_round_trip(tmp_path):
    path = str(tmp_path / "database.db")
    rng = np.random.default_rng(1)
    d1, d2 = rng.integers(0, 256, (5, 128), dtype=np.uint8), rng.integers(0, 256, (0, 128), dtype=np.uint8)
    with DB.Database(path, create=True) as db:
        assert db.write_image("b.jpg") == 1 and db.write_image("a.jpg") == 2 and db.write_image("c.jpg", image_id=7) == 7
        db.write_descriptors(1, d1)
        db.write_descriptors(2, d2)
    with DB.Database(path) as db:
        assert db.read_image_names() == {1: "b.jpg", 2: "a.jpg", 7: "c.jpg"} and db.read_image_ids() == [1, 2, 7]
        np.testing.assert_array_equal(db.read_descriptors(1), d1)
        assert db.read_descriptors(2).shape == (0, 128) and db.read_descriptors(7).shape == (0, 128)
        m = np.array([[0, 4], [2, 1], [3, 3]], np.uint32)
        assert not db.exists_matches(1, 2) and not db.exists_two_view_geometry(1, 2)
        db.write_matches(1, 2, m)
        db.write_matches(7, 1, m)                       # swapped: stored as (point of 1, point of 7)
        db.write_matches(2, 7, np.zeros((0, 2), np.uint32))
        assert db.exists_matches(2, 1) and db.exists_matches(1, 7) and db.exists_matches(7, 2)
        np.testing.assert_array_equal(db.read_matches(1, 2), m)
        np.testing.assert_array_equal(db.read_matches(2, 1), m[:, ::-1])
        np.testing.assert_array_equal(db.read_matches(7, 1), m)
        np.testing.assert_array_equal(db.read_matches(1, 7), m[:, ::-1])
        assert db.read_matches(2, 7).shape == (0, 2) and db.read_matches(1, 99).shape == (0, 2)
        with pytest.raises(sqlite3.IntegrityError):
            db.write_matches(2, 1, m)                   # one row per pair, as in the reference
    # the stored rows, read with sqlite3 alone
    con = sqlite3.connect(path)
    rows = {r[0]: r[1:] for r in con.execute("SELECT pair_id, rows, cols, data FROM matches")}
    con.close()
    assert rows[2147483647 * 1 + 2] == (3, 2, m.tobytes())
    assert rows[2147483647 * 1 + 7] == (3, 2, np.ascontiguousarray(m[:, ::-1]).tobytes())
    assert rows[2147483647 * 2 + 7][:2] == (0, 2) and not rows[2147483647 * 2 + 7][2]
    with pytest.raises(DB.DatabaseError, match="does not exist"):
        DB.Database(str(tmp_path / "missing.db"))


def test_database_without_the_type_column_and_refusals(tmp_path):
    path = str(tmp_path / "old.db")
    d = np.arange(3 * 128, dtype=np.uint32).reshape(3, 128).astype(np.uint8)
    with DB.Database(path, create=True, descriptor_type_column=False) as db:
        assert "type" not in db._columns("descriptors")
        db.write_image("a.jpg")
        db.write_descriptors(1, d)
        np.testing.assert_array_equal(db.read_descriptors(1), d)
    path = str(tmp_path / "new.db")
    with DB.Database(path, create=True) as db:
        for name in ("a", "b", "c"):
            db.write_image(name)
        db.write_descriptors(1, d, type_id=1)                       # ALIKED_N16ROT
        db.write_descriptors(2, np.zeros((3, 64), np.uint8))
        db.con.execute("INSERT INTO descriptors (image_id, type, rows, cols, data) VALUES (3, 0, 3, 128, ?)", (b"xx",))
        with pytest.raises(DB.DatabaseError, match="not SIFT"):
            db.read_descriptors(1)
        with pytest.raises(DB.DatabaseError, match="64 columns, not 128"):
            db.read_descriptors(2)
        with pytest.raises(DB.DatabaseError, match="blob has 2 bytes"):
            db.read_descriptors(3)


def test_options_mirror():
    o = FM.SiftMatchingOptions()
    assert (o.max_ratio, o.max_distance, o.cross_check, o.max_num_matches, o.min_num_inliers) == (0.8, 0.7, True, 32768, 15)
    c = o.to_c()
    assert (c.max_ratio, c.max_distance) == (np.float32(0.8), np.float32(0.7)) and c.cross_check == 1 and c.min_num_inliers == 15
    assert FM.device_bytes(0) == 0 and FM.device_bytes(1) == 64 * 132 and FM.device_bytes(65) == 128 * 132


# ---- commands ----------------------------------------------------------------------------------------------------------

def test_commands_are_registered():
    for name in COMMANDS:
        assert name in cli_main.COMMANDS
        assert callable(importlib.import_module(cli_main.COMMANDS[name][0]).main)


def run(command, *args):
    return importlib.import_module(cli_main.COMMANDS[command][0]).main([str(a) for a in args])


@pytest.fixture
def empty_db(tmp_path):
    path = str(tmp_path / "database.db")
    DB.Database(path, create=True).close()
    return path


@pytest.mark.parametrize("command,option,value,needle", [
    ("exhaustive_matcher", "--FeatureMatching.guided_matching", "1", "guided_matching is not built"),
    ("exhaustive_matcher", "--FeatureMatching.rig_verification", "1", "rig_verification is not built"),
    ("exhaustive_matcher", "--FeatureMatching.type", "ALIKED_LIGHTGLUE", "ALIKED"),
    ("exhaustive_matcher", "--FeatureMatching.type", "SIFT_LIGHTGLUE", "LightGlue"),
    ("exhaustive_matcher", "--FeatureMatching.use_gpu", "0", "no CPU matcher"),
    ("exhaustive_matcher", "--FeatureMatching.skip_geometric_verification", "0", "two-view geometry estimation is missing"),
    ("sequential_matcher", "--SequentialMatching.loop_detection", "1", "loop_detection is not built"),
    ("sequential_matcher", "--SequentialMatching.expand_rig_images", "1", "expand_rig_images is not built"),
    ("sequential_matcher", "--FeatureMatching.guided_matching", "1", "guided_matching is not built"),
])
def test_unsupported_options_exit_1(empty_db, capsys, command, option, value, needle):
    assert run(command, "--database_path", empty_db, option, value) == 1
    assert needle in capsys.readouterr().err


@pytest.mark.parametrize("match_type", ["raw", "inliers"])
def test_matches_importer_types_exit_1(empty_db, tmp_path, capsys, match_type):
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("")
    assert run("matches_importer", "--database_path", empty_db, "--match_list_path", pairs, "--match_type", match_type) == 1
    assert f"match_type {match_type} is not built" in capsys.readouterr().err


@pytest.mark.parametrize("command,what", [("vocab_tree_matcher", "vocabulary-tree pairing"),
                                          ("spatial_matcher", "spatial pairing"),
                                          ("transitive_matcher", "transitive pairing")])
def test_other_pairings_exit_1(capsys, command, what):
    assert cli_main.main([command, "--database_path", "x.db"]) == 1
    err = capsys.readouterr().err
    assert "is not built" in err and what in err


def test_missing_database_exits_1(tmp_path, capsys):
    assert run("exhaustive_matcher", "--database_path", tmp_path / "none.db") == 1
    assert "does not exist" in capsys.readouterr().err
