"""The parts of a COLMAP `database.db` that descriptor matching reads and writes, through the standard library's sqlite3
(reference scene/database_sqlite.cc): image ids and names, SIFT descriptors, and the `matches` table. Pair ids and the
blob layout follow util/types.h:209-239 and database_sqlite.cc:1365-1390: pair_id = 2147483647 * min(id) + max(id); the
blob is uint32 [rows][2] in the order (smaller id's point, larger id's point); an empty result is rows = 0, cols = 2.
The matchers only look at `two_view_geometries`; `geometric_verifier` (colmap_amd/geometric_verifier.py) reads cameras,
keypoints and matches and writes its rows.
"""
from __future__ import annotations

import os
import sqlite3
from typing import Dict, List, Tuple

import numpy as np

MAX_NUM_IMAGES = 2147483647   # kMaxNumImages
SIFT_TYPE = 0                 # FeatureExtractorType::SIFT


class DatabaseError(RuntimeError):
    pass


def image_pair_to_pair_id(image_id1: int, image_id2: int) -> int:
    """ImagePairToPairId."""
    for i in (image_id1, image_id2):
        if not 0 <= i < MAX_NUM_IMAGES:
            raise DatabaseError(f"image id {i} outside [0, {MAX_NUM_IMAGES})")
    lo, hi = min(image_id1, image_id2), max(image_id1, image_id2)
    return MAX_NUM_IMAGES * lo + hi


def pair_id_to_image_pair(pair_id: int) -> Tuple[int, int]:
    """PairIdToImagePair: (smaller id, larger id)."""
    hi = pair_id % MAX_NUM_IMAGES
    return (pair_id - hi) // MAX_NUM_IMAGES, hi


def swap_image_pair(image_id1: int, image_id2: int) -> bool:
    return image_id1 > image_id2


class Database:
    def __init__(self, path: str, create: bool = False, descriptor_type_column: bool = True):
        if not create and not os.path.isfile(path):
            raise DatabaseError(f"database {path} does not exist")
        self.path = path
        self.con = sqlite3.connect(path)
        if create:
            self.create_tables(descriptor_type_column)
        self._has_type = "type" in self._columns("descriptors")

    # -- schema -----------------------------------------------------------------------------------------------------
    def _columns(self, table: str) -> List[str]:
        return [r[1] for r in self.con.execute(f"PRAGMA table_info({table})")]

    def _has_table(self, table: str) -> bool:
        return self.con.execute("SELECT 1 FROM sqlite_master WHERE type = 'table' AND name = ?", (table,)).fetchone() is not None

    def create_tables(self, descriptor_type_column: bool = True):
        """The tables this module touches, with the reference's column lists (a database made by `colmap` has more)."""
        kind = "type INTEGER NOT NULL, " if descriptor_type_column else ""
        self.con.executescript(
            "CREATE TABLE IF NOT EXISTS images (image_id INTEGER PRIMARY KEY AUTOINCREMENT NOT NULL, "
            "name TEXT NOT NULL UNIQUE, camera_id INTEGER NOT NULL);"
            f"CREATE TABLE IF NOT EXISTS descriptors (image_id INTEGER PRIMARY KEY NOT NULL, {kind}"
            "rows INTEGER NOT NULL, cols INTEGER NOT NULL, data BLOB);"
            "CREATE TABLE IF NOT EXISTS matches (pair_id INTEGER PRIMARY KEY NOT NULL, rows INTEGER NOT NULL, "
            "cols INTEGER NOT NULL, data BLOB);")
        self.create_verification_tables()   # cameras and keypoints: what feature extraction writes
        self._has_type = "type" in self._columns("descriptors")

    def close(self):
        self.con.commit()
        self.con.close()

    def commit(self):
        self.con.commit()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    pair_id = staticmethod(image_pair_to_pair_id)

    # -- images and descriptors -------------------------------------------------------------------------------------
    def read_image_names(self) -> Dict[int, str]:
        return {int(i): str(n) for i, n in self.con.execute("SELECT image_id, name FROM images ORDER BY image_id")}

    def read_image_ids(self) -> List[int]:
        return list(self.read_image_names())

    def write_image(self, name: str, camera_id: int = 1, image_id: int = None) -> int:
        cur = self.con.execute("INSERT INTO images (image_id, name, camera_id) VALUES (?, ?, ?)", (image_id, name, camera_id))
        return int(cur.lastrowid)

    def write_descriptors(self, image_id: int, descriptors: np.ndarray, type_id: int = SIFT_TYPE):
        d = np.ascontiguousarray(descriptors, dtype=np.uint8)
        if self._has_type:
            self.con.execute("INSERT INTO descriptors (image_id, type, rows, cols, data) VALUES (?, ?, ?, ?, ?)",
                             (image_id, type_id, d.shape[0], d.shape[1], d.tobytes()))
        else:
            self.con.execute("INSERT INTO descriptors (image_id, rows, cols, data) VALUES (?, ?, ?, ?)",
                             (image_id, d.shape[0], d.shape[1], d.tobytes()))

    def read_descriptors(self, image_id: int) -> np.ndarray:
        """[rows][128] uint8; an image without a descriptors row has none (as the reference's ReadDescriptors)."""
        cols = "type, rows, cols, data" if self._has_type else "0, rows, cols, data"   # older databases: SIFT only
        row = self.con.execute(f"SELECT {cols} FROM descriptors WHERE image_id = ?", (image_id,)).fetchone()
        if row is None:
            return np.zeros((0, 128), np.uint8)
        kind, rows, ncols, data = row
        if kind != SIFT_TYPE:
            raise DatabaseError(f"image {image_id}: descriptors of type {kind} are not SIFT (0): only 128-byte SIFT "
                                "descriptors under the dot-product metric are matched on the GPU")
        if ncols != 128:
            raise DatabaseError(f"image {image_id}: descriptors have {ncols} columns, not 128: the kernel is built for "
                                "SIFT's 128 bytes (two k-steps of the int8 matrix instruction)")
        data = data or b""
        if len(data) != rows * ncols:
            raise DatabaseError(f"image {image_id}: descriptor blob has {len(data)} bytes, expected {rows * ncols}")
        return np.frombuffer(data, np.uint8).reshape(rows, ncols)

    # -- matches ----------------------------------------------------------------------------------------------------
    def exists_matches(self, image_id1: int, image_id2: int) -> bool:
        pid = image_pair_to_pair_id(image_id1, image_id2)
        return self.con.execute("SELECT 1 FROM matches WHERE pair_id = ?", (pid,)).fetchone() is not None

    def exists_two_view_geometry(self, image_id1: int, image_id2: int) -> bool:
        if not self._has_table("two_view_geometries"):
            return False
        pid = image_pair_to_pair_id(image_id1, image_id2)
        return self.con.execute("SELECT 1 FROM two_view_geometries WHERE pair_id = ?", (pid,)).fetchone() is not None

    def write_matches(self, image_id1: int, image_id2: int, matches: np.ndarray):
        """matches: [n][2] (point of image_id1, point of image_id2); stored in the order of the pair id."""
        m = np.asarray(matches, dtype=np.uint32).reshape(-1, 2)
        if swap_image_pair(image_id1, image_id2):
            m = m[:, ::-1]
        m = np.ascontiguousarray(m)
        self.con.execute("INSERT INTO matches (pair_id, rows, cols, data) VALUES (?, ?, ?, ?)",
                         (image_pair_to_pair_id(image_id1, image_id2), m.shape[0], 2, m.tobytes()))

    def read_matches(self, image_id1: int, image_id2: int) -> np.ndarray:
        """[n][2] uint32 as (point of image_id1, point of image_id2); a pair without a row has none."""
        pid = image_pair_to_pair_id(image_id1, image_id2)
        row = self.con.execute("SELECT rows, cols, data FROM matches WHERE pair_id = ?", (pid,)).fetchone()
        if row is None or row[0] == 0:
            return np.zeros((0, 2), np.uint32)
        m = np.frombuffer(row[2], np.uint32).reshape(row[0], row[1])
        return np.ascontiguousarray(m[:, ::-1]) if swap_image_pair(image_id1, image_id2) else m.copy()

    def num_match_rows(self) -> int:
        return int(self.con.execute("SELECT COUNT(*) FROM matches").fetchone()[0])

    def num_two_view_geometry_rows(self) -> int:
        if not self._has_table("two_view_geometries"):
            return 0
        return int(self.con.execute("SELECT COUNT(*) FROM two_view_geometries").fetchone()[0])

    # -- what geometric verification reads and writes ---------------------------------------------------------------
    def create_verification_tables(self):
        """`cameras` and `keypoints` with the reference's column lists (database_sqlite.cc:2031-2038, 2101-2106), for
        databases made here; a database made by `colmap` has them."""
        self.con.executescript(
            "CREATE TABLE IF NOT EXISTS cameras (camera_id INTEGER PRIMARY KEY AUTOINCREMENT NOT NULL, "
            "model INTEGER NOT NULL, width INTEGER NOT NULL, height INTEGER NOT NULL, params BLOB, "
            "prior_focal_length INTEGER NOT NULL);"
            "CREATE TABLE IF NOT EXISTS keypoints (image_id INTEGER PRIMARY KEY NOT NULL, rows INTEGER NOT NULL, "
            "cols INTEGER NOT NULL, data BLOB);")

    # -- what feature extraction writes (controllers/feature_extraction.cc:238-300) ---------------------------------
    def write_camera(self, model: int, width: int, height: int, params, prior_focal_length: bool = False,
                     camera_id: int = None) -> int:
        """Database::WriteCamera (database_sqlite.cc): params as float64; returns the camera id."""
        blob = np.ascontiguousarray(params, np.float64).tobytes()
        cur = self.con.execute("INSERT INTO cameras (camera_id, model, width, height, params, prior_focal_length) "
                               "VALUES (?, ?, ?, ?, ?, ?)", (camera_id, int(model), int(width), int(height), blob,
                                                             int(bool(prior_focal_length))))
        return int(cur.lastrowid)

    def write_keypoints(self, image_id: int, keypoints: np.ndarray):
        """Database::WriteKeypoints: float32 [rows][6] = x, y, a11, a12, a21, a22 (or 2 / 4 columns), the form
        read_keypoints reads."""
        k = np.ascontiguousarray(keypoints, dtype=np.float32)
        if k.ndim != 2 or k.shape[1] not in (2, 4, 6):
            raise DatabaseError(f"image {image_id}: keypoints must be [rows][2, 4 or 6], got {k.shape}")
        self.con.execute("INSERT INTO keypoints (image_id, rows, cols, data) VALUES (?, ?, ?, ?)",
                         (image_id, k.shape[0], k.shape[1], k.tobytes()))

    def exists_keypoints(self, image_id: int) -> bool:
        return self._has_table("keypoints") and \
            self.con.execute("SELECT 1 FROM keypoints WHERE image_id = ?", (image_id,)).fetchone() is not None

    def exists_descriptors(self, image_id: int) -> bool:
        return self.con.execute("SELECT 1 FROM descriptors WHERE image_id = ?", (image_id,)).fetchone() is not None

    def read_cameras(self) -> Dict[int, dict]:
        """camera_id -> {model, width, height, params (float64), prior_focal_length} (database_sqlite.cc:2031-2038)."""
        out = {}
        for cid, model, width, height, params, prior in self.con.execute(
                "SELECT camera_id, model, width, height, params, prior_focal_length FROM cameras ORDER BY camera_id"):
            out[int(cid)] = {"model": int(model), "width": int(width), "height": int(height),
                             "params": np.frombuffer(params or b"", np.float64).copy(), "prior_focal_length": bool(prior)}
        return out

    def read_image_camera_ids(self) -> Dict[int, int]:
        return {int(i): int(c) for i, c in self.con.execute("SELECT image_id, camera_id FROM images ORDER BY image_id")}

    def read_keypoints(self, image_id: int) -> np.ndarray:
        """float32 [rows][cols], cols 2, 4 or 6, the first two are x, y (database_sqlite.cc:102-128); an image without
        a row has none."""
        if not self._has_table("keypoints"):
            return np.zeros((0, 2), np.float32)
        row = self.con.execute("SELECT rows, cols, data FROM keypoints WHERE image_id = ?", (image_id,)).fetchone()
        if row is None or row[0] == 0:
            return np.zeros((0, 2), np.float32)
        rows, cols, data = row
        if cols not in (2, 4, 6):
            raise DatabaseError(f"image {image_id}: keypoints have {cols} columns, expected 2, 4 or 6")
        if len(data or b"") != 4 * rows * cols:
            raise DatabaseError(f"image {image_id}: keypoint blob has {len(data or b'')} bytes, expected {4 * rows * cols}")
        return np.frombuffer(data, np.float32).reshape(rows, cols).copy()

    def read_matched_pair_ids(self) -> List[int]:
        """The pair ids of the `matches` table in pair-id order."""
        return [int(r[0]) for r in self.con.execute("SELECT pair_id FROM matches ORDER BY pair_id")]

    def exists_inlier_matches(self, image_id1: int, image_id2: int) -> bool:
        """ExistsInlierMatches: a two_view_geometries row with inlier matches."""
        if not self._has_table("two_view_geometries"):
            return False
        pid = image_pair_to_pair_id(image_id1, image_id2)
        return self.con.execute("SELECT 1 FROM two_view_geometries WHERE pair_id = ? AND rows > 0", (pid,)).fetchone() is not None

    def delete_two_view_geometry(self, image_id1: int, image_id2: int):
        if self._has_table("two_view_geometries"):
            self.con.execute("DELETE FROM two_view_geometries WHERE pair_id = ?", (image_pair_to_pair_id(image_id1, image_id2),))

    def write_two_view_geometry(self, image_id1: int, image_id2: int, inlier_matches: np.ndarray, config: int,
                                F: np.ndarray = None, H: np.ndarray = None):
        """One row of `two_view_geometries`; the table is created with the reference's column list
        (database_sqlite.cc:2144-2156) where it is absent, and only the columns an older table has are written.
        inlier_matches: [n][2] as (point of image_id1, point of image_id2), stored in the order of the pair id, as the
        matches blob. F and H are 9 row-major doubles; E, qvec, tvec, camera1 and camera2 stay NULL. A swapped pair
        would need TwoViewGeometry::Invert; geometric verification works in pair-id order, so a geometry with F or H
        is only accepted for image_id1 < image_id2."""
        if not self._has_table("two_view_geometries"):
            self.con.execute("CREATE TABLE IF NOT EXISTS two_view_geometries (pair_id INTEGER PRIMARY KEY NOT NULL, "
                             "rows INTEGER NOT NULL, cols INTEGER NOT NULL, data BLOB, config INTEGER NOT NULL, F BLOB, "
                             "E BLOB, H BLOB, qvec BLOB, tvec BLOB, camera1 BLOB, camera2 BLOB)")
        m = np.asarray(inlier_matches, dtype=np.uint32).reshape(-1, 2)
        if swap_image_pair(image_id1, image_id2):
            if F is not None or H is not None:
                raise DatabaseError("a two-view geometry with F or H must be written in the order of the pair id")
            m = m[:, ::-1]
        m = np.ascontiguousarray(m)

        def blob(a):
            return None if a is None else np.ascontiguousarray(a, np.float64).reshape(9).tobytes()
        values = {"pair_id": image_pair_to_pair_id(image_id1, image_id2), "rows": m.shape[0], "cols": 2,
                  "data": m.tobytes() if m.shape[0] else None, "config": int(config), "F": blob(F), "H": blob(H)}
        have = self._columns("two_view_geometries")
        cols = [c for c in values if c in have]
        self.con.execute(f"INSERT INTO two_view_geometries ({', '.join(cols)}) VALUES ({', '.join('?' * len(cols))})",
                         [values[c] for c in cols])
