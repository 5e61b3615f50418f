"""SIFT descriptor matching on the MI355X (include/colmap_amd_match.h, colmap_amd/csrc/feature_match.hip): the Python
mirror of include/colmap_amd/feature_matching.hpp, the pair generators of the reference's controllers/pairing.cc and the
controller loop of controllers/feature_matching_utils.cc:423-518 over a colmap_amd.database.Database.

A FeatureMatcher keeps descriptor sets resident on the device by image id (SiftGPUFeatureMatcher's SetDescriptors reuse
and FeatureMatcherCache) and matches a list of pairs in one launch. There is no CPU path: a missing library is an error.
"""
from __future__ import annotations

import ctypes as C
import sys
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

DESCRIPTOR_DIM = 128
DEFAULT_BATCH_PAIRS = 64  # pairs per launch of the controller loop: DESIGN.md 2.4e


class FeatureMatchingError(RuntimeError):
    pass


class MatchOptions(C.Structure):
    """match_options."""
    _fields_ = [("max_ratio", C.c_float), ("max_distance", C.c_float), ("cross_check", C.c_int32),
                ("min_num_inliers", C.c_int32)]


class MatchPair(C.Structure):
    _fields_ = [("image_id1", C.c_uint32), ("image_id2", C.c_uint32)]


@dataclass
class SiftMatchingOptions:
    """SiftMatchingOptions (feature/sift.h) with FeatureMatchingOptions::max_num_matches and
    TwoViewGeometryOptions::min_num_inliers, the fields the brute-force GPU matcher reads."""
    max_ratio: float = 0.8
    max_distance: float = 0.7
    cross_check: bool = True
    max_num_matches: int = 32768
    min_num_inliers: int = 15

    def to_c(self) -> MatchOptions:
        return MatchOptions(self.max_ratio, self.max_distance, 1 if self.cross_check else 0, self.min_num_inliers)


def lib() -> C.CDLL:
    L = _lib.lib()
    if not hasattr(L, "match_pairs"):
        raise _lib.LibraryMissingError("the loaded library has no match_* entry points: rebuild it "
                                       "(`python -m colmap_amd.build`)")
    return declare(L)


def declare(L: C.CDLL) -> C.CDLL:
    """The prototypes of include/colmap_amd_match.h on a loaded library."""
    L.match_last_error.restype = C.c_char_p
    L.match_destroy.restype = None
    L.match_destroy.argtypes = [C.c_void_p]
    L.match_create.argtypes = [C.c_int32, C.c_int32, C.c_size_t, C.POINTER(C.c_void_p)]
    L.match_set_descriptors.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p]
    L.match_has_descriptors.argtypes = [C.c_void_p, C.c_uint32]
    L.match_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.match_num_matches.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    L.match_copy_matches.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.match_num_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    L.match_copy_selection.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]
    L.match_cache_stats.restype = None
    L.match_cache_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.match_last_timing.restype = None
    L.match_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return L


def _check(L, rc):
    if rc != 0:
        raise FeatureMatchingError(L.match_last_error().decode())


def tile_rows() -> int:
    return int(lib().match_tile_rows())


def device_bytes(rows: int) -> int:
    """Device bytes of a resident set (match_plan::device_bytes): rows padded to 64, 128 + 4 bytes each."""
    return (rows + 63) // 64 * 64 * (DESCRIPTOR_DIM + 4)


class FeatureMatcher:
    """SiftGPUFeatureMatcher (feature/sift.cc:1346-1473) over the C ABI, for many pairs per call."""

    def __init__(self, options: Optional[SiftMatchingOptions] = None, gpu_index: int = 0, cache_bytes: int = 0):
        self.options = options or SiftMatchingOptions()
        self._L = lib()
        self._h = C.c_void_p()
        _check(self._L, self._L.match_create(gpu_index, self.options.max_num_matches, cache_bytes, C.byref(self._h)))
        limit = self.options.max_num_matches or 32768
        self.cache_bytes = max(cache_bytes or (4 << 30), 2 * device_bytes(limit))   # match_plan::effective_cache_bytes
        self._rows: Dict[int, int] = {}   # rows that take part, per image ever uploaded

    def close(self):
        if self._h:
            self._L.match_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the cache --------------------------------------------------------------------------------------------------
    def set_descriptors(self, image_id: int, descriptors: np.ndarray):
        d = np.asarray(descriptors)
        if d.ndim != 2:
            raise FeatureMatchingError("descriptors must be a 2-D array")
        if d.dtype != np.uint8:
            raise FeatureMatchingError(f"descriptors must be uint8, got {d.dtype}")
        d = np.ascontiguousarray(d)
        _check(self._L, self._L.match_set_descriptors(self._h, image_id, d.shape[0], d.shape[1],
                                                      d.ctypes.data_as(C.c_void_p)))
        self._rows[image_id] = min(d.shape[0], self.options.max_num_matches or 32768)

    def has_descriptors(self, image_id: int) -> bool:
        return bool(self._L.match_has_descriptors(self._h, image_id))

    def cache_stats(self) -> Dict[str, int]:
        e, b, v = C.c_int64(), C.c_int64(), C.c_int64()
        self._L.match_cache_stats(self._h, C.byref(e), C.byref(b), C.byref(v))
        return {"entries": e.value, "bytes": b.value, "evictions": v.value}

    def last_timing(self) -> Tuple[float, float]:
        k, t = C.c_double(), C.c_double()
        self._L.match_last_timing(C.byref(k), C.byref(t))
        return k.value, t.value

    # -- matching ---------------------------------------------------------------------------------------------------
    def match_resident(self, pairs: Sequence[Tuple[int, int]], selections: bool = False):
        """One launch for `pairs`, whose images must be resident. Returns the list of FeatureMatches, each [n][2] uint32;
        with selections=True a list of (matches, sel12, sel21), sel = [rows][3] int32 (idx, best, second)."""
        n = len(pairs)
        arr = (MatchPair * max(n, 1))(*[MatchPair(int(a), int(b)) for a, b in pairs])
        opts = self.options.to_c()
        _check(self._L, self._L.match_pairs(self._h, arr if n else None, n, C.byref(opts)))
        out = []
        for k in range(n):
            count = C.c_int64()
            _check(self._L, self._L.match_num_matches(self._h, k, C.byref(count)))
            m = np.zeros((count.value, 2), np.uint32)
            _check(self._L, self._L.match_copy_matches(self._h, k, m.ctypes.data_as(C.c_void_p), count.value))
            if not selections:
                out.append(m)
                continue
            sels = []
            for d in (0, 1):
                rows = C.c_int64()
                _check(self._L, self._L.match_num_rows(self._h, k, d, C.byref(rows)))
                s = np.zeros((rows.value, 3), np.int32)
                _check(self._L, self._L.match_copy_selection(self._h, k, d, s.ctypes.data_as(C.c_void_p), rows.value))
                sels.append(s)
            out.append((m, sels[0], sels[1]))
        return out

    def Match(self, descriptors1: np.ndarray, descriptors2: np.ndarray, image_id1: int = 1, image_id2: int = 2) -> np.ndarray:
        """FeatureMatcher::Match (feature/matcher.h) of one pair given by value."""
        self.set_descriptors(image_id1, descriptors1)
        self.set_descriptors(image_id2, descriptors2)
        return self.match_resident([(image_id1, image_id2)])[0]

    def match_pairs(self, pairs: Sequence[Tuple[int, int]], load: Callable[[int], np.ndarray],
                    batch_pairs: int = DEFAULT_BATCH_PAIRS) -> List[np.ndarray]:
        """Matches `pairs` with descriptors fetched through load(image_id) where they are not resident. The list is cut
        into launches of at most batch_pairs pairs whose distinct images fit the cache together."""
        results: List[np.ndarray] = []
        limit = self.options.max_num_matches or 32768
        group: List[Tuple[int, int]] = []
        needed: Dict[int, int] = {}          # image id -> device bytes
        fetched: Dict[int, np.ndarray] = {}

        def bytes_of(image_id):
            if self.has_descriptors(image_id):
                return device_bytes(self._rows[image_id])
            if image_id not in fetched:
                fetched[image_id] = load(image_id)
            return device_bytes(min(len(fetched[image_id]), limit))

        def flush():
            for image_id in needed:          # the resident ones become the most recently used: uploads drop others
                self.has_descriptors(image_id)
            for image_id in needed:
                if not self.has_descriptors(image_id):
                    self.set_descriptors(image_id, fetched.pop(image_id) if image_id in fetched else load(image_id))
            results.extend(self.match_resident(group))
            group.clear()
            needed.clear()   # (what was fetched for the pair that opens the next group stays in `fetched`)

        for a, b in pairs:
            extra = {i: bytes_of(i) for i in (a, b) if i not in needed}
            if group and (len(group) >= batch_pairs or
                          sum(needed.values()) + sum(extra.values()) > self.cache_bytes):
                flush()
                extra = {i: bytes_of(i) for i in (a, b)}
            needed.update(extra)
            group.append((a, b))
        if group:
            flush()
        return results


# ----------------------------------------------------------------------------------------------------------------------
# pair generators (controllers/pairing.cc)
# ----------------------------------------------------------------------------------------------------------------------

def exhaustive_pair_blocks(image_ids: Sequence[int], block_size: int = 50) -> Iterator[List[Tuple[int, int]]]:
    """ExhaustivePairGenerator::Next (pairing.cc:200-233): one list per (block1, block2), with its rule against
    duplicates: inside the block grid a pair is taken where the first index is later in the sequence and not later in its
    block, or earlier in the sequence and earlier in its block."""
    if block_size <= 1:
        raise FeatureMatchingError("ExhaustiveMatching.block_size must be greater than 1")
    n = len(image_ids)
    for start1 in range(0, n, block_size):
        for start2 in range(0, n, block_size):
            block = []
            for idx1 in range(start1, min(n, start1 + block_size)):
                for idx2 in range(start2, min(n, start2 + block_size)):
                    b1, b2 = idx1 % block_size, idx2 % block_size
                    if (idx1 > idx2 and b1 <= b2) or (idx1 < idx2 and b1 < b2):
                        block.append((image_ids[idx1], image_ids[idx2]))
            yield block


def sequential_pair_blocks(ordered_image_ids: Sequence[int], overlap: int = 10,
                           quadratic_overlap: bool = True) -> Iterator[List[Tuple[int, int]]]:
    """SequentialPairGenerator::Next (pairing.cc:521-576) over image ids ordered by name (:578-600): image i with
    i + 1 .. i + overlap, or with i + 2^0 .. i + 2^(overlap - 1)."""
    if overlap <= 0:
        raise FeatureMatchingError("SequentialMatching.overlap must be positive")
    n = len(ordered_image_ids)
    for i in range(n):
        block = []
        for k in range(overlap):
            j = i + (1 << k) if quadratic_overlap else i + k + 1
            if j >= n:
                break
            block.append((ordered_image_ids[i], ordered_image_ids[j]))
        yield block


def order_by_name(names: Dict[int, str]) -> List[int]:
    return [i for i, _ in sorted(names.items(), key=lambda kv: kv[1])]


def imported_pair_blocks(path: str, names: Dict[int, str], block_size: int = 1225) -> Iterator[List[Tuple[int, int]]]:
    """ImportedPairGenerator (pairing.cc:786-870): a text file of `name1 name2` lines, empty lines and `#` comments
    skipped; a name the database does not know is reported and its pair skipped."""
    by_name = {v: k for k, v in names.items()}
    pairs = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            parts = line.split()
            if len(parts) < 2:
                raise FeatureMatchingError(f"{path}: expected `name1 name2`, got `{line}`")
            missing = [p for p in parts[:2] if p not in by_name]
            if missing:
                print(f"E Image {missing[0]} does not exist.", file=sys.stderr)
                continue
            pairs.append((by_name[parts[0]], by_name[parts[1]]))
    for s in range(0, len(pairs), block_size):
        yield pairs[s:s + block_size]


# ----------------------------------------------------------------------------------------------------------------------
# the controller loop
# ----------------------------------------------------------------------------------------------------------------------

def match_blocks(database, blocks: Iterable[List[Tuple[int, int]]], options: Optional[SiftMatchingOptions] = None,
                 gpu_index: int = 0, cache_bytes: int = 0, batch_pairs: int = DEFAULT_BATCH_PAIRS,
                 matcher: Optional[FeatureMatcher] = None) -> Dict[str, int]:
    """FeatureMatcherController::Match (feature_matching_utils.cc:423-518) with skip_geometric_verification: per block,
    self pairs, repeated pairs and pairs that already have matches are skipped, the rest is matched in batched launches
    and written. No two_view_geometries row is written. Returns the counts of pairs matched and skipped."""
    own = matcher is None
    matcher = matcher or FeatureMatcher(options, gpu_index, cache_bytes)
    stats = {"matched": 0, "skipped": 0, "matches": 0}
    try:
        for block in blocks:
            seen, todo = set(), []
            for a, b in block:
                if a == b:
                    stats["skipped"] += 1
                    continue
                pid = database.pair_id(a, b)
                if pid in seen or database.exists_matches(a, b):
                    stats["skipped"] += 1
                    continue
                seen.add(pid)
                todo.append((a, b))
            if not todo:
                continue
            found = matcher.match_pairs(todo, database.read_descriptors, batch_pairs)
            for (a, b), m in zip(todo, found):
                database.write_matches(a, b, m)
                stats["matches"] += len(m)
            database.commit()
            stats["matched"] += len(todo)
    finally:
        if own:
            matcher.close()
    return stats
