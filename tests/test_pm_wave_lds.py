"""CPU only: the LDS block of a four-wave workgroup of the 11 x 11 sweep kernels (pm_kernels.hip: lds_offsets_wave) at
the benchmark's shape. Five photometric workgroups share a CU's 160 KB only up to 32 768 bytes each (32 000 in whole
allocation granules), four geometric ones up to 40 960: one byte more silently costs a workgroup per CU."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from colmap_amd import build
    build.build()
    L = C.CDLL(build.LIB_PATH)
    L.pm_debug_wave_lds_bytes.restype = C.c_size_t
    L.pm_debug_wave_lds_bytes.argtypes = [C.c_int32] * 4
    L.pm_debug_pick_columns.restype = C.c_int32
    L.pm_debug_pick_columns.argtypes = [C.c_int32] * 3
    return L


def _granules(nbytes):
    return -(-nbytes // 1280)   # LDS is allocated in granules of 1 280 bytes, 128 of them per CU


def test_bench_shape_fits_five_photometric_and_four_geometric_workgroups(lib):
    """C = 2, S = 20, M = 15. The byte bounds, and what the hardware really grants: whole granules -- a block of 32 720
    bytes passes the first test and still runs four to a CU (sweep launches 472 ms against 444:
    profiles/r07_bench_ab_44_byte_record/)."""
    photo, geom = lib.pm_debug_wave_lds_bytes(20, 15, 2, 0), lib.pm_debug_wave_lds_bytes(20, 15, 2, 1)
    assert photo <= 32768 and geom <= 40960
    assert 5 * _granules(photo) <= 128, photo
    assert 4 * _granules(geom) <= 128, geom


@pytest.mark.parametrize("geom", [0, 1])
@pytest.mark.parametrize("S", [4, 12, 20, 32])
def test_default_columns_per_wave(lib, S, geom):
    """Two columns per wave while the four-wave block stays within 40 960 bytes: 2, 2, 2 and, at S = 32, 2 photometric
    / 1 geometric -- the round records changed none of these."""
    want = 1 if (S == 32 and geom) else 2
    assert lib.pm_debug_pick_columns(S, 15, geom) == want
    assert lib.pm_debug_wave_lds_bytes(S, 15, want, geom) <= 40960
