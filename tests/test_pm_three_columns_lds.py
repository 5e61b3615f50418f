"""CPU only: the LDS block of pm_sweep_quad_kernel at three columns per wave (four waves per workgroup,
pm_kernels.hip: lds_offsets_wave) at the benchmark's S = 20, M = 15. The shape was measured, and its rule counts wave
slots, at four workgroups per CU, which the CU's 128 granules of 1 280 bytes must hold; the geometric block of three
columns exceeds the 40 960 bytes a workgroup may have, which is why pm_host::PlanWideColumns leaves the geometric pass
at two columns."""
import ctypes as C

import pytest

WORKGROUPS_PER_CU = 4   # pm_host::PlanWideColumns: 16 wave slots per CU = four four-wave workgroups
WAVE_BUDGET = 40960     # pm_kernels.hip: kQuadLdsBudget (wave_kernels_fit)


@pytest.fixture(scope="module")
def lib():
    from colmap_amd import build
    build.build()
    L = C.CDLL(build.LIB_PATH)
    L.pm_debug_wave_lds_bytes.restype = C.c_size_t
    L.pm_debug_wave_lds_bytes.argtypes = [C.c_int32] * 4
    return L


def _granules(nbytes):
    return -(-nbytes // 1280)   # LDS is allocated in granules of 1 280 bytes, 128 of them per CU


def test_four_photometric_workgroups_of_three_columns_share_a_cu(lib):
    photo = lib.pm_debug_wave_lds_bytes(20, 15, 3, 0)
    assert photo <= WAVE_BUDGET, photo
    assert WORKGROUPS_PER_CU * _granules(photo) <= 128, photo
    # ... and two columns still leave room for the five the two-column kernel is compiled for
    assert 5 * _granules(lib.pm_debug_wave_lds_bytes(20, 15, 2, 0)) <= 128


def test_geometric_block_of_three_columns_exceeds_the_budget(lib):
    assert lib.pm_debug_wave_lds_bytes(20, 15, 3, 1) > WAVE_BUDGET
    assert lib.pm_debug_wave_lds_bytes(20, 15, 2, 1) <= WAVE_BUDGET
