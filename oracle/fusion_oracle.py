"""ctypes binding of oracle/libfusion_oracle.so (fusion_oracle.cpp) -- TEST INFRASTRUCTURE ONLY.

    fuse(options, images, overlapping_images, mode)   mode 0: the reference's sequential walk, pixels row-major
                                                      mode 1: the same walk, turns in the order of the reference's
                                                              pool schedule (what fusion.hip computes)
                                                      mode 2: simulation of fusion.hip's passes (== mode 1)

    fuse_census(options, images, overlapping_images, mode=1)   the same through the census build: (points, counts)
    fuse_extremes(options, images, overlapping_images)         mode 2 and its extremes: (points, {deepest stack, ...})

Takes the same arguments as colmap_amd.fusion.fuse and reuses its marshalling, so both sides see the
identical structs.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libfusion_oracle.so")
        src = os.path.join(_HERE, "fusion_oracle.cpp")
        if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
            subprocess.check_call(["make", "-C", _HERE, "libfusion_oracle.so"])
        _LIB = C.CDLL(path)
        _LIB.fuo_last_error.restype = C.c_char_p
        _LIB.fuo_num_points.restype = C.c_size_t
    return _LIB


# ---- census build: the same source with counters of the rarely taken paths (fusion_oracle.cpp: FUO_CENSUS) ----------
# A second library, loaded only by the tests of the degenerate-input cases (tests/fusion_edge_cases.py); lib() above,
# what smoke() and bench.py's cpu_baseline use, never touches it.
CENSUS_FIELDS = ("seed_depth_nonpos", "nb_depth_nonpos", "depth_subnormal", "proj_z_nonpos", "coord_nonfinite",
                 "coord_tie", "coord_neg_zero", "coord_far_edge", "depth_err_at_bar", "reproj_at_bar", "cos_at_bar",
                 "cos_zero_below_bar", "seed_out_of_box", "nb_out_of_box", "on_box_face", "support_1", "support_2",
                 "support_even", "support_odd", "median_tie", "normal_too_short", "normal_at_epsilon", "colour_tie",
                 "colour_outside", "cap_reached", "level_bound", "below_min_pixels")
_CENSUS_LIB = None


def census_lib():
    global _CENSUS_LIB
    if _CENSUS_LIB is None:
        path = os.path.join(_HERE, "libfusion_oracle_census.so")
        src = os.path.join(_HERE, "fusion_oracle.cpp")
        if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
            subprocess.check_call(["make", "-C", _HERE, "libfusion_oracle_census.so"], stdout=subprocess.DEVNULL)
        _CENSUS_LIB = C.CDLL(path)
        _CENSUS_LIB.fuo_last_error.restype = C.c_char_p
        _CENSUS_LIB.fuo_num_points.restype = C.c_size_t
        assert _CENSUS_LIB.fuo_census(None, 0, 0) == len(CENSUS_FIELDS)
    return _CENSUS_LIB


class _EntryPoints:
    def __init__(self, mode, L=None):
        L = L or lib()
        self.run = lambda *a: L.fuo_run(C.c_int32(mode), *a)
        self.num_points, self.get_points = L.fuo_num_points, L.fuo_get_points
        self.get_visibility, self.free, self.last_error = L.fuo_get_visibility, L.fuo_free, L.fuo_last_error


def fuse(options, images, overlapping_images, mode):
    from colmap_amd import fusion
    return fusion.fuse(options, images, overlapping_images, entry_points=_EntryPoints(mode))


EXTREME_FIELDS = ("deepest_stack", "deepest_committed_stack", "largest_support", "largest_step_records")


def fuse_extremes(options, images, overlapping_images):
    """fuse() in mode 2, and what that run says about the input under these options: (points, {deepest_stack: entries
    on the stack of any walk after an expansion's pushes, deepest_committed_stack: the same over the committed walks
    (which every execution of the schedule repeats entry for entry; speculative walks depend on timing),
    largest_support: in-box pixels of a committed walk, largest_step_records: pixels recorded by the committed walks of one image step}). They decide which capacities of
    fusion.hip a run reaches (tests/fusion_capacity_cases.py); they never change a result."""
    out = fuse(options, images, overlapping_images, mode=2)
    vals = [C.c_longlong() for _ in EXTREME_FIELDS]
    lib().fuo_last_extremes(*[C.byref(v) for v in vals])
    return out, dict(zip(EXTREME_FIELDS, (v.value for v in vals)))


def fuse_census(options, images, overlapping_images, mode=1):
    """fuse() through the census build: (points, {counter name: count of this solve})."""
    from colmap_amd import fusion
    L = census_lib()
    L.fuo_census(None, 0, 1)
    out = fusion.fuse(options, images, overlapping_images, entry_points=_EntryPoints(mode, L))
    counts = (C.c_uint64 * len(CENSUS_FIELDS))()
    L.fuo_census(counts, len(CENSUS_FIELDS), 1)
    return out, dict(zip(CENSUS_FIELDS, (int(c) for c in counts)))
