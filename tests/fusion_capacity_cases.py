"""Inputs that reach the four capacities of colmap_amd/csrc/fusion.hip AT THEIR PRODUCT VALUES, the table tiers of its walk
kernel and the overlap-list lengths at which the walk changes shape -- each shown to reach its path by the checker alone
(oracle/fusion_oracle.cpp: the extremes of mode 2, or the plan's arithmetic restated here), each compared bit for bit
with the checker's mode 1, twice.

The case functions take a Target: the entry points (`fusion.fuse(..., entry_points=...)`), the library that holds their
development switches and statistics, and how a fresh process gets the same. tests/test_fusion_capacity_gpu.py hands them
the product library on the GPU, tests/test_fusion_capacity_emul.py the CPU stand-in built from the same source at the
same capacities (tests/hip_emul), which also keeps every precondition checked without a GPU (`run=False`: the
precondition alone; `run="once"`: one run of the variant that is sure to reach the path, for the stand-in's slower cases).

Which extreme proves what. A walk treats as masked what is committed and what its own thread has marked in this pass;
marks of other threads read as free (a walk that runs into territory a lower rank of another thread has marked masks
nothing there and goes round until a limit stops it: the deepest stacks of a run belong to such speculative walks, and
they depend on how the waves interleave). A COMMITTED walk has seen the sequential masks on every pixel it looked at, so
every execution of the schedule -- the checker's simulation, the stand-in, the GPU -- repeats it entry for entry:
"deepest_committed_stack > capacity" means the depth-first kernel (COLMAP_AMD_FUSION_WIDE=0, whose stack is the
checker's) MUST cross that capacity. "At most" is asserted where it can be known: with one pool thread there is no
speculation, every walk commits, and the checker's deepest stack is the kernel's. So the two capacities are straddled
with one pool thread, and crossed again with one thread per stripe. The default (breadth-first where exact) runs on the
same inputs: same result, other stack."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np

import fusion_oracle
from colmap_amd import fusion
from pm_common import scene
from switches import switches
from test_fusion import _case, _images, _overlap, _same

_TESTS = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_TESTS)
_CSRC = os.path.join(_ROOT, "colmap_amd", "csrc")


# ---- the product's constants, read from its source ------------------------------------------------------------------

def _int_expr(text, what):
    """`2048`, `(1 << 15)` or `20 * 1024` -- the forms the constants are written in; anything else fails loudly."""
    t = text.strip()
    for pat, f in ((r"\d+", lambda m: int(m.group(0))), (r"\(\s*1\s*<<\s*(\d+)\s*\)", lambda m: 1 << int(m.group(1))),
                   (r"(\d+)\s*\*\s*(\d+)", lambda m: int(m.group(1)) * int(m.group(2)))):
        m = re.fullmatch(pat, t)
        if m:
            return f(m)
    raise AssertionError(f"{what}: cannot read the value {text!r}")


def _capacity(src, name):
    m = re.search(r"#ifndef %s\n#define %s ([^\n]+)\n#endif" % (name, name), src)
    assert m, f"colmap_amd/csrc/fusion.hip: no '#ifndef {name} / #define {name} <value> / #endif' block"
    return _int_expr(m.group(1), name)


def _constant(src, name, where):
    m = re.search(r"\b%s\s*=\s*([^;,]+)[;,]" % name, src)
    assert m, f"{where}: no '{name} = <value>'"
    return _int_expr(m.group(1), name)


_CTYPES = {"float": C.c_float, "int": C.c_int, "long long": C.c_longlong, "const uint8_t*": C.c_void_p}


def _sizeof_dev_image(header):
    """sizeof(DevImage) from the member declarations of fusion_plan.h, laid out by ctypes like the C++ compiler does."""
    m = re.search(r"struct DevImage \{\n(.*?)\n\};", header, re.S)
    assert m, "fusion_plan.h: no 'struct DevImage { ... };'"
    fields = []
    for line in m.group(1).split("\n"):
        decl = line.split("//")[0].strip()
        if not decl:
            continue
        d = re.fullmatch(r"(const uint8_t\*|long long|float|int)\s+([^;]+);", decl)
        assert d, f"fusion_plan.h: DevImage member not understood: {decl!r}"
        for var in d.group(2).split(","):
            v = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", var)
            assert v, f"fusion_plan.h: DevImage member not understood: {decl!r}"
            ct = _CTYPES[d.group(1)]
            fields.append((v.group(1), ct * int(v.group(2)) if v.group(2) else ct))
    return C.sizeof(type("DevImage", (C.Structure,), {"_fields_": fields}))


def _read_constants():
    hip = open(os.path.join(_CSRC, "fusion.hip")).read()
    plan = open(os.path.join(_CSRC, "fusion_plan.h")).read()
    k = dict(kRecordBuf=_capacity(hip, "FUSION_RECORD_BUF"), kStackLds=_capacity(hip, "FUSION_STACK_LDS"),
             kStackSpill=_capacity(hip, "FUSION_STACK_SPILL"), kStage=_capacity(hip, "FUSION_MEDIAN_STAGE"))
    for name in ("kTableBytes", "kWave", "kElemCapMin", "kElemCapMax", "kRowStride"):
        k[name] = _constant(plan, name, "fusion_plan.h")
    k["sizeof_DevImage"] = _sizeof_dev_image(plan)
    return k


K = _read_constants()
kRecordBuf, kStackLds, kStackSpill, kStage = K["kRecordBuf"], K["kStackLds"], K["kStackSpill"], K["kStage"]
kTableBytes, kWave = K["kTableBytes"], K["kWave"]


# ---- make_limits (fusion_plan.h), restated ------------------------------------------------------------------------------

def plan_tier(n, n_overlap):
    desc = n * K["sizeof_DevImage"] + (n + 1) * 4
    return 0 if desc > kTableBytes else (1 if desc + n_overlap * 4 > kTableBytes else 2)


def plan_spill_bound(max_num_pixels, total_pix, max_overlap):
    rec_cap = min(min(max(max_num_pixels, K["kElemCapMin"]), K["kElemCapMax"]), max(total_pix, 1))
    return rec_cap * max_overlap + kWave


def ticks(w, h, num_threads):
    ns = (h + K["kRowStride"] - 1) // K["kRowStride"]
    T = ns if num_threads <= 0 else min(num_threads, ns)
    return (ns + T - 1) // T * K["kRowStride"] * w


# ---- targets ----------------------------------------------------------------------------------------------------------

class Target:
    """entry_points: what fusion.fuse takes (None = the product library); lib: colmap_amd_set_switch / fusion_last_stats;
    child_setup: Python source that defines `target` in a fresh process."""

    def __init__(self, name, entry_points, lib, child_setup):
        self.name, self.entry_points, self.lib, self.child_setup = name, entry_points, lib, child_setup

    def fuse(self, opt, images, overlap):
        return fusion.fuse(opt, images, overlap, entry_points=self.entry_points)

    def rounds(self):
        st = [C.c_int64() for _ in range(4)]
        self.lib.fusion_last_stats(*[C.byref(x) for x in st])
        return st[2].value


def gpu_target():
    from colmap_amd._lib import lib
    return Target("gpu", None, lib(), "target = K.gpu_target()\n")


def emul_target():
    from test_fusion_emul import _EmulEntryPoints
    e = _EmulEntryPoints("libfusion_emul.so")
    return Target("emul", e, e.lib, "target = K.emul_target()\n")


# ---- inputs -----------------------------------------------------------------------------------------------------------

_LOOSE = dict(min_num_pixels=2, max_depth_error=0.05, max_normal_error=30.0)


def noisy(n, w, h, sigma=0.003, seed=1):
    """pm_common.scene with multiplicative depth noise: walks leave the surface patch of their start pixel"""
    images = _images(scene(n, w, h))
    rng = np.random.default_rng(seed)
    for im in images:
        im.depth_map = (im.depth_map * (1 + sigma * rng.standard_normal(im.depth_map.shape))).astype(np.float32)
    return images


_CHECKED = {}   # the checker's side of an input: computed once, shared by the tests that need it, never changed
REPORT = []     # (case, extremes / plan figures, rounds, seconds) of the runs of this process: DESIGN.md's tables


def checked(key, opt, images, overlap):
    """(mode 1 result, extremes of mode 2); mode 2 == mode 1 is asserted, and that both stay under a second"""
    if key not in _CHECKED:
        t0 = time.perf_counter()
        want = fusion_oracle.fuse(opt, images, overlap, mode=1)
        sim, ext = fusion_oracle.fuse_extremes(opt, images, overlap)
        dt = time.perf_counter() - t0
        assert _same(sim, want), key
        assert dt < 1.0, (key, dt)
        _CHECKED[key] = (want, ext)
    return _CHECKED[key]


def _compare(target, case, want, opt, images, overlap, figures, second=True, **sw):
    """fusion.fuse == mode 1 bit for bit (points, normals, colours, visibility), and so is a second run"""
    with switches(target.lib, **sw):
        t0 = time.perf_counter()
        got = target.fuse(opt, images, overlap)
        dt = time.perf_counter() - t0
        rounds = target.rounds()
        assert len(want.xyz) > 0 and _same(got, want), (case, sw, len(got.xyz), len(want.xyz))
        if second:
            assert _same(target.fuse(opt, images, overlap), want), (case, sw, "second run")
    REPORT.append((case, sw, figures, rounds, round(dt, 3)))
    print("capacity case", target.name, case, sw, figures, "rounds", rounds, "seconds %.3f" % dt)
    return rounds


# ---- the stack of a walk: LDS | spill -----------------------------------------------------------------------------------

# One pool thread on 6 x 96 x 72, all-to-all, max_reproj_error 30; max_traversal_depth below | above. The deepest stack of the
# run is 2048 | 2051 entries: the lower run fills the LDS part to its last entry, index 2047, and leaves the spill alone;
# the upper run puts three entries into the spill. (Found by scanning the depth limit with the checker.)
STACK_LDS_CASE = (6, 96, 72, 856, 857)


def case_stack_lds_border(target, side, run=True):
    n, w, h, below, above = STACK_LDS_CASE
    d = below if side == "below" else above
    opt = fusion.StereoFusionOptions(max_reproj_error=30.0, max_traversal_depth=d, max_num_pixels=10000, num_threads=1, **_LOOSE)
    images, overlap = noisy(n, w, h), _overlap(n)
    want, ext = checked(("lds", d), opt, images, overlap)
    assert ext["deepest_stack"] == ext["deepest_committed_stack"], ext   # one thread: no speculation
    if side == "below":
        assert kStackLds - (n - 2) < ext["deepest_stack"] <= kStackLds, ext
    else:
        assert kStackLds < ext["deepest_stack"] <= kStackLds + (n - 2), ext
    if run:
        fig = dict(deepest=ext["deepest_stack"], committed=ext["deepest_committed_stack"])
        _compare(target, f"stack_lds d={d}", want, opt, images, overlap, fig, second=run is True, COLMAP_AMD_FUSION_WIDE=0)
        if run is True:
            _compare(target, f"stack_lds d={d}", want, opt, images, overlap, fig)


# ---- the spill: overflow, growth --------------------------------------------------------------------------------------

# name: (n, w, h, num_threads, max_num_pixels, max_traversal_depth). first = kStackLds + kStackSpill = 18432 entries.
#  T1_below | T1_above: one pool thread on 24 x 64 x 48; the deepest stack of the run is 18426 | 18459 (the closest pair a scan
#     of the depth limit with the checker found: the depth of the deepest walk is not monotone in the limit). The spill
#     bound 2400 * 23 + 64 = 55264 is below 4 * kStackSpill: the one growth of the upper run is clamped by it.
#  clamp: one thread per stripe on 32 x 64 x 48, bound 2000 * 31 + 64 = 62064: the clamped growth with waves in flight.
#  factor4: 24 x 64 x 48 at max_num_pixels 10000 (bound 230064): the first growth is the plain 16384 -> 65536.
#  second: 32 x 64 x 48, a committed stack above kStackLds + 4 * kStackSpill: 16384 -> 65536 -> 262144.
SPILL_CASES = {"T1_below": (24, 64, 48, 1, 2400, 1784), "T1_above": (24, 64, 48, 1, 2400, 1838),
               "clamp": (32, 64, 48, -1, 2000, 8000), "factor4": (24, 64, 48, -1, 10000, 8000),
               "second": (32, 64, 48, -1, 10000, 8000)}


def case_spill(target, name, run=True):
    n, w, h, threads, cap, d = SPILL_CASES[name]
    opt = fusion.StereoFusionOptions(max_reproj_error=30.0, max_traversal_depth=d, max_num_pixels=cap, num_threads=threads,
                                     **_LOOSE)
    images, overlap = noisy(n, w, h), _overlap(n)
    want, ext = checked(("spill", name), opt, images, overlap)
    first, bound = kStackLds + kStackSpill, plan_spill_bound(cap, n * w * h, n - 1)
    deep, committed = ext["deepest_stack"], ext["deepest_committed_stack"]
    assert committed <= kStackLds + bound, (ext, bound)
    if name == "T1_below":
        assert deep == committed and first - 2 * (n - 2) < deep <= first, ext   # deep in the spill, never past it
    elif name == "T1_above":
        assert deep == committed and first < deep <= first + 2 * (n - 2), ext
        assert bound < 4 * kStackSpill, bound
    elif name == "clamp":
        assert first < committed and bound < 4 * kStackSpill, (ext, bound)
    elif name == "factor4":
        assert first < committed and 4 * kStackSpill <= bound, (ext, bound)
    else:
        assert kStackLds + 4 * kStackSpill < committed and 16 * kStackSpill <= bound, (ext, bound)
    if run:
        fig = dict(deepest=deep, committed=committed, spill_bound=bound)
        _compare(target, f"spill {name}", want, opt, images, overlap, fig, second=run is True, COLMAP_AMD_FUSION_WIDE=0)
        if run is True:
            _compare(target, f"spill {name}", want, opt, images, overlap, fig)


# ---- medians: staged | radix select -----------------------------------------------------------------------------------

# max_num_pixels -> input: the largest support of a committed walk equals the cap in each
MEDIAN_CASES = {kStage - 1: (6, 96, 72, 1000), kStage: (6, 96, 72, 1000), kStage + 1: (6, 96, 72, 1000),
                10000: (32, 64, 48, 8000)}


def case_median(target, cap, run=True):
    n, w, h, d = MEDIAN_CASES[cap]
    opt = fusion.StereoFusionOptions(max_reproj_error=30.0, max_traversal_depth=d, max_num_pixels=cap, **_LOOSE)
    images, overlap = noisy(n, w, h), _overlap(n)
    want, ext = checked(("median", cap), opt, images, overlap)
    assert ext["largest_support"] == cap, ext
    if run:
        _compare(target, f"median cap={cap}", want, opt, images, overlap, dict(largest_support=ext["largest_support"]))


# ---- a wave's record buffer full --------------------------------------------------------------------------------------

RECORD_CASE = (4, 128, 96)


def case_record_buffer(target, run=True):
    n, w, h = RECORD_CASE
    opt = fusion.StereoFusionOptions(num_threads=1)   # default thresholds
    images, overlap = _images(scene(n, w, h)), _overlap(n)
    want, ext = checked(("record",), opt, images, overlap)
    assert ext["largest_step_records"] > kRecordBuf, ext
    assert len(want.xyz) > 1000
    if run:
        # one wave, the whole image step in the first window: nothing but the full buffer can cut a pass
        window = ticks(w, h, 1)
        fig = dict(largest_step_records=ext["largest_step_records"])
        rounds = _compare(target, "record buffer", want, opt, images, overlap, fig, second=run is True,
                          COLMAP_AMD_FUSION_WINDOW_FIRST=window)
        assert rounds > n, rounds
        if run is True:
            _compare(target, "record buffer", want, opt, images, overlap, fig)


# ---- table tiers ------------------------------------------------------------------------------------------------------

def _tiny(n):
    return _images(scene(n, 12, 10))


def tier_input(tier):
    if tier == 0:   # 130 images, ring overlap: the descriptors alone exceed the table
        n = 130
        return n, [[(i + d) % n for d in (-2, -1, 1, 2)] for i in range(n)]
    n = 66          # all-to-all: the descriptors fit, the lists do not
    return n, _overlap(n)


def case_planned_tier(target, tier, run=True):
    n, overlap = tier_input(tier)
    assert plan_tier(n, sum(len(v) for v in overlap)) == tier
    assert plan_tier(5, 20) == 2   # what every other fusion test runs
    opt = fusion.StereoFusionOptions(max_reproj_error=3.0, **_LOOSE)
    images = _tiny(n)
    want, ext = checked(("tier", tier), opt, images, overlap)
    assert len(want.xyz) > 100
    if run:
        _compare(target, f"planned tier {tier}", want, opt, images, overlap, dict(tier=tier, n=n))


FORCED_TIER_INPUTS = ("defaults_5x64x48", "sparse_overlap", "mask0")


def forced_tier_child(target, tier):
    """runs in the child process: the switch is set before the library's first fusion run"""
    with switches(target.lib, COLMAP_AMD_FUSION_LDS_TABLES=tier):
        for name in FORCED_TIER_INPUTS:
            opt, images, overlap = _case(name)
            want = fusion_oracle.fuse(opt, images, overlap, mode=1)
            assert len(want.xyz) > 20 and _same(target.fuse(opt, images, overlap), want), name
            assert _same(target.fuse(opt, images, overlap), want), (name, "second run")
    print("forced tier ok", tier)


def case_forced_tier(target, tier):
    """a fresh child process per switch value (started, never exec'd over this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import fusion_capacity_cases as K\n" % (_TESTS, os.path.join(_ROOT, "oracle"), _ROOT)
            + target.child_setup + "K.forced_tier_child(target, %d)\n" % tier)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "forced tier ok %d" % tier in out.stdout, (out.stdout[-1000:], out.stderr[-2000:])


# ---- overlap-list lengths ---------------------------------------------------------------------------------------------

OVERLAP_IMAGES = (33, 34, 64, 65, 66)   # all-to-all: lists of 32 | 33 (breadth-first walks off) and 63 | 64 | 65 (second batch of lanes)


def case_overlap_length(target, n, run=True):
    opt = fusion.StereoFusionOptions(max_reproj_error=3.0, **_LOOSE)
    images, overlap = _tiny(n), _overlap(n)
    want, ext = checked(("overlap", n), opt, images, overlap)
    assert len(want.xyz) > 100
    if n == 34:
        assert max(len(v) for v in overlap) > kWave // 2 >= 33 - 1   # make_limits: wide only up to kWave / 2
    if n == 66:  # the entries past the first 64 of a list matter: without them the result is another
        cut = fusion_oracle.fuse(opt, images, [v[:kWave] for v in overlap], mode=1)
        assert not _same(cut, want)
    if run:
        _compare(target, f"overlap lists of {n - 1}", want, opt, images, overlap, dict(max_overlap=n - 1))
