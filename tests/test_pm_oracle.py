"""CPU tests of the PatchMatch oracle: known answers the reference's own tests hold for
the pieces either side of the kernel, the arithmetic spec, and end-to-end sanity."""
import ctypes as C

import numpy as np
import pytest

from pm_common import scene, oracle_inputs
from colmap_amd import synthetic as syn


def _f(*v):
    return (C.c_float * len(v))(*v)


# ---- known answers from the reference's mvs/image_test.cc ------------------------------

def test_compute_projection_center_identity(pm_oracle):
    # image_test.cc:147-156
    Cc = (C.c_float * 3)()
    pm_oracle.lib().pmo_compute_projection_center(_f(1, 0, 0, 0, 1, 0, 0, 0, 1), _f(1, 2, 3), Cc)
    assert list(Cc) == [-1.0, -2.0, -3.0]


def test_compose_projection_matrix(pm_oracle):
    # image_test.cc:158-169
    P = (C.c_float * 12)()
    pm_oracle.lib().pmo_compose_projection_matrix(_f(2, 0, 0, 0, 2, 0, 0, 0, 1), _f(0, 1, 0, 1, 0, 0, 0, 0, 1),
                                                  _f(1, 2, 3), P)
    assert list(P) == [0, 2, 0, 2, 2, 0, 0, 4, 0, 0, 1, 3]


def test_rotate_pose(pm_oracle):
    # image_test.cc:171-209
    R = _f(1, 0, 0, 0, 1, 0, 0, 0, 1)
    T = _f(1, 2, 3)
    pm_oracle.lib().pmo_rotate_pose(_f(1, 0, 0, 0, 1, 0, 0, 0, 1), R, T)
    assert list(R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(T) == [1, 2, 3]
    R = _f(1, 0, 0, 0, 1, 0, 0, 0, 1)
    T = _f(1, 0, 0)
    pm_oracle.lib().pmo_rotate_pose(_f(0, -1, 0, 1, 0, 0, 0, 0, 1), R, T)
    assert list(R) == [0, -1, 0, 1, 0, 0, 0, 0, 1] and list(T) == [0, 1, 0]


def test_inverse_projection_matrix(pm_oracle):
    rng = np.random.default_rng(0)
    K = np.array([[500, 0, 320], [0, 510, 240], [0, 0, 1]], np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R = (q * np.sign(np.linalg.det(q))).astype(np.float32)
    T = rng.normal(size=3).astype(np.float32)
    out = (C.c_float * 12)()
    pm_oracle.lib().pmo_compose_inverse_projection_matrix(_f(*K.ravel()), _f(*R.ravel()), _f(*T), out)
    P = np.eye(4)
    P[:3] = K.astype(np.float64) @ np.concatenate([R, T[:, None]], 1).astype(np.float64)
    np.testing.assert_allclose(np.array(out).reshape(3, 4), np.linalg.inv(P)[:3], rtol=2e-4, atol=2e-5)


def test_rotate_matches_gpu_mat_test(pm_oracle):
    # expectation of TestRotateImage, reference mvs/gpu_mat_test.cu:151-186
    for (w, h, d) in [(20, 40, 1), (60, 20, 3), (40, 40, 2)]:
        a = np.random.default_rng(1).uniform(0, 100, (d, h, w)).astype(np.float32)
        out = np.zeros((d, w, h), np.float32)
        pm_oracle.lib().pmo_rotate_f32(a.ctypes.data_as(C.c_void_p), w, h, d, out.ctypes.data_as(C.c_void_p))
        ch, cv, ang = w / 2.0 - 0.5, h / 2.0 - 0.5, -np.pi / 2
        for r in range(h):
            for c in range(w):
                rotc = int(round(np.cos(ang) * (c - ch) - np.sin(ang) * (r - cv) + cv))
                rotr = int(round(np.sin(ang) * (c - ch) + np.cos(ang) * (r - cv) + ch))
                assert np.array_equal(a[:, r, c], out[:, rotr, rotc])


# ---- arithmetic spec -------------------------------------------------------------------

def test_exp_polynomial(pm_oracle):
    x = np.concatenate([np.linspace(-87, 2, 4001), [-1e-8, 0.0, -100.0, -87.5]]).astype(np.float32)
    y = pm_oracle.exp_f32(x)
    ref = np.exp(x.astype(np.float64))
    ok = x >= -87
    assert np.max(np.abs(y[ok] - ref[ok]) / ref[ok]) < 2.5e-7
    assert np.all(y[~ok] == 0)


def test_sincos_polynomial(pm_oracle):
    a = np.linspace(-7, 7, 5001).astype(np.float32)
    s, c = pm_oracle.sincos_f32(a)
    assert np.max(np.abs(s - np.sin(a.astype(np.float64)))) < 3e-7
    assert np.max(np.abs(c - np.cos(a.astype(np.float64)))) < 3e-7


def test_xorwow_stream(pm_oracle):
    """Generator recurrence + rocRAND seeding (rocrand_xorwow.h), independent numpy restatement."""
    def stream(seed, n):
        M = 0xFFFFFFFF
        x = [123456789, 362436069, 521288629, 88675123, 5783321]
        d = 6615241
        s0 = (seed & M) ^ 0x2c7f967f
        s1 = (seed >> 32) ^ 0xa03697cb
        t0 = (1228688033 * s0) & M
        t1 = (2073658381 * s1) & M
        x[0] = (x[0] + t0) & M; x[1] ^= t0; x[2] = (x[2] + t1) & M; x[3] ^= t1; x[4] = (x[4] + t0) & M
        d = (d + t1 + t0) & M
        out = []
        for _ in range(n):
            t = x[0] ^ (x[0] >> 2)
            x = x[1:] + [((x[4] ^ (x[4] << 4)) ^ (t ^ (t << 1))) & M]
            d = (d + 362437) & M
            out.append((d + x[4]) & M)
        return np.array(out, np.uint32)
    for seed in (0, 1, 511, 123456, 2**33 + 5):
        raw, uni = pm_oracle.rng_stream(seed, 64)
        assert np.array_equal(raw, stream(seed, 64))
        expect = np.float32(2.3283064e-10) + raw.astype(np.float32) * np.float32(2.3283064e-10)
        assert np.array_equal(uni, expect.astype(np.float32))
        assert np.all(uni > 0) and np.all(uni <= 1)


def _pin_seeds():
    """Sequence ids as InitRandomStateKernel produces them (small), 32-bit boundary cases and random
    64-bit values (both halves of the seed enter rocRAND's scrambling)."""
    return np.concatenate([np.arange(0, 600, dtype=np.uint64),
                           np.array([2**32 - 1, 2**32, 2**32 + 5, 2**40 + 123, 2**63 + 17, 2**64 - 1], np.uint64),
                           np.random.default_rng(0).integers(0, 2**63, 400).astype(np.uint64)])


def rocrand_pin_lib():
    import ctypes as C, os, subprocess
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip")
    path = os.path.join(d, "librocrand_pin.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(os.path.join(d, "rocrand_pin.hip")):
        subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL)
    return C.CDLL(path)


def test_xorwow_equals_rocrand_host_engine(pm_oracle):
    """The oracle's generator against rocRAND itself -- rocrand_init(seed, 0, 0) + rocrand_uniform on
    rocrand_state_xorwow, what curand_init / curand_uniform (gpu_mat_prng.cu:36-48) resolve to in the
    reference's own HIP build -- through rocRAND's host path (tests/hip/rocrand_pin.hip), bit for bit."""
    import ctypes as C
    seeds, nd = _pin_seeds(), 40
    want = np.zeros((len(seeds), nd), np.float32)
    rocrand_pin_lib().rocrand_pin_host(seeds.ctypes.data_as(C.c_void_p), len(seeds), nd,
                                       want.ctypes.data_as(C.c_void_p))
    got = np.stack([pm_oracle.rng_stream(int(sd), nd)[1] for sd in seeds])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(want > 0) and np.all(want <= 1)


def test_texel_requantisation_is_identity():
    """FilterKernel re-quantises the reference image as uint8(255 * (b/255)) (reference
    gpu_mat_ref_image.cu:77); with correctly rounded b/255 this maps every byte to itself."""
    b = np.arange(256, dtype=np.float32)
    t = (b / np.float32(255.0)).astype(np.float32)
    assert np.array_equal((np.float32(255.0) * t).astype(np.uint8), np.arange(256))


# ---- algorithm-level sanity ---------------------------------------------------------------

def test_ref_filter_matches_numpy(pm_oracle):
    v = scene()[2]
    img, s, ss = pm_oracle.filter_ref_image(v.gray, 3, 1, 3.0, 0.2)
    assert np.array_equal(img, v.gray)
    g = np.pad(v.gray.astype(np.float64) / 255.0, 3)
    H, W = v.gray.shape
    r, c = 17, 29
    acc = np.zeros(3)
    for dr in range(-3, 4):
        for dc in range(-3, 4):
            col = g[r + 3 + dr, c + 3 + dc]
            w = np.exp(-(dr * dr + dc * dc) / (2 * 9.0) - (g[r + 3, c + 3] - col) ** 2 / (2 * 0.04))
            acc += [w * col, w * col * col, w]
    assert abs(s[r, c] - acc[0] / acc[2]) < 1e-5 and abs(ss[r, c] - acc[1] / acc[2]) < 1e-5


def test_memoised_equals_plain(pm_oracle):
    """Caching bit-identical NCC values / bilateral weights inside a row step (what the
    HIP kernel does) does not change a single bit of the result."""
    views = scene(4, 64, 48)
    imgs = oracle_inputs(views)
    dmin, dmax = syn.depth_range(views, 1)
    outs = []
    for memo in (0, 1):
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=1,
                                      num_iterations=1, memoize=memo)
        outs.append(pm_oracle.run(o, imgs, 1, [0, 2, 3], want_cost=True))
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_device_order_vs_reference_order(pm_oracle):
    """order=1 (taps dealt to 16 lanes + fixed tree sum + per-tap direct homography: what
    the HIP kernel evaluates, bit for bit) against order=0 (the reference's sequential
    order, patch_match_cuda.cu:503-569). Same mathematics, different rounding:
    tolerance 5e-4 absolute on the NCC cost in [0, 2] (observed max 1.5e-4, mean 5e-6),
    and the full solves must be statistically equivalent against ground truth."""
    views = scene(5, 128, 96)
    imgs = oracle_inputs(views)
    dmin, dmax = syn.depth_range(views, 2)
    res = {}
    for order in (0, 1):
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0,
                                      order=order, max_sweeps=0)
        res[order] = pm_oracle.run(o, imgs, 2, [0, 1, 3, 4], want_cost=True)
    assert np.array_equal(res[0]["depth"], res[1]["depth"])  # same PRNG initialisation
    d = np.abs(res[0]["cost"] - res[1]["cost"])
    assert d.max() < 5e-4 and d.mean() < 2e-5
    gt = views[2].depth
    frac = {}
    for order in (0, 1):
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0,
                                      order=order)
        r = pm_oracle.run(o, imgs, 2, [0, 1, 3, 4])
        rel = np.abs(r["depth"] - gt) / gt
        frac[order] = ((rel < 0.01).mean(), np.median(rel))
    assert abs(frac[0][0] - frac[1][0]) < 0.03      # same fraction of pixels within 1 %
    assert abs(frac[0][1] - frac[1][1]) < 1e-3      # same median relative depth error


def test_device_order_is_closer_to_a_double_evaluation_than_the_reference_order(pm_oracle):
    """Why the HIP kernel's ComputeInitialCost sits further from the reference build than the oracle in the
    reference's order does (2.1e-4 / 3.4e-6 against 8.8e-5 / 8.9e-7): the two orders are two roundings of
    the same sums, and measured against the same cost with every intermediate in double (PMO_DEVICE_MIX bit 16) the
    DEVICE order is the more accurate one -- the reference's running-sum coordinates and its 121-term sequential sums
    carry the larger error. Reverting the four ingredients of the device order one by one reproduces order 0 bit for
    bit (scripts/pm_order_decomposition.py, profiles/r04_pm_initial_cost_decomposition.json)."""
    views = scene()
    imgs = oracle_inputs(views)
    dmin, dmax = syn.depth_range(views, 2)
    L = pm_oracle.lib()

    def init_cost(order, mix):
        L.pmo_set_device_mix(C.c_int(mix))
        try:
            o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0, order=order,
                                          max_sweeps=0)
            return pm_oracle.run(o, imgs, 2, [0, 1, 3, 4], want_cost=True)["cost"].astype(np.float64)
        finally:
            L.pmo_set_device_mix(C.c_int(0))

    ref_order, dev_order, exact = init_cost(0, 0), init_cost(1, 0), init_cost(1, 16)
    assert np.array_equal(init_cost(1, 15), ref_order)          # all four ingredients reverted = the reference's order
    sel = (exact > 0.0) & (exact < 2.0)
    e_ref, e_dev = np.abs(ref_order - exact)[sel], np.abs(dev_order - exact)[sel]
    assert e_dev.mean() < 0.5 * e_ref.mean() and e_dev.max() < 0.5 * e_ref.max(), (e_dev.mean(), e_ref.mean(), e_dev.max(), e_ref.max())
    assert e_dev.max() < 1e-4 and e_dev.mean() < 2e-6           # SURVEY.md section 7's slice asked for <= 1e-4
    # the largest single differences between the two orders come from the summation order
    only_sums_device = np.abs(init_cost(1, 14) - ref_order)
    sums_reverted = np.abs(init_cost(1, 1) - ref_order)
    assert sums_reverted.max() < 0.6 * np.abs(dev_order - ref_order).max() < 1.2 * only_sums_device.max()


def test_device_order_vs_reference_order_s20_m15(pm_oracle):
    """The same bridge at BASELINE's view / sample counts (S = 20 sources, M = 15 samples, 96 x 72):
    initial costs within 5e-4, and the full 5 x 4-sweep photometric + filter solves statistically
    equivalent (kept fraction, accuracy against ground truth, pixel-wise agreement)."""
    views = scene(22, 96, 72, 3.6 * 21)
    ref = 10
    src = [i for i in range(21) if i != ref]
    imgs = oracle_inputs(views)
    dmin, dmax = syn.depth_range(views, ref)
    res = {}
    for order in (0, 1):
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0,
                                      order=order, max_sweeps=0)
        res[order] = pm_oracle.run(o, imgs, ref, src, want_cost=True)
    d = np.abs(res[0]["cost"] - res[1]["cost"])
    assert d.max() < 5e-4 and d.mean() < 2e-5
    gt = views[ref].depth
    out = {}
    for order in (0, 1):
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=1, order=order)
        out[order] = pm_oracle.run(o, imgs, ref, src)["depth"]
    kept = [(out[k] > 0) for k in (0, 1)]
    assert abs(kept[0].mean() - kept[1].mean()) < 0.02
    assert (kept[0] == kept[1]).mean() > 0.95
    both = kept[0] & kept[1]
    rel = np.abs(out[0][both] - out[1][both]) / out[0][both]
    # 96 x 72 images (f = 90 px) resolve depth to ~1 % at best (60 % of either solve is within 1 % of
    # ground truth), so pixel-wise agreement is bounded by that: observed 0.84 / 0.96 at 1 % / 5 %
    assert (rel < 1e-2).mean() > 0.80 and (rel < 5e-2).mean() > 0.93
    err = [np.abs(out[k][kept[k]] - gt[kept[k]]) / gt[kept[k]] for k in (0, 1)]
    assert abs(np.median(err[0]) - np.median(err[1])) < 5e-4          # observed 5.04e-3 vs 5.17e-3
    assert abs((err[0] < 0.01).mean() - (err[1] < 0.01).mean()) < 0.02  # observed 0.602 vs 0.599


def test_device_order_vs_reference_order_full_resolution_crop(pm_oracle):
    """bench.py's cpu_baseline problem shape (a crop of a 2560 x 1920 reference image against S = 20
    full-resolution sources: packed 2563 x 1923 footprints, large pixel coordinates in the
    homographies): ComputeInitialCost in both orders. Pixel coordinates of ~1300 carry 1.2e-4 px of
    fp32 rounding per operation, and the reference's incremental stepping accumulates it over the 11
    taps of a row where the device order evaluates every tap directly: the bound is 2e-3 here (observed
    max 1.1e-3, mean 3.2e-5) against 5e-4 on the small scenes. (128 x 96 crop: the CPU suite has to
    stay in minutes; the sweeps of this shape are compared on the GPU box.)"""
    W, H, S, cw, ch = 2560, 1920, 20, 128, 96
    views = syn.make_scene(S + 1, W, H, arc_deg=3.6 * S)
    ref = S // 2
    src = [i for i in range(S + 1) if i != ref]
    x0, y0 = (W - cw) // 2, (H - ch) // 2
    v = views[ref]
    K = v.K.copy()
    K[0, 2] -= x0
    K[1, 2] -= y0
    imgs = oracle_inputs(views)
    imgs[ref] = dict(K=K, R=v.R, T=v.T, gray=np.ascontiguousarray(v.gray[y0:y0 + ch, x0:x0 + cw]))
    dmin, dmax = float(v.depth.min() * 0.9), float(v.depth.max() * 1.1)
    res = {}
    for order in (0, 1):
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0,
                                      order=order, max_sweeps=0)
        res[order] = pm_oracle.run(o, imgs, ref, src, want_cost=True)
    d = np.abs(res[0]["cost"] - res[1]["cost"])
    assert d.max() < 2e-3 and d.mean() < 6e-5, (d.max(), d.mean())


# ---- degenerate inputs (tests/pm_edge_cases.py) ----

def _edge_oracle_run(pm_oracle, name, census=False, **kw):
    import pm_edge_cases as E
    p = E.build(name)
    opt = {k: v for k, v in p.options.items() if k not in ("columns_per_group", "threads_per_group")}
    opt.update(kw)
    o = pm_oracle.default_options(depth_min=p.depth_range[0], depth_max=p.depth_range[1], **opt)
    run = pm_oracle.run_census if census else pm_oracle.run
    return run(o, oracle_inputs(p.views, p.maps is not None, p.maps), p.ref, p.src, want_cost=True)


def _edge_case_names():
    import pm_edge_cases as E
    return list(E.CASES)


@pytest.mark.parametrize("name", _edge_case_names())
def test_edge_case_reaches_the_paths_it_is_named_for(pm_oracle, name):
    """The census build (pm_oracle.c: PMO_CENSUS) counts, for the oracle's device-order solve of the case, how often the
    paths the case exists for were taken: every counter the case names clears its floor (a bit-exact pass on a case
    that never leaves the happy path would prove nothing). The census build returns the plain build's bits."""
    import pm_edge_cases as E
    out, counts = _edge_oracle_run(pm_oracle, name, census=True, order=1)
    print(name, {k: v for k, v in counts.items() if v})
    for counter, floor in E.CASES[name].counters.items():
        assert counts[counter] >= floor, (counter, counts[counter], floor)
    E.assert_same_bits(_edge_oracle_run(pm_oracle, name, order=1), out)


def test_census_covers_every_counter(pm_oracle):
    """Every counter of the census is named, with a floor, by at least one case of the table: none is dead under it."""
    import pm_edge_cases as E
    named = set().union(*(c.counters for c in E.CASES.values()))
    assert named <= set(pm_oracle.CENSUS_FIELDS)
    informational = {"taps", "ncc_evals"}       # the denominators
    assert set(pm_oracle.CENSUS_FIELDS) - named <= informational, set(pm_oracle.CENSUS_FIELDS) - named - informational


@pytest.mark.parametrize("name", _edge_case_names())
def test_edge_case_device_order_vs_reference_order(pm_oracle, name):
    """order=1 against order=0 on ComputeInitialCost of the degenerate cases (max_sweeps = 0: the geometric cases
    contribute their start maps -- salted or scaled normals -- but not the source depth maps, which only a sweep
    reads), with the bounds of test_device_order_vs_reference_order: same PRNG initialisation, no NaN in either cost
    map, mean difference below 2e-5. The two orders round the same weighted sums (values within [0, 1]) differently,
    by about 1e-7 in the covariance; the cost divides that by sqrt(var_ref var_src), and the cut-off keeps both
    variances at or above 1e-5: no single cost may differ by more than 1e-7 / 1e-5 = 1e-2, wherever the patch lies.
    The 5e-4 of the benign test holds for variances well above the cut-off; next to it -- the rim of a flat block, a
    window that is mostly border -- larger differences, and entries where the two orders fall on different sides
    of the cut-off and one of them reads 2.0 (left out of the cap), stay below 1 % of the entries each."""
    r = {order: _edge_oracle_run(pm_oracle, name, order=order, filter=0, max_sweeps=0) for order in (0, 1)}
    for k in ("depth", "normal"):
        assert np.array_equal(r[0][k].view(np.uint32), r[1][k].view(np.uint32)), k
    a, b = r[0]["cost"], r[1]["cost"]
    assert not np.isnan(a).any() and not np.isnan(b).any()
    flip = (a == 2.0) != (b == 2.0)
    d = np.abs(a - b)[~flip]
    print(name, "flips", flip.mean(), "beyond 5e-4", (d >= 5e-4).mean(), "max", d.max(), "mean", d.mean())
    assert d.mean() < 2e-5 and d.max() < 1e-2
    assert (d >= 5e-4).mean() < 0.01 and flip.mean() < 0.01


def test_thread_count_does_not_change_result(pm_oracle):
    views = scene(4, 64, 48)
    imgs = oracle_inputs(views)
    dmin, dmax = syn.depth_range(views, 1)
    outs = []
    for nt in (1, 3):
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0,
                                      num_iterations=1, num_threads=nt)
        outs.append(pm_oracle.run(o, imgs, 1, [0, 2, 3]))
    assert np.array_equal(outs[0]["depth"], outs[1]["depth"])


def test_recovers_ground_truth_depth(pm_oracle):
    views = scene(5, 128, 96)
    imgs = oracle_inputs(views)
    dmin, dmax = syn.depth_range(views, 2)
    o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0)
    out = pm_oracle.run(o, imgs, 2, [0, 1, 3, 4])
    gt = views[2].depth
    rel = np.abs(out["depth"] - gt) / gt
    assert np.median(rel) < 0.01
    assert (rel < 0.05).mean() > 0.8
    nrm = np.linalg.norm(out["normal"], axis=0)
    np.testing.assert_allclose(nrm, 1.0, atol=1e-4)


def test_geometric_pass_and_filter(pm_oracle):
    """Two-pass flow of PatchMatchController::Run (reference patch_match.cc:183-204):
    photometric without filtering for every image, then geometric + filter."""
    views = scene(3, 64, 48)
    imgs = oracle_inputs(views)
    maps = []
    for ref in range(3):
        dmin, dmax = syn.depth_range(views, ref)
        o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=0, filter=0,
                                      num_iterations=2)
        r = pm_oracle.run(o, imgs, ref, [i for i in range(3) if i != ref])
        maps.append((r["depth"], r["normal"]))
    imgs2 = oracle_inputs(views, True, maps)
    dmin, dmax = syn.depth_range(views, 1)
    o = pm_oracle.default_options(depth_min=dmin, depth_max=dmax, geom_consistency=1, filter=1,
                                  num_iterations=2)
    r = pm_oracle.run(o, imgs2, 1, [0, 2])
    kept = r["depth"] > 0
    assert 0.2 < kept.mean() <= 1.0
    # filtered pixels: depth, normal and mask all zero (reference :1267-1275)
    assert np.all(r["normal"][:, ~kept] == 0) and np.all(r["mask"][:, ~kept] == 0)
    # kept pixels have >= filter_min_num_consistent consistent views
    assert np.all(r["mask"][:, kept].sum(0) >= 2)
    gt = views[1].depth
    rel = np.abs(r["depth"][kept] - gt[kept]) / gt[kept]
    assert np.median(rel) < 0.03  # 64x48 images, two iterations


def test_problem_checks(pm_oracle):
    views = scene(3, 64, 48)
    imgs = oracle_inputs(views)
    o = pm_oracle.default_options(depth_min=1, depth_max=10, geom_consistency=0, filter=0)
    with pytest.raises(RuntimeError):
        pm_oracle.run(o, imgs, 1, [1, 2])  # reference image as source (patch_match.cc:87-91)
    with pytest.raises(RuntimeError):
        pm_oracle.run(o, imgs, 1, [0, 0])  # duplicates
    with pytest.raises(RuntimeError):
        pm_oracle.run(o, imgs, 1, [])      # no sources (:85)
