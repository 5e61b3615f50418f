"""The exact-tier kernels of colmap_amd/csrc/ba_schur_explicit.hip called directly through the internal C++ interface
(ba_schur_explicit.h: mangled names) and compared with plain numpy references: the explicit formation of the reduced
camera system (point-major and pair-major, fixed point and fp64), the prior rows and the LM diagonal, the blocked
Cholesky with its solve and its two-stream lookahead, the triangular inverse and the covariance blocks.

The case functions are shared: tests/test_ba_explicit_gpu.py runs them on the hipcc build with device buffers
(TorchBuffers), tests/test_ba_emul.py on the CPU stand-in build of the same sources (HostBuffers). A case takes an
adaptor with
    to_device(ndarray) -> object with .ptr        to_host(object) -> ndarray (synchronises first)
    lookahead() -> (st2, ev_panel, ev_u2)         a second stream and two events for Workspace, as integers
    api                                           the entry points of the library under test
`st` is always the null stream. FormArgs::pairs stays a host pointer to a host PairLists. No input makes the library
throw (BAX_HIP, the record-buffer check): ctypes cannot carry a C++ exception.

Every bar below comes from the reference or from the number formats, never from what the kernels return:
eps = 2^-53 is the unit roundoff of fp64, gamma_k = k eps / (1 - k eps)."""
import ctypes as C
import functools
import subprocess

import numpy as np

EPS = 2.0 ** -53
LD = np.longdouble
QUANTUM = 2.0 ** -60  # one unit of the fixed-point accumulators
COV_SLOT = 256        # ba_explicit::kCovSlot


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


# ------------------------------------------------------------------------------------------------
# ctypes mirrors of ba_schur_explicit.h (field order and types as declared there; natural alignment)
# ------------------------------------------------------------------------------------------------

class FormArgs(C.Structure):
    _fields_ = [("n_obs", C.c_int), ("n_points", C.c_int), ("n_c", C.c_int), ("n_poses", C.c_int), ("kd", C.c_int)] + \
               [(n, C.c_void_p) for n in ("Jpose", "Jcam", "Jsens", "Jpt", "Cinv", "a2c", "pt_ptr", "pt_off", "a_pose", "a_cam",
                                          "a_pt", "pairs", "a_sensor", "pose_off", "pose_dim", "cam_off", "cam_dim", "sens_off")] + \
               [("fixed_point", C.c_bool), ("bad", C.c_void_p)]


class Workspace(C.Structure):
    _fields_ = [("Linv", C.c_void_p), ("tmp", C.c_void_p), ("info", C.c_void_p), ("st2", C.c_void_p),
                ("ev_panel", C.c_void_p), ("ev_u2", C.c_void_p), ("min_rows128", C.c_int)]


class PairLists(C.Structure):
    _fields_ = [("inc", C.c_void_p), ("n_inc", C.c_longlong), ("rec", C.c_void_p), ("rec_doubles", C.c_size_t)]


class CovPair(C.Structure):
    _fields_ = [("a0", C.c_int), ("da", C.c_int), ("b0", C.c_int), ("db", C.c_int)]


assert C.sizeof(FormArgs) == 24 + 18 * 8 + 8 + 8 and FormArgs.Jpose.offset == 24 and FormArgs.bad.offset == 176
assert C.sizeof(Workspace) == 56 and Workspace.min_rows128.offset == 48
assert C.sizeof(PairLists) == 32 and C.sizeof(CovPair) == 16


class _Api:
    pass


@functools.lru_cache(maxsize=None)
def _entry_points(path):
    L = C.CDLL(path)
    names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.split()
    api = _Api()
    for attr, key in (("form", "ba_explicit4formE"), ("finish", "ba_explicit6finishE"),
                      ("factor_solve", "ba_explicit12factor_solveE"), ("build_pair_lists", "ba_explicit16build_pair_listsE"),
                      ("free_pair_lists", "ba_explicit15free_pair_listsE"), ("tri_inverse", "ba_explicit11tri_inverseE"),
                      ("extract_cov_blocks", "ba_explicit18extract_cov_blocksE"),
                      ("add_prior_rows", "ba_explicit14add_prior_rowsE"), ("add_lm_diagonal", "ba_explicit15add_lm_diagonalE")):
        found = [n for n in names if key in n]
        assert len(found) == 1, (key, found)
        fn = getattr(L, found[0])
        fn.restype = None
        setattr(api, attr, fn)
    api.build_pair_lists.restype = C.c_bool
    api.lib = L
    return api


def entry_points(lib):
    """The ba_explicit:: functions of a loaded library (a ctypes.CDLL), looked up by their mangled names."""
    return _entry_points(lib._name)


# ------------------------------------------------------------------------------------------------
# buffer adaptors
# ------------------------------------------------------------------------------------------------

class _HostBuf:
    def __init__(self, arr):
        self.arr = arr
        self.ptr = arr.ctypes.data


class HostBuffers:
    """The stand-in: device memory is host memory. Its streams are synchronous and its events are small host objects
    (struct { double t; }): the lookahead call order runs with a dummy stream and two such events."""

    def __init__(self, lib):
        self.api = entry_points(lib)
        self._keep = []

    def to_device(self, a):
        return _HostBuf(np.array(a, order="C", copy=True))

    def to_host(self, b):
        return b.arr.copy()

    def lookahead(self):
        objs = [np.zeros(1) for _ in range(3)]
        self._keep.append(objs)
        return tuple(o.ctypes.data for o in objs)


class _TorchBuf:
    def __init__(self, t):
        self.t = t
        self.ptr = t.data_ptr()


class TorchBuffers:
    """The hipcc build: torch CUDA tensors, as colmap_amd.mvs hands them to the library."""

    def __init__(self, lib):
        import torch
        self.torch = torch
        self.api = entry_points(lib)
        self._keep = []
        # torch brings its own copy of the HIP runtime and asks for it by file name; the library asks for the runtime by
        # soname and shares torch's copy only when torch was loaded FIRST. Loaded the other way round, the process holds two
        # runtimes, torch's pointers mean nothing to the library's, and its first call throws through ctypes: say so here.
        with open("/proc/self/maps") as f:
            runtimes = {line.split()[-1] for line in f if "libamdhip64" in line}
        if len(runtimes) > 1:
            raise RuntimeError(f"two HIP runtimes in one process {sorted(runtimes)}: import torch before the library is loaded")

    def to_device(self, a):
        return _TorchBuf(self.torch.from_numpy(np.array(a, order="C", copy=True)).cuda())

    def to_host(self, b):
        self.torch.cuda.synchronize()
        return b.t.cpu().numpy()

    def lookahead(self):
        torch = self.torch
        st2 = torch.cuda.Stream()
        evs = [torch.cuda.Event(), torch.cuda.Event()]
        for e in evs:  # (a torch event has a handle once it has been recorded)
            e.record()
        torch.cuda.synchronize()
        self._keep.append((st2, evs))
        return st2.cuda_stream, evs[0].cuda_event, evs[1].cuda_event


def _p(buf):
    return C.c_void_p(buf.ptr if buf is not None else None)


# ------------------------------------------------------------------------------------------------
# formation
# ------------------------------------------------------------------------------------------------

LONG_TRACKS = (1, 2, 15, 16, 17, 33)  # around form_kernel's chunk of 16 staged observations: one, two and three chunks


@functools.lru_cache(maxsize=None)
def formation_problem(seed, n_poses, n_points, shared_cams, rigs, kd=4, long_tracks=False):
    """A random linearisation in the layouts FormArgs describes (c-order planes, p-order point columns, p-order
    topology) with constant poses / cameras / sensors / points, 5-wide pose blocks, optionally cameras shared between
    images and rig frames (several images per pose block, each with its own sensor_from_rig block).

    long_tracks = False: tracks of 1-7 observations in distinct images, 2 or 3 refined intrinsics (kd = 4).
    long_tracks = True: track lengths from LONG_TRACKS (a pose block may then carry several observations of a point),
    a constant point with a 17-long and one with a 33-long track, cam_dim from {0, 1, kd - 1, kd}, and one observation
    with every column: a 6-wide pose, kd intrinsics and (with rigs) a variable sensor.

    Returns the arrays and, in longdouble, `want` = S, and per entry `T` = the number of terms
    J_a[:, i]^T (delta_ab I - E_a C^-1 E_b^T) J_b[:, k] that land on it and `A` = the sum of their absolute values.
    (Cached: the tests share one reference per problem and leave it unchanged.)"""
    rng = np.random.default_rng(seed)
    n_cams = (5 if long_tracks else 2) if shared_cams else n_poses
    n_sens = 3 if rigs else 0
    obs = []  # (point, pose, cam, sensor)
    forced = {}
    if long_tracks:
        forced = {1: 17, 2: 33, 3: 16, 4: 15, 5: 1, 6: 2, 7: 33, 8: 17}
    for j in range(n_points):
        if long_tracks:
            t = forced.get(j, int(LONG_TRACKS[int(rng.integers(len(LONG_TRACKS)))]))
            images = [(int(rng.integers(n_poses)), int(rng.integers(n_sens)) if rigs else -1) for _ in range(t)]
            if j == 0:
                images[0] = (0, 0 if rigs else -1)
            images.sort()
        else:
            t = int(rng.integers(1, 8))
            images = set()
            while len(images) < t:
                pose = int(rng.integers(n_poses))
                sens = int(rng.integers(n_sens)) if rigs else -1
                images.add((pose, sens))
            images = sorted(images)
        for pose, sens in images:
            obs.append((j, pose, pose % n_cams, sens))
    N = len(obs)
    perm = rng.permutation(N)  # p-order slot a -> c-order slot
    off = 0
    pose_off, pose_dim = [], []
    for i in range(n_poses):
        d = [6, 6, 6, 5, 0][int(rng.integers(5))]
        if long_tracks and i == 0:
            d = 6
        pose_dim.append(d); pose_off.append(off if d else -1); off += d
    cam_off, cam_dim = [], []
    for i in range(n_cams):
        d = [0, 1, kd - 1, kd][int(rng.integers(4))] if long_tracks else [2, 3, 0][int(rng.integers(3))]
        if long_tracks and i == 0:
            d = kd
        cam_dim.append(d); cam_off.append(off if d else -1); off += d
    sens_off = []
    for i in range(n_sens):
        v = bool(rng.integers(2)) or (long_tracks and i == 0)
        sens_off.append(off if v else -1); off += 6 if v else 0
    n_c = off
    pt_off = [(-1 if rng.integers(5) == 0 else 3 * j) for j in range(n_points)]
    if long_tracks:
        pt_off[0] = 0
        pt_off[1] = pt_off[2] = -1  # the constant points with a 17-long and a 33-long track
        pt_off[7] = 21
    scale = 0.08
    Jpose, Jcam, Jsens = (scale * rng.uniform(-1, 1, (12, N)) for _ in range(3))
    Jcam = scale * rng.uniform(-1, 1, (2 * kd, N))
    Jpt = scale * rng.uniform(-1, 1, (6, N))
    pt_ptr = np.zeros(n_points + 1, np.int32)
    for j, *_ in obs:
        pt_ptr[j + 1] += 1
    pt_ptr = np.cumsum(pt_ptr).astype(np.int32)
    Cinv = np.zeros((n_points, 9))
    wmax = 6 + kd + (6 if rigs else 0)
    want, A, T = np.zeros(n_c * n_c, LD), np.zeros(n_c * n_c, LD), np.zeros(n_c * n_c, np.int64)
    widest = 0
    for j in range(n_points):
        sl = range(pt_ptr[j], pt_ptr[j + 1])
        t = len(sl)
        E = np.stack([Jpt[:, a].reshape(2, 3) for a in sl])                        # [t][2][3]
        Ci = np.linalg.inv(sum(e.T @ e for e in E) + 0.01 * np.eye(3))
        Cinv[j] = Ci.reshape(9)
        J, idx = np.zeros((t, 2, wmax), LD), np.full((t, wmax), -1, np.int64)      # camera-side columns, tangent indices
        for q, a in enumerate(sl):
            _, pose, cam, sens = obs[a]
            c, w = perm[a], 0
            if pose_off[pose] >= 0:
                for d in range(pose_dim[pose]):
                    J[q, :, w] = Jpose[d, c], Jpose[6 + d, c]; idx[q, w] = pose_off[pose] + d; w += 1
            if cam_off[cam] >= 0:
                for d in range(cam_dim[cam]):
                    J[q, :, w] = Jcam[d, c], Jcam[kd + d, c]; idx[q, w] = cam_off[cam] + d; w += 1
            if sens >= 0 and sens_off[sens] >= 0:
                for d in range(6):
                    J[q, :, w] = Jsens[d, c], Jsens[6 + d, c]; idx[q, w] = sens_off[sens] + d; w += 1
            widest = max(widest, w)
        M = np.zeros((t, t, 2, 2), LD)
        M[np.arange(t), np.arange(t)] = np.eye(2)
        if pt_off[j] >= 0:
            El = E.astype(LD)
            M -= np.einsum("aum,mn,bvn->abuv", El, Ci.astype(LD), El)
            pair = np.ones((t, t), bool)
        else:
            pair = np.eye(t, dtype=bool)  # a constant point couples nothing: only J_a^T J_a
        terms = np.einsum("aui,abuv,bvk->abik", J, M, J)                           # [a][b][i][k]
        ok = pair[:, :, None, None] & (idx[:, None, :, None] >= 0) & (idx[None, :, None, :] >= 0)
        tgt = (idx[:, None, :, None] * n_c + idx[None, :, None, :])[ok]
        np.add.at(want, tgt, terms[ok])
        np.add.at(A, tgt, np.abs(terms[ok]))
        np.add.at(T, tgt, 1)
    if long_tracks:
        assert widest == wmax and np.diff(pt_ptr)[1] == 17 and np.diff(pt_ptr)[2] == 33
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    arrs = dict(Jpose=np.ascontiguousarray(Jpose), Jcam=np.ascontiguousarray(Jcam), Jpt=np.ascontiguousarray(Jpt),
                Cinv=np.ascontiguousarray(Cinv), a2c=ints(perm), pt_ptr=ints(pt_ptr), pt_off=ints(pt_off),
                a_pose=ints([o[1] for o in obs]), a_cam=ints([o[2] for o in obs]), a_pt=ints([o[0] for o in obs]),
                pose_off=ints(pose_off), pose_dim=ints(pose_dim), cam_off=ints(cam_off), cam_dim=ints(cam_dim))
    if rigs:
        arrs.update(Jsens=np.ascontiguousarray(Jsens), a_sensor=ints([o[3] for o in obs]), sens_off=ints(sens_off))
    for v in arrs.values():
        v.setflags(write=False)
    sq = lambda v: v.reshape(n_c, n_c)
    return dict(N=N, n_points=n_points, n_c=n_c, n_poses=n_poses, kd=kd, arrs=arrs, want=sq(want), A=sq(A), T=sq(T),
                want64=sq(want).astype(np.float64))


def formation_bar(P, fixed):
    """Per entry, from the reference alone. Fixed point: one quantum for each __double2ll_rn (at most one per term) plus
    the fp64 rounding inside a term, a few operations deep: T 2^-60 + 4 eps A. fp64 atomics: (T + 4) eps A, any order."""
    T, A = P["T"].astype(np.float64), P["A"].astype(np.float64)
    return T * QUANTUM + 4 * EPS * A if fixed else (T + 4) * EPS * A


def _upload_form_args(ad, P, fixed):
    dev = {k: ad.to_device(v) for k, v in P["arrs"].items()}
    bad = ad.to_device(np.zeros(1, np.int32))
    fa = FormArgs(n_obs=P["N"], n_points=P["n_points"], n_c=P["n_c"], n_poses=P["n_poses"], kd=P["kd"], fixed_point=fixed,
                  bad=bad.ptr)
    for k, b in dev.items():
        setattr(fa, k, b.ptr)
    return fa, bad, dev


def _form(ad, fa, bad, n_c, pairs, fixed, finish=True):
    """form() (+ finish()) into a fresh S pre-filled with 7.0; pairs: None or a built PairLists."""
    S = ad.to_device(np.full((n_c, n_c), 7.0))
    fa.pairs = C.addressof(pairs) if pairs is not None else None
    ad.api.form(C.byref(fa), _p(S), None)
    if finish:
        ad.api.finish(_p(S), C.c_int(n_c), C.c_bool(fixed), _p(bad), None)
    fa.pairs = None
    return S


def _assert_within(got, want, bar, what):
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    worst = float((err / np.maximum(bar, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max |err| {err.max():.3e}, worst err / bar {worst:.3f}")
    assert np.isfinite(got).all(), what
    assert (err <= bar).all(), (what, float(err.max()), worst)


def case_formation(ad, P, fixed, legacy_bars=False, repeat=True):
    """form() both ways -- a.pairs == NULL (form_kernel, one wave per point, one atomic per term) and built pair lists
    (records, incidences sorted by pose pair, one wave per 64 of them) -- against the longdouble reference on the lower
    triangle, within formation_bar. The two formations differ by rounding only (the records use F G^T): close, not
    bit-equal; a second run of each fixed-point formation is bit-identical to the first.
    legacy_bars adds the flat bars the stand-in suite has always asserted (2e-15 against numpy, 1e-15 between the two)."""
    n_c, low = P["n_c"], np.tril_indices(P["n_c"])
    assert np.abs(P["want64"]).max() < 1.0  # the fixed point needs it
    bar = formation_bar(P, fixed)[low]
    fa, bad, dev = _upload_form_args(ad, P, fixed)
    got = {}
    for which in ("points", "pairs"):
        pl = PairLists()
        if which == "pairs":
            assert ad.api.build_pair_lists(C.byref(fa), C.byref(pl), None) and pl.n_inc >= P["N"]
        runs = []
        for _ in range(2 if (fixed and repeat) else 1):
            S = ad.to_host(_form(ad, fa, bad, n_c, pl if which == "pairs" else None, fixed))
            assert ad.to_host(bad)[0] == 0
            runs.append(S)
        ad.api.free_pair_lists(C.byref(pl))
        assert pl.inc is None
        if len(runs) == 2:
            assert np.array_equal(runs[0][low].view(np.int64), runs[1][low].view(np.int64)), which + ": not bit-reproducible"
        got[which] = runs[0][low]
        _assert_within(got[which], P["want"][low], bar, f"formation {which} kd={P['kd']} fixed={fixed}")
        if legacy_bars:
            np.testing.assert_allclose(got[which], P["want64"][low], rtol=0, atol=2e-15)
    # the two formations against each other: the stand-in suite's flat 1e-15 on its own problems; elsewhere what the two
    # bars against the reference leave (entries near 1 summed from hundreds of terms in fp64 differ by more than 1e-15)
    if legacy_bars:
        np.testing.assert_allclose(got["pairs"], got["points"], rtol=0, atol=1e-15)
    assert (np.abs(got["pairs"] - got["points"]) <= 2 * bar).all()


def case_fixed_point_overflow(ad, scale, expect_bad):
    """form_kernel<.., FIXED> on two observations of one point in two pose blocks against numpy:
    S = sum_ab J_a^T (delta_ab I - E_a C^-1 E_b^T) J_b, accumulated in 2^-60 fixed point. With columns scaled as Jacobi
    scaling leaves them (|term| < 1) the matrix is exact to the quantum; a term the fixed point cannot hold raises
    FormArgs::bad, finish() poisons S[0][0] and the factorisation answers NaN (the LM loop rejects such a step) --
    the integer conversion alone would have produced a finite, wrong matrix."""
    rng = np.random.default_rng(5)
    N, n_c = 2, 12
    Jpose = (scale * rng.uniform(-1, 1, (12, N)))          # c-order planes [2 * 6][N]
    Jpt = (scale * rng.uniform(-1, 1, (6, N)))             # p-order planes [2 * 3][N]
    E = [np.array([[Jpt[r * 3 + m, a] for m in range(3)] for r in range(2)]) for a in range(N)]
    Cinv = np.linalg.inv(sum(e.T @ e for e in E) + 0.5 * scale * scale * np.eye(3))
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    arrs = dict(Jpose=np.ascontiguousarray(Jpose), Jcam=np.zeros((8, N)), Jpt=np.ascontiguousarray(Jpt),
                Cinv=np.ascontiguousarray(Cinv.reshape(1, 9)), a2c=ints([0, 1]), pt_ptr=ints([0, 2]), pt_off=ints([0]),
                a_pose=ints([0, 1]), a_cam=ints([0, 0]), pose_off=ints([0, 6]), pose_dim=ints([6, 6]), cam_off=ints([-1]),
                cam_dim=ints([0]))
    P = dict(N=N, n_points=1, n_c=n_c, n_poses=0, kd=4, arrs=arrs)
    fa, bad, dev = _upload_form_args(ad, P, True)
    Sd = ad.to_device(np.full((n_c + 1, n_c), 7.0))  # (n_c + 1 rows: factor_solve's buffer)
    ad.api.form(C.byref(fa), _p(Sd), None)
    ad.api.finish(_p(Sd), C.c_int(n_c), C.c_bool(True), _p(bad), None)
    S = ad.to_host(Sd)
    J = [np.array([[Jpose[r * 6 + d, a] for d in range(6)] for r in range(2)]) for a in range(N)]
    want = np.zeros((n_c, n_c))
    for a in range(N):
        for b in range(N):
            M = (np.eye(2) if a == b else 0.0) - E[a] @ Cinv @ E[b].T
            want[6 * a:6 * a + 6, 6 * b:6 * b + 6] += J[a].T @ M @ J[b]
    assert bool(ad.to_host(bad)[0]) == expect_bad
    if not expect_bad:
        low = np.tril_indices(n_c)
        assert np.abs(want).max() < 1.0
        np.testing.assert_allclose(S[:n_c][low], want[low], rtol=0, atol=144 * 2.0 ** -60 + 1e-17)
        return
    assert np.isnan(S[0, 0])
    _, _, x, info = _run_factor_solve(ad, Sd, n_c, np.ones(n_c), 12 * 128, False)
    assert info == 1 and np.isnan(x).all()


# ------------------------------------------------------------------------------------------------
# prior rows and the LM diagonal
# ------------------------------------------------------------------------------------------------

def case_prior_rows_and_lm_diagonal(ad, fixed):
    """add_prior_rows and add_lm_diagonal on top of a formed S (pair-major; kd = 4 with rigs) against J^T J scattered by
    numpy. J is [3][12][count]: pdim pose columns, then six sensor columns when so >= 0 (prior_rows_kernel). The solver
    passes pdim = 0 with po = -1 (constant pose) and never a prior with both blocks constant; here: pose alone with
    pdim 6 / 5 / 3, sensor alone, and both, several priors on one block. A prior term sum_r J[r][i] J[r][k] enters the
    bar like a formation term, with the absolute products as its magnitude. The diagonal kernel adds Dc[i]^2 (the header:
    D, not D^2, is passed): one more rounded product and one more rounded sum on the diagonal."""
    P = formation_problem(14, 9, 60, True, True)
    n_c, low = P["n_c"], np.tril_indices(P["n_c"])
    a = P["arrs"]
    pose_off, pose_dim, sens_off = a["pose_off"], a["pose_dim"], a["sens_off"]
    live_p = [i for i in range(len(pose_off)) if pose_off[i] >= 0]
    live_s = [i for i in range(len(sens_off)) if sens_off[i] >= 0]
    p6 = [i for i in live_p if pose_dim[i] == 6]
    assert len(p6) >= 2 and live_s
    pa, pb, s0 = pose_off[p6[0]], pose_off[p6[1]], sens_off[live_s[0]]
    # (pose offset, sensor offset, pdim): the kernel takes pdim from its argument -- 5 and 3 address the first columns of
    # a block
    priors = [(pa, -1, 6), (pb, -1, 5), (pa, -1, 3), (-1, s0, 0), (pa, s0, 6), (pb, s0, 5), (pb, sens_off[live_s[-1]], 3),
              (pa, -1, 6)]
    count = len(priors)
    rng = np.random.default_rng(77)
    J = 0.1 * rng.uniform(-1, 1, (3, 12, count))
    want, A, T = P["want"].copy(), P["A"].copy(), P["T"].astype(np.float64)
    for k, (po, so, pd) in enumerate(priors):
        idx = [po + i for i in range(pd)] + ([so + i for i in range(6)] if so >= 0 else [])
        Jk = J[:, :len(idx), k].astype(LD)
        prods = Jk[:, :, None] * Jk[:, None, :]
        want[np.ix_(idx, idx)] += prods.sum(0)
        A[np.ix_(idx, idx)] += np.abs(prods).sum(0)
        T[np.ix_(idx, idx)] += 1
    Dc = rng.uniform(0.01, 0.3, n_c)
    dg = np.arange(n_c)
    bar = (T * QUANTUM + 4 * EPS * A if fixed else (T + 4) * EPS * A).astype(np.float64)
    want[dg, dg] += Dc.astype(LD) ** 2
    bar[dg, dg] += 2 * EPS * (np.abs(want[dg, dg]).astype(np.float64) + Dc * Dc)
    assert np.abs(want).max() < 1.0
    fa, bad, dev = _upload_form_args(ad, P, fixed)
    pl = PairLists()
    assert ad.api.build_pair_lists(C.byref(fa), C.byref(pl), None)
    S = _form(ad, fa, bad, n_c, pl, fixed, finish=False)
    ad.api.free_pair_lists(C.byref(pl))
    ints = lambda v: ad.to_device(np.ascontiguousarray(v, np.int32))
    Jd, pod, sod, pdd = ad.to_device(J), ints([p[0] for p in priors]), ints([p[1] for p in priors]), ints([p[2] for p in priors])
    ad.api.add_prior_rows(_p(S), C.c_int(n_c), _p(Jd), _p(pod), _p(sod), _p(pdd), C.c_int(count), C.c_bool(fixed), _p(bad), None)
    ad.api.finish(_p(S), C.c_int(n_c), C.c_bool(fixed), _p(bad), None)
    Dd = ad.to_device(Dc)
    ad.api.add_lm_diagonal(_p(S), C.c_int(n_c), _p(Dd), None)
    got = ad.to_host(S)
    assert ad.to_host(bad)[0] == 0
    _assert_within(got[low], want[low], bar[low], f"prior rows + diagonal fixed={fixed}")
    # the priors and the diagonal did change what they should: without them the comparison fails
    assert (np.abs(got[low] - P["want64"][low]) > bar[low]).sum() >= count


# ------------------------------------------------------------------------------------------------
# blocked Cholesky
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def spd_problem(n):
    """A = B B^T / n + 0.5 I (eigenvalues in about [0.5, 5]: every 64-block of its factor is well conditioned) and a
    right-hand side; shared between the tests, read-only."""
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n + 8))
    A = B @ B.T / n + 0.5 * np.eye(n)
    rhs = rng.standard_normal(n)
    A.setflags(write=False); rhs.setflags(write=False)
    return A, rhs


def _run_factor_solve(ad, Sd, n, rhs, min_rows128, lookahead):
    """factor_solve on the device buffer Sd ((n + 1) x n). Returns (S host, Linv host [nb][64][64], x, info)."""
    nb = (n + 63) // 64
    x, linv = ad.to_device(np.zeros(n)), ad.to_device(np.zeros(nb * 64 * 64))
    tmp, info = ad.to_device(np.zeros(n)), ad.to_device(np.zeros(1, np.int32))
    rhs_d = ad.to_device(np.ascontiguousarray(rhs, np.float64))
    ws = Workspace(Linv=linv.ptr, tmp=tmp.ptr, info=info.ptr, min_rows128=min_rows128)
    if lookahead:
        ws.st2, ws.ev_panel, ws.ev_u2 = ad.lookahead()
    ad.api.factor_solve(_p(Sd), C.c_int(n), _p(rhs_d), _p(x), C.byref(ws), None, None, None, None)
    S = ad.to_host(Sd)
    return S, ad.to_host(linv).reshape(-1, 64, 64), ad.to_host(x), int(ad.to_host(info)[0])


def factor_solve(ad, A, rhs, min_rows128=12 * 128, lookahead=False, keep_device=False):
    n = A.shape[0]
    S = np.full((n + 1, n), 1e300)  # the upper triangle is never read; row n: the right-hand side rides along
    S[np.tril_indices(n)] = A[np.tril_indices(n)]
    Sd = ad.to_device(S)
    out = _run_factor_solve(ad, Sd, n, rhs, min_rows128, lookahead)
    return out + (Sd,) if keep_device else out


def _check_factor(A, rhs, S, linv, x, forward_bars):
    """The componentwise backward bounds of the factorisation and of the solve (theorems for any summation order, Higham,
    Accuracy and Stability of Numerical Algorithms, 10.2 and 10.4), the structure of the stored block inverses, the
    inverses of the 64-blocks; forward_bars adds the comparisons with numpy's own factor and solution.
        |A - L L^T| <= gamma_{n+1} |L| |L^T|,         |b - A x| <= gamma_{3n+1} |L| |L^T| |x|.
    The kernels replace the triangular solves by products with the explicit inverses of the 64 x 64 diagonal blocks; with
    the well-conditioned blocks of spd_problem that stays inside the same bounds (the n-fold slack of gamma_n over the
    actual rounding covers the blocks' condition numbers, < 4). Up to n = 333 the products are evaluated in longdouble;
    beyond, in fp64 BLAS, and that evaluation's own error -- gamma_n |L| |L^T| for the product, eps |A| for the
    subtraction, gamma_{n+1} (|A| |x| + |b|) for the residual -- is added to the bound."""
    n = A.shape[0]
    low = np.tril_indices(n)
    assert np.isfinite(S[:n][low]).all() and np.isfinite(x).all()
    L = np.tril(S[:n])
    exact = n <= 333
    Lw = L.astype(LD) if exact else L
    absLLt = np.abs(L) @ np.abs(L).T
    res = np.abs(A - Lw @ Lw.T).astype(np.float64)
    bound = gamma(n + 1) * absLLt if exact else (gamma(n + 1) + gamma(n)) * absLLt * (1 + gamma(n)) + EPS * np.abs(A)
    worst_f = float((res[low] / bound[low]).max())
    assert (res[low] <= bound[low]).all(), ("factorisation", n, worst_f)
    Aw, xw = (A.astype(LD), x.astype(LD)) if exact else (A, x)
    r = np.abs(rhs - Aw @ xw).astype(np.float64)
    sbound = gamma(3 * n + 1) * (1 + gamma(n)) * (absLLt @ np.abs(x))
    if not exact:
        sbound = sbound + gamma(n + 1) * (np.abs(A) @ np.abs(x) + np.abs(rhs))
    worst_s = float((r / sbound).max())
    print(f"factor_solve n={n}: worst |A - L L^T| / bound {worst_f:.4f}, worst |b - A x| / bound {worst_s:.4f}")
    assert (r <= sbound).all(), ("solve", n, worst_s)
    for k in range((n + 63) // 64):
        kb = min(64, n - 64 * k)
        assert (linv[k][kb:, :] == 0).all() and (linv[k][:, kb:] == 0).all()
        assert (np.triu(linv[k][:kb, :kb], 1) == 0).all()
        # against the inverse of the device's own block (for the numpy factor's blocks see forward_bars: same 1e-11)
        np.testing.assert_allclose(linv[k][:kb, :kb], np.linalg.inv(L[64 * k:64 * k + kb, 64 * k:64 * k + kb]), rtol=0, atol=1e-11)
    if forward_bars:
        Ln = np.linalg.cholesky(A)
        np.testing.assert_allclose(S[:n][low], Ln[low], rtol=0, atol=1e-12)
        for k in range((n + 63) // 64):
            kb = min(64, n - 64 * k)
            np.testing.assert_allclose(linv[k][:kb, :kb], np.linalg.inv(Ln[64 * k:64 * k + kb, 64 * k:64 * k + kb]), rtol=0, atol=1e-11)
        np.testing.assert_allclose(x, np.linalg.solve(A, rhs), rtol=0, atol=1e-10)


FORWARD_BAR_CASES = {(45, 12 * 128), (64, 12 * 128), (333, 12 * 128), (900, 256)}


def case_cholesky(ad, n, min_rows128=12 * 128, lookahead=False):
    """factor_solve on a random SPD matrix. n = 1 / 45 / 64: one diagonal block (chol_diag_kernel alone); 65: a second,
    one-row block; 255 / 256 / 257: around the outer panel of 256 columns; 333: six panels, a ragged last block, two outer
    panels; 900 with the tile threshold lowered and 2100 with the production threshold (the first second-stream update has
    1589 >= 1536 rows: 128 x 128 tiles; the next, 1333 rows: 64 x 64; a ragged last panel)."""
    A, rhs = spd_problem(n)
    S, linv, x, info = factor_solve(ad, A, rhs, min_rows128, lookahead)
    assert info == 0
    _check_factor(A, rhs, S, linv, x, (n, min_rows128) in FORWARD_BAR_CASES)
    return S, linv, x


def case_cholesky_lookahead(ad, n, min_rows128):
    """Without the second stream and with it, on the same matrix: both meet the bounds (tile shapes differ: no bit
    equality between them); two runs WITH lookahead are bit-identical in S, Linv and x -- an update that did not wait
    for the other stream's writes cannot pass that reliably. Run twice, not in a loop."""
    case_cholesky(ad, n, min_rows128, lookahead=False)
    first = case_cholesky(ad, n, min_rows128, lookahead=True)
    A, rhs = spd_problem(n)
    second = factor_solve(ad, A, rhs, min_rows128, True)[:3]
    low = np.tril_indices(n)
    for name, u, v in zip(("S", "Linv", "x"), first, second):
        if name == "S":
            u, v = np.concatenate([u[:n][low], u[n]]), np.concatenate([v[:n][low], v[n]])
        assert np.array_equal(u.view(np.int64), v.view(np.int64)), f"lookahead, n = {n}: {name} differs between two runs"


def case_failed_pivot(ad, n, pivot):
    A = np.eye(n)
    A[pivot, pivot] = -1.0
    _, _, x, info = factor_solve(ad, A, np.ones(n))
    assert info == 1 and np.isnan(x).all()


# ------------------------------------------------------------------------------------------------
# triangular inverse and covariance blocks
# ------------------------------------------------------------------------------------------------

def _tri_inverse_longdouble(L):
    """L^-1 of a lower-triangular matrix by forward substitution in longdouble, row by row."""
    m = L.shape[0]
    Lw = L.astype(LD)
    X = np.zeros((m, m), LD)
    for i in range(m):
        row = -(Lw[i, :i] @ X[:i, :i + 1]) if i else np.zeros(1, LD)
        row[i] += 1.0
        X[i, :i + 1] = row / Lw[i, i]
    return X


def _tri_inverse_fp64(L):
    """The same substitution in plain fp64 (scipy's solve_triangular where there is one)."""
    try:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, np.eye(L.shape[0]), lower=True)
    except ImportError:
        return np.linalg.solve(L, np.eye(L.shape[0]))


def run_tri_inverse(ad, n, j0):
    """factor_solve, then tri_inverse from block j0 on. Returns (X device, X host, trailing block of the device's L)."""
    A, rhs = spd_problem(n)
    S, linv, x, info, Sd = factor_solve(ad, A, rhs, keep_device=True)
    assert info == 0
    m = n - 64 * j0
    linv_d = ad.to_device(linv.reshape(-1))
    Xd = ad.to_device(np.full(m * m, 3.0))  # (cleared inside)
    ad.api.tri_inverse(_p(Sd), C.c_int(n), C.c_int(j0), _p(linv_d), _p(Xd), None)
    X = ad.to_host(Xd).reshape(m, m)
    return Xd, X, np.tril(S[:n])[64 * j0:, 64 * j0:]


def case_tri_inverse(ad, n, j0):
    """X = tri_inverse(L, j0) against the inverse of the trailing block of the DEVICE'S OWN factor, computed in longdouble
    by forward substitution (this isolates tri_inv_row_kernel from the factorisation). X holds exactly (n - 64 j0)^2
    doubles, lower triangular with exact zeros above the diagonal. Bar: 10 x the floor, the floor being the error of the
    same inverse computed in plain fp64 against the longdouble one on the same factor -- measured from the reference, with
    the margin tests/ba_compare.py gives a different but valid operation order."""
    Xd, X, Lt = run_tri_inverse(ad, n, j0)
    m = n - 64 * j0
    assert X.shape == (m, m) and np.isfinite(X).all()
    assert (np.triu(X, 1) == 0).all()
    ref = _tri_inverse_longdouble(Lt)
    floor = float(np.abs(_tri_inverse_fp64(Lt).astype(LD) - ref).max())
    err = float(np.abs(X.astype(LD) - ref).max())
    print(f"tri_inverse n={n} j0={j0}: floor {floor:.3e}, error {err:.3e}, bar {10 * floor:.3e}")
    assert floor > 0 and err <= 10 * floor, (n, j0, err, floor)


def cov_pairs(m, count, seed):
    """`count` block pairs inside an m x m X: the widths (1, 1), (6, 6), (6, 16), (16, 6), (16, 16) -- the last fills the
    256-double slot --, a0 < b0, a0 > b0 and a0 == b0, blocks at column 0 and ending at the last column."""
    rng = np.random.default_rng(seed)
    fixed = [(m - 16, 16, m - 16, 16), (0, 16, m - 16, 16), (m - 6, 6, 0, 16), (0, 1, 0, 1), (m - 1, 1, 3, 1), (5, 6, 5, 6),
             (7, 6, 40, 16), (90, 16, 12, 6), (64, 16, 60, 16), (m - 16, 16, m - 22, 6)]
    widths = [(1, 1), (6, 6), (6, 16), (16, 6), (16, 16)]
    out = list(fixed[:count])
    while len(out) < count:
        da, db = widths[len(out) % 5]
        out.append((int(rng.integers(0, m - da + 1)), da, int(rng.integers(0, m - db + 1)), db))
    assert all(0 <= a0 and a0 + da <= m and 0 <= b0 and b0 + db <= m for a0, da, b0, db in out)
    return out


def case_extract_cov_blocks(ad, n=333, j0=2):
    """extract_cov_blocks on the X of tri_inverse (its n argument is the leading dimension of X, n - 64 j0) with a random
    positive scale, a list of 40 pairs and a list of one, against s_a (X^T X)_ab s_b in longdouble. Bar per entry:
    (m + 2) eps sum_r |X_ra| |X_rb| s_a s_b with m the number of summed rows -- the fma chain over a wave's rows plus the
    fixed four-way tree and the two scalings. Two calls give bit-identical results. Slots beyond da db are not asserted."""
    Xd, X, _ = run_tri_inverse(ad, n, j0)
    m = n - 64 * j0
    rng = np.random.default_rng(9)
    scale = rng.uniform(0.5, 2.0, m)
    scale_d = ad.to_device(scale)
    Xl, aX = X.astype(LD), np.abs(X)
    for count in (40, 1):
        pairs = cov_pairs(m, count, seed=count)
        pairs_d = ad.to_device(np.ascontiguousarray(pairs, np.int32))
        outs = []
        for _ in range(2):
            out_d = ad.to_device(np.full(count * COV_SLOT, -5.0))
            ad.api.extract_cov_blocks(_p(Xd), C.c_int(m), _p(pairs_d), C.c_int(count), _p(scale_d), _p(out_d), None)
            outs.append(ad.to_host(out_d).reshape(count, COV_SLOT))
        worst = 0.0
        for k, (a0, da, b0, db) in enumerate(pairs):
            sa, sb = scale[a0:a0 + da], scale[b0:b0 + db]
            want = sa.astype(LD)[:, None] * (Xl[:, a0:a0 + da].T @ Xl[:, b0:b0 + db]) * sb.astype(LD)[None, :]
            rows = m - max(a0, b0)
            bar = (rows + 2) * EPS * (aX[:, a0:a0 + da].T @ aX[:, b0:b0 + db]) * sa[:, None] * sb[None, :] * (1 + 1e-12)
            got = outs[0][k, :da * db].reshape(da, db)
            err = np.abs(got.astype(LD) - want).astype(np.float64)
            worst = max(worst, float((err / bar).max()))
            assert np.isfinite(got).all() and (err <= bar).all(), (count, k, pairs[k], float((err / bar).max()))
            assert np.array_equal(got.view(np.int64), outs[1][k, :da * db].reshape(da, db).view(np.int64)), (count, k)
        print(f"extract_cov_blocks {count} pairs: worst err / bar {worst:.4f}")
