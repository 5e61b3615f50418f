"""colmap_amd/csrc/camera_projection.h built for the host alone (tests/cpp/test_camera_projection.cc, g++ with
-ffp-contract=off like the product) at every case of tests/camera_edge_cases.py, against references that share no code
with it:

  * distortion()'s hand-derived Jacobian against the checker's complex-step Jacobian (h = 1e-30: no subtraction, so both
    sides carry rounding only), within 1e-12 of max(1, max |J|) per point. No point is left out: near FULL_OPENCV's
    denominator zero (|den| down to 5e-4 in these cases) the quotient rule's den^2 scales J and its error alike, and the
    difference stays at 3e-15 of max |J| (9e-15 is the worst of all cases);
  * iterative_undistortion()'s flag and value, cam_from_img() and img_from_normalized() against the numpy checker: the same
    points without a value, values within 1e-9 of max(1, |value|);
  * the numpy checker's forward models against the 50-digit evaluation (tests/camera_projection_mp.py): the noise floor
    B of a double evaluation, asserted in test_camera_projection_gpu.forward_truth.

The second build runs the same program under the address and undefined-behaviour sanitizers: the header must be clean at
every case, the non-converging ones included."""
import os
import subprocess

import numpy as np
import pytest

import camera_edge_cases as E
import test_camera_projection_gpu as P
import undistort_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JACOBIAN_BAR = 1e-12
VALUE_BAR = 1e-9


def _write_cases(path):
    with open(path, "w") as f:
        for name in E.ALL:
            c = E.case(name)
            f.write(f"{name} {0 if c.kind == 'inverse' else 1} {c.cam.model_id} {len(c.cam.params)} {len(c.points)}\n")
            f.write(" ".join(repr(float(v)) for v in c.cam.params) + "\n")
            f.writelines(f"{float(x)!r} {float(y)!r}\n" for x, y in c.points)


def _read_dump(text):
    lines = text.splitlines()
    assert lines[-1] == "camera projection dump OK"
    out, i = {}, 0
    while i < len(lines) - 1:
        name, n = lines[i].split()
        n = int(n)
        out[name] = np.array([ln.split() for ln in lines[i + 1:i + 1 + n]], np.float64).reshape(n, 12)
        i += 1 + n
    return out


def _complex_step_jacobian(model, e, u, v):
    h = 1e-30
    with np.errstate(all="ignore"):
        dux, dvx = R.distortion(model, e, u + 1j * h, v + 0j)
        duy, dvy = R.distortion(model, e, u + 0j, v + 1j * h)
    return np.stack([np.imag(dux), np.imag(duy), np.imag(dvx), np.imag(dvy)], 1) / h


def _check_case(c, d):
    m, cam = c.cam.model_id, c.cam
    ok, value, dist, J, it_ok, it_value = d[:, 0] != 0, d[:, 1:3], d[:, 3:5], d[:, 5:9], d[:, 9] != 0, d[:, 10:12]
    e = R.split(m, cam.params)[4]
    if c.kind == "inverse":
        u, v, _ = E._normalized(cam, c.points)
        want = R.cam_from_img(cam, c.points)
    else:
        u, v = c.points[:, 0], c.points[:, 1]
        x, y, valid = R.img_from_normalized(cam, u, v)
        want = np.stack([x, y], 1)
        want[~valid] = np.nan
    figures = {}
    # values and validity
    assert np.array_equal(ok, ~np.isnan(want[:, 0])), f"{c.name}: the header and the checker disagree on which points have a value"
    assert np.isnan(value[~ok]).all()
    if ok.any():
        figures["value"] = float((np.abs(value[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max())
        assert figures["value"] <= VALUE_BAR
        if c.kind == "forward" and m in R.NO_TRANSCENDENTAL:
            assert np.array_equal(value[ok], want[ok])
    # distortion and its Jacobian
    if m in R.ITERATIVE:
        with np.errstate(all="ignore"):
            du, dv = R.distortion(m, e, u, v)
        want_J = _complex_step_jacobian(m, e, u, v)
        assert np.isfinite(want_J).all() and np.isfinite(J).all(), f"{c.name}: a Jacobian is not finite"
        rel = np.abs(J - want_J).max(1) / np.maximum(1.0, np.abs(want_J).max(1))
        figures["jacobian"] = float(rel.max())
        assert figures["jacobian"] <= JACOBIAN_BAR, f"{c.name}: Jacobian off by {figures['jacobian']:.3e} at {int(np.argmax(rel))}"
        scale = np.maximum(1.0, np.maximum(np.abs(du), np.abs(dv)))
        assert (np.abs(dist - np.stack([du, dv], 1)).max(1) <= 1e-12 * scale).all()
    # the Newton iteration itself
    if c.kind == "inverse" and m in R.ITERATIVE:
        x, y, done = R.iterative_undistortion(m, e, u, v)
        assert np.array_equal(it_ok, done), f"{c.name}: convergence flags differ at {np.nonzero(it_ok != done)[0][:8].tolist()}"
        w = np.stack([x, y], 1)[done]
        figures["newton"] = float((np.abs(it_value[done] - w) / np.maximum(1.0, np.abs(w))).max())
        assert figures["newton"] <= VALUE_BAR
        figures["not_converged"] = int((~done).sum())
    return figures


@pytest.mark.parametrize("sanitize", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_header_matches_independent_references(tmp_path, sanitize):
    exe, cases = str(tmp_path / "test_camera_projection"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + sanitize +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "colmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_camera_projection.cc"), "-o", exe])
    _write_cases(cases)
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    dump = _read_dump(r.stdout)
    assert sorted(dump) == sorted(E.ALL)
    for name in E.ALL:
        figures = _check_case(E.case(name), dump[name])
        print(name, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in figures.items()})


@pytest.mark.parametrize("name", E.FORWARD)
def test_checker_forward_models_against_50_digits(name):
    hi, lo, valid, B = P.forward_truth(name)
    assert valid.any() and np.isfinite(B)


def test_50_digit_equirectangular_matches_checker():
    """The 18th model has no pointwise device call (a spherical camera stays spherical); its formula is held here."""
    mp = pytest.importorskip("mpmath")
    import camera_projection_mp as M
    cam = R.Camera(R.EQUIRECTANGULAR, 1000, 500, [1000.0, 500.0])
    pts = E.FORWARD_GRID
    x, y, ok = R.img_from_normalized(cam, pts[:, 0], pts[:, 1])
    assert ok.all()
    worst = 0.0
    for (u, v), a, b in zip(pts, x, y):
        val = M.img_from_normalized(R.EQUIRECTANGULAR, cam.params, u, v)
        worst = max(worst, abs(float(mp.mpf(float(a)) - val[0])), abs(float(mp.mpf(float(b)) - val[1])))
    print(f"EQUIRECTANGULAR: max |checker - 50 digits| {worst:.3e} px")
    assert worst <= P.NOISE_FLOOR_BAR
