"""What the camera edge cases (tests/camera_edge_cases.py) must contain for the tests that use them to mean anything,
from the numpy checker alone: no GPU, no library."""
import numpy as np
import pytest

import camera_edge_cases as E
import rectify_reference as RR
import test_camera_projection_gpu as P
import undistort_reference as R


@pytest.mark.parametrize("name", E.ALL)
def test_edge_case_reaches_the_paths_it_is_named_for(name):
    c = E.case(name)
    n = E.census(c)
    print(f"{name}: {len(c.points)} points, {n}")
    for branch in c.branches:
        assert n[branch] > 0, f"{name} is named for {branch} and reaches it at no point"
    E.assert_margins(c)


def test_every_listed_branch_is_named_by_a_case():
    named = {b for name in E.ALL for b in E.case(name).branches}
    assert set(E.REQUIRED) <= named, sorted(set(E.REQUIRED) - named)


def test_census_figures_of_the_strongest_cases():
    """The counts the cases were chosen by: they change only if the cases or the checker change."""
    n = E.census(E.case("inverse-FULL_OPENCV-x40"))
    assert (n["newton_row_swap"], n["newton_not_converged"]) == (1563, 947)
    assert E.census(E.case("inverse-RAD_TAN_THIN_PRISM_FISHEYE-x8"))["newton_not_converged"] == 715
    assert E.census(E.case("inverse-SIMPLE_RADIAL-x40"))["newton_row_swap"] == 0
    assert E.census(E.case("forward-DIVISION-k0.2"))["disc_sq_negative"] == 1055
    assert E.census(E.case("forward-SIMPLE_DIVISION-k0.05"))["disc_sq_negative"] == 607
    assert E.census(E.case("forward-EUCM-0.9--0.3"))["eucm_rho2_negative"] == 807


def test_place_moves_a_point_off_a_threshold_and_keeps_the_rest():
    cam = E.case("forward-DIVISION-k0.2").cam                 # disc_sq = 1 - 0.8 r^2 is 0 at r^2 = 1.25
    pts = np.array([[np.sqrt(1.25), 0.0], [0.5, 0.25]])
    assert E.too_close("forward", cam, pts).tolist() == [True, False]
    moved = E.place("forward", cam, pts)
    assert len(moved) == 2 and np.array_equal(moved[1], pts[1]) and not np.array_equal(moved[0], pts[0])
    assert not E.too_close("forward", cam, moved).any()


def test_trace_leaves_the_checkers_values_unchanged():
    c = E.case("inverse-FULL_OPENCV-x8")
    xn, yn, e = E._normalized(c.cam, c.points)
    tr = R.NewtonTrace(len(xn))
    plain, traced = R.iterative_undistortion(c.cam.model_id, e, xn, yn), R.iterative_undistortion(c.cam.model_id, e, xn, yn, tr)
    for a, b in zip(plain, traced):
        assert a.tobytes() == b.tobytes()
    assert tr.iterations.max() == 100 and tr.iterations.min() >= 1 and (tr.clamped <= tr.iterations).all()
    assert np.array_equal(tr.converged, plain[2])


def test_checker_eligibility_share_is_small():
    """The exception of the warp parity rule, counted from the checker alone on the warps into the invalid region."""
    for name, channels, interp in P.WARP_CASES:
        cam, img = P.warp_inputs(name, channels)
        res = RR.warp_with_homography(np.eye(3), cam, E.WARP_TARGET, img, interp)
        assert res.may_differ.mean() <= 0.01, (name, channels, interp, res.may_differ.mean())
        assert 0.1 <= P._blank(res.image).mean() <= 0.9
