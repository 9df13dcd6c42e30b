"""The host reference of camera resection (tests/_resectref.py) against what it must reproduce, without a GPU: with exact
observations it returns dome_problem's true poses within its own bound; rows of fewer than six observations are too few; the
hand-placed edge set gets the statuses its docstring lists; no decision of the problems the GPU tests compare statuses on
lies at its threshold (the cap condition); and Gauss-Newton never ends above the linear start."""
import numpy as np
import pytest

import _resectref as T
import oracle as O


def _reference(P, **kw):
    return T.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], **kw)


@pytest.fixture(scope="module")
def dome():
    out = {}
    for noise in (0.0, 1e-3):
        P = T.dome_case(False, noise)
        out[noise] = (P, _reference(P))
    return out


def test_exact_observations_give_the_true_poses_within_the_bound(dome):
    P, ref = dome[0.0]
    ok = ref["status"] == T.OK
    lengths = np.diff(P["row_ptr"].astype(np.int64))
    assert np.array_equal(ok, lengths >= 6) and ok.sum() == 63
    assert (ref["status"][~ok] == T.TOO_FEW).all() and set(lengths[~ok]) == {0, 1, 2, 3, 4, 5}
    Rt, tt = T.pose_of(O.camera_from_bal(P["true_bal9"]))
    # the truth is the minimiser up to the rounding of the f64 observations it was projected to: uv carries 2^-53 relative,
    # which the bound's reruns (uv moved by 2^-52) cover
    eR = np.abs((ref["R"][ok] - Rt[ok]).astype(np.float64)).max(axis=(1, 2))
    et = np.linalg.norm((ref["t"][ok] - tt[ok]).astype(np.float64), axis=1)
    print("RESECTREF exact: worst |R - R_true| %.3g (bound %.3g), worst |t - t_true| %.3g (bound %.3g), worst angle %.3g deg"
          % (eR.max(), ref["bound_R"][ok].max(), et.max(), ref["bound_t"][ok].max(), T.rotation_angle_deg(ref["R"][ok], Rt[ok]).max()))
    assert (eR <= ref["bound_R"][ok]).all() and (et <= ref["bound_t"][ok]).all()
    assert T.counts_of(ref["status"]) == dict(resected=63, too_few=18, degenerate=0, behind=0, constant=0)


def test_noisy_observations_stay_near_the_truth(dome):
    P, ref = dome[1e-3]
    ok = ref["status"] == T.OK
    assert ok.sum() == 63
    Rt, tt = T.pose_of(O.camera_from_bal(P["true_bal9"]))
    ang = T.rotation_angle_deg(ref["R"][ok], Rt[ok])
    print("RESECTREF noise 1e-3: rotation error median %.3g max %.3g deg" % (np.median(ang), ang.max()))
    assert ang.max() < 1.0                                       # DESIGN 4.10's table: 0.56 degrees at most on the dome


def test_gauss_newton_never_ends_above_the_linear_start(dome):
    for noise, (P, ref) in dome.items():
        ok = ref["status"] == T.OK
        # the form is evaluated in longdouble: |r|^2 = 3, so it rounds at 3 lambda_9 eps (what exact observations leave of it)
        slack = 4 * float(np.finfo(T.LD).eps) * ref["lam9"][ok]
        assert (ref["form_end"][ok] <= ref["form_start"][ok] + slack).all(), noise
    P, ref = dome[1e-3]
    ok = ref["status"] == T.OK
    assert (ref["form_end"][ok] < ref["form_start"][ok]).all()


@pytest.mark.parametrize("min_gap", [1e-4, 1e-7])
def test_edge_set_statuses(min_gap):
    P = T.edge_problem()
    ref = _reference(P, min_gap=min_gap)
    assert np.array_equal(ref["status"], T.edge_expected(min_gap)), ref["status"]
    ratio = ref["lam2"] / ref["lam9"]
    assert abs(ratio[T.EDGE["coplanar"]]) < 1e-12 and 1e-7 < ratio[T.EDGE["clustered"]] < 1e-4
    assert ref["n_used"][T.EDGE["two_unusable"]] == 5
    assert len(T.cap_violations(ref)) == 0
    Rt, tt = T.pose_of(P["true_cams15"])
    for name in ("general", "no_distortion") + (("clustered",) if min_gap < 1e-6 else ()):
        c = T.EDGE[name]
        assert np.abs((ref["R"][c] - Rt[c]).astype(np.float64)).max() <= ref["bound_R"][c], name
        assert np.linalg.norm((ref["t"][c] - tt[c]).astype(np.float64)) <= ref["bound_t"][c], name


@pytest.mark.parametrize("state,obs_noise", T.DOME_CASES)
def test_cap_condition_on_the_dome(state, obs_noise, dome):
    ref = dome[obs_noise][1] if not state else _reference(T.dome_case(state, obs_noise), bound=False)
    assert len(T.cap_violations(ref)) == 0
    ok = ref["status"] == T.OK
    assert (ref["lam2"][ok] >= 5e-4 * ref["lam9"][ok]).all()     # the default min_gap = 1e-4 has room


def test_the_pose_bits_of_the_mask_make_a_camera_constant():
    P = T.dome_case(False, 1e-3)
    mask = np.zeros(len(P["bal9"]), dtype=np.uint16)
    mask[[2, 7]] = 0x001, 0x038
    mask[[11, 12]] = 0x1c0, 0x040                                # intrinsics only: still resected
    free, held = _reference(P, bound=False), _reference(P, cam_mask=mask, bound=False)
    assert (held["status"][[2, 7]] == T.CONSTANT).all()
    rest = np.ones(len(mask), dtype=bool)
    rest[[2, 7]] = False
    assert np.array_equal(held["status"][rest], free["status"][rest])
