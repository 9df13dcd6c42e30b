"""tests/_triangref.py on the CPU: with exact observations the reference returns the true points within its own bound,
the statuses are what dome_problem's construction says, the edge set yields statuses 2 and 3 (and 1 for the unusable
observations), and on every problem tests/test_gpu_triangulate.py compares statuses on, no point's lambda_min lies within
1e-6 (relative) of the threshold 1 - cos(min_angle) -- so no GPU test has to excuse a point from the status comparison."""
import numpy as np
import pytest

import _triangref as T
from _problems import DOME_CROWDED, DOME_N_PTS, DOME_SINGLES, DOME_UNOBSERVED

ONE_DEGREE = float(np.deg2rad(1.0))


def _reference(P, min_angle=ONE_DEGREE, **kw):
    return T.reference(P["cams15"], T.centers_of(P["cams15"]), P["row_ptr"], P["pt_idx"], P["uv"], len(P["pts"]), min_angle, **kw)


@pytest.fixture(scope="module")
def exact():
    from _problems import dome_problem
    P = dome_problem(obs_noise=0.0, start_noise=0.0)
    return P, _reference(P)


def test_exact_observations_give_the_true_points(exact):
    P, ref = exact
    ok = ref["status"] == T.OK
    assert ok.sum() > 200
    err = np.linalg.norm((ref["X"][ok] - P["true_pts"][ok].astype(T.LD)).astype(np.float64), axis=1)
    over = err / ref["bound"][ok]
    print("TRIANGREF exact: %d points, worst |X - truth| %.3g, worst |err| / bound %.3g, largest bound %.3g"
          % (ok.sum(), err.max(), over.max(), ref["bound"][ok].max()))
    assert np.isfinite(ref["bound"]).all() and (over <= 1.0).all()
    assert ref["bound"][ok].max() < 1e-9 and np.median(ref["bound"][ok]) < 1e-12     # the bound is rounding, not slack
    assert np.isnan(ref["X"][~ok].astype(np.float64)).all() and (ref["bound"][~ok] == 0).all()


def test_statuses_are_what_the_construction_says(exact):
    P, ref = exact
    s, n = ref["status"], ref["n_used"]
    assert (s[1:DOME_SINGLES + 1] == T.TOO_FEW).all() and (n[1:DOME_SINGLES + 1] == 1).all()
    assert (s[DOME_N_PTS - DOME_UNOBSERVED:] == T.TOO_FEW).all() and (n[DOME_N_PTS - DOME_UNOBSERVED:] == 0).all()
    assert s[DOME_CROWDED] == T.OK and 80 <= n[DOME_CROWDED] <= 93
    assert (n == np.bincount(P["pt_idx"].astype(np.int64), minlength=DOME_N_PTS)).all()      # every observation is usable
    assert set(np.unique(s)) <= {T.OK, T.TOO_FEW, T.DEGENERATE}
    assert (n[s == T.TOO_FEW] < 2).all() and (n[s != T.TOO_FEW] >= 2).all()


@pytest.mark.parametrize("state,obs_noise", T.DOME_CASES)
def test_no_dome_point_sits_at_the_threshold(state, obs_noise):
    P = T.dome_case(state, obs_noise)
    ref = _reference(P, bound=False)
    assert len(T.cap_violations(ref)) == 0, T.cap_violations(ref)
    assert np.allclose(np.linalg.norm(P["pts"] - P["true_pts"], axis=1), T.START)


@pytest.mark.parametrize("deg", [1.0, 0.1])
def test_edge_set_statuses(deg):
    P = T.edge_problem()
    ref = _reference(P, float(np.deg2rad(deg)))
    assert len(T.cap_violations(ref)) == 0
    assert (ref["status"] == T.edge_expected(deg)).all(), ref["status"]
    assert ref["n_used"][T.EDGE["f_zero"]] == 1 and ref["n_used"][T.EDGE["k1_negative"]] == 1
    assert ref["status"][T.EDGE["diverging"]] == T.BEHIND and ref["status"][T.EDGE["same_centre"]] == T.DEGENERATE
    half = T.EDGE["half_degree"]
    assert abs(float(ref["lam_min"][half]) - (1 - np.cos(np.deg2rad(0.5)))) < 1e-9
    ok = ref["status"] == T.OK
    err = np.linalg.norm((ref["X"][ok] - P["true_pts"][ok].astype(T.LD)).astype(np.float64), axis=1)
    assert (err <= 1e-12).all(), err                          # exact observations (made in f64): the midpoint is the point


def test_a_masked_point_is_constant_and_reads_nothing():
    P = T.dome_case(False, 1e-3)
    mask = np.zeros(DOME_N_PTS, dtype=bool)
    mask[[DOME_CROWDED, 5, 100]] = True
    free, ref = _reference(P, bound=False), _reference(P, bound=False, pt_mask=mask)
    assert (ref["status"][mask] == T.CONSTANT).all() and (ref["n_used"][mask] == 0).all()
    assert (ref["status"][~mask] == free["status"][~mask]).all()
    same = ~mask & (free["status"] == T.OK)
    assert np.array_equal(ref["X"][same], free["X"][same])
