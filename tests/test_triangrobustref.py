"""tests/_triangrobustref.py on the CPU: the pair enumeration is what the rules say, no point of any problem the GPU tests
compare on is excused (no decision within 1e-6 of its threshold, so every status, hypothesis and mask byte is compared with
==), the wrong-match dome is a problem on which plain triangulation fails and the consensus rules do not -- conditions on
the inputs, checked on the references alone -- and the edge set yields the statuses its construction says."""
import numpy as np
import pytest

import _triangref as T
import _triangrobustref as RR

ONE_DEGREE = float(np.deg2rad(1.0))


def _reference(P, **kw):
    kw.setdefault("bound", False)
    return RR.reference(P["cams15"], T.centers_of(P["cams15"]), P["row_ptr"], P["pt_idx"], P["uv"], len(P["pts"]), ONE_DEGREE, RR.MAX_ERROR,
                        pt_mask=P.get("pt_mask"), **kw)


def test_the_pair_enumeration():
    assert RR.pairs(2, 64) == [(0, 1)]
    assert RR.pairs(3, 64) == [(0, 1), (1, 2), (0, 2)]
    assert RR.pairs(4, 64) == [(0, 2), (1, 3), (0, 1), (1, 2), (2, 3), (0, 3)]
    assert RR.pairs(5, 64) == [(0, 2), (1, 3), (2, 4), (0, 3), (1, 4), (0, 1), (1, 2), (2, 3), (3, 4), (0, 4)]
    assert RR.pairs(5, 4) == RR.pairs(5, 64)[:4]
    for m in range(2, 65):
        pr = RR.pairs(m, 10 ** 6)
        assert len(pr) == m * (m - 1) // 2 == len(set(pr)) and all(a < b for a, b in pr)
        gaps = [min(b - a, m - (b - a)) for a, b in pr]
        assert gaps == sorted(gaps, reverse=True)                 # wide gaps first
        assert len(RR.pairs(m, 64)) == min(64, len(pr))
    seen = np.bincount(np.array(RR.pairs(64, 64)).ravel(), minlength=64)
    assert seen.min() >= 1 and seen.max() <= 3                    # the cap at a full sample: every observation about twice


@pytest.mark.parametrize("state,obs_noise", RR.DOME_CASES)
@pytest.mark.parametrize("max_hypotheses", [64, 4])
def test_no_dome_point_is_excused(state, obs_noise, max_hypotheses):
    P = RR.wrong_match_dome(state, obs_noise)
    ref = _reference(P, max_hypotheses=max_hypotheses)
    assert ref["excused"] == [], ref["excused"]
    assert ref["decisions"] > (50000 if max_hypotheses == 64 else 5000)
    assert ref["counts"]["triangulated"] > 250 and ref["counts"]["no_consensus"] > 10 and ref["counts"]["too_few"] >= 60
    from _problems import DOME_CROWDED
    n = np.bincount(P["pt_idx"].astype(np.int64), minlength=len(P["pts"]))
    assert n[DOME_CROWDED] > 64 and ref["status"][DOME_CROWDED] == RR.OK       # the second chunk is walked
    crowded = np.flatnonzero(P["pt_idx"] == DOME_CROWDED)
    assert (ref["inlier"][crowded[:64]] == 0).any() and (ref["inlier"][crowded[64:]] == 0).any()     # wrong matches on both sides of entry 64


def test_the_wrong_match_dome_defeats_the_midpoint_and_not_the_consensus():
    P = RR.wrong_match_dome(False, 1e-3)
    assert 300 < P["wrong"].sum() < 500
    ref = _reference(P)
    ok = ref["status"] == RR.OK
    far = np.linalg.norm(ref["X"][ok].astype(np.float64) - P["true_pts"][ok], axis=1)
    plain = T.reference(P["cams15"], T.centers_of(P["cams15"]), P["row_ptr"], P["pt_idx"], P["uv"], len(P["pts"]), ONE_DEGREE, bound=False)
    pok = plain["status"] == T.OK
    pfar = np.linalg.norm(plain["X"][pok].astype(np.float64) - P["true_pts"][pok], axis=1)
    print("TRIANGROBUSTREF dome: %d wrong of %d; consensus %s, %.2f %% of %d more than 0.05 from the truth, median %.4g; midpoint %.1f %% of %d, median %.3g; %d decisions"
          % (P["wrong"].sum(), len(P["wrong"]), ref["counts"], 100 * (far > 0.05).mean(), ok.sum(), np.median(far), 100 * (pfar > 0.05).mean(), pok.sum(),
             np.median(pfar), ref["decisions"]))
    assert (far > 0.05).mean() <= 0.02
    assert (pfar > 0.05).mean() >= 0.5
    assert (~P["wrong"] & (ref["inlier"] == 0)).sum() == 0          # no right observation is dropped


@pytest.mark.parametrize("min_inliers", [2, 3])
def test_edge_set_statuses(min_inliers):
    P = RR.edge_problem()
    ref = _reference(P, min_inliers=min_inliers, bound=True)
    status, hyp, zeros = RR.edge_expected(min_inliers)
    assert ref["excused"] == []
    assert np.array_equal(ref["status"], status), ref["status"]
    assert all(ref["hyp"][p] == k for p, k in hyp.items()), ref["hyp"]
    assert np.array_equal(np.flatnonzero(ref["inlier"] == 0), zeros)
    e = RR.EDGE
    assert ref["n_inl"][e["two_wrong"]] == 3 and ref["n_inl"][e["f_zero"]] == 3 and ref["n_inl"][e["behind"]] == 4
    assert ref["n_inl"][e["two_ray"]] == 2 and ref["n_inl"][e["tie"]] == 2
    ok = np.flatnonzero(ref["status"] == RR.OK)
    err = np.linalg.norm((ref["X"][ok] - P["true_pts"][ok].astype(T.LD)).astype(np.float64), axis=1)
    assert (err <= 1e-12).all(), err                              # exact observations: the inliers' midpoint is the point
    assert np.isfinite(ref["bound"]).all() and (ref["bound"][ok] > 0).all() and ref["bound"].max() < 1e-9


def test_the_refit_is_the_midpoint_of_the_inliers():
    P = RR.wrong_match_dome(True, 1e-3)
    ref = _reference(P, bound=True)
    ok = ref["status"] == RR.OK
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], ref["inlier"].astype(bool))
    mid = T.reference(P["cams15"], T.centers_of(P["cams15"]), rp, ri, ruv, len(P["pts"]), ONE_DEGREE, bound=False)
    assert (mid["status"][ok] == T.OK).all() and np.array_equal(mid["X"][ok], ref["X"][ok])
    assert (mid["n_used"][ok] == ref["n_inl"][ok]).all()
    assert np.isfinite(ref["bound"]).all() and ref["bound"][ok].max() < 1e-9


def test_no_point_is_excused_in_the_other_states_the_gpu_tests_compare_on():
    """under the masks the GPU tests set, on the list a first pass has cleaned (at both bounds of the second pass), and at the
    command-line test's flags"""
    import _solvecheck as SC
    P = RR.wrong_match_dome(False, 1e-3)
    _, pm = SC.dome_mask(P)
    first = _reference(dict(P, pt_mask=pm))
    assert first["excused"] == [] and (first["inlier"] == 0).sum() > 200
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], first["inlier"].astype(bool))
    cen = T.centers_of(P["cams15"])
    again = RR.reference(P["cams15"], cen, rp, ri, ruv, len(P["pts"]), ONE_DEGREE, RR.MAX_ERROR, pt_mask=pm, bound=False)
    tighter = RR.reference(P["cams15"], cen, rp, ri, ruv, len(P["pts"]), ONE_DEGREE, RR.SECOND_MAX_ERROR, pt_mask=pm, bound=False)
    assert again["excused"] == [] and (again["inlier"] == 0).sum() == 0          # the pass is idempotent on its own output here
    assert tighter["excused"] == [] and (tighter["inlier"] == 0).sum() > 0
    mask = np.zeros(len(P["pts"]), dtype=bool)
    mask[[3, 300]] = True
    for state in (False, True):
        assert _reference(dict(RR.wrong_match_dome(state, 1e-3), pt_mask=mask))["excused"] == []
    from _problems import DOME_CROWDED
    mask[:] = False
    mask[[DOME_CROWDED, 5, 100, 255, 256, 379, 399]] = True
    assert _reference(dict(P, pt_mask=mask))["excused"] == []
    cli = RR.reference(P["cams15"], cen, P["row_ptr"], P["pt_idx"], P["uv"], len(P["pts"]), float(np.deg2rad(2.0)), RR.MAX_ERROR, min_inliers=4,
                       max_hypotheses=8, bound=False)
    assert cli["excused"] == [] and cli["counts"]["triangulated"] > 200
