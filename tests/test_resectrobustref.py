"""The host reference of consensus resection (tests/_resectrobustref.py) against what it must reproduce, without a GPU: the
enumeration of triples; on the wrong-match dome plain resection loses most cameras and the consensus keeps them, drops no
right observation and stays near the truth; its refit is _resectref.reference on the restricted list; the hand-placed edge
set gets what its docstring lists; and no camera of the problems the GPU tests compare on is excused (the cap is zero)."""
import numpy as np
import pytest

import _resectref as T
import _resectrobustref as RR
import oracle as O


def _reference(P, **kw):
    return RR.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], RR.MAX_ERROR, **kw)


@pytest.fixture(scope="module")
def dome():
    out = {}
    for noise in (0.0, 1e-3):
        P = RR.wrong_match_dome_cameras(False, noise)
        out[noise] = (P, _reference(P))
    return out


def _closed_form(k, m):
    """the device's rrc_triple, restated: triple k of a sample of m without the loops"""
    if m < 3:
        return None
    third = m // 3
    exact = third * 3 == m
    if exact and k < third:
        g, i = third, k
    else:
        r = k - third if exact else k
        g, i = (third - 1 if exact else third) - r // m, r % m
    if g < 1:
        return None
    return tuple(sorted((i, (i + g) % m, (i + 2 * g) % m)))


def test_the_enumeration_names_every_triple_once_and_the_closed_form_agrees():
    for m in range(0, 65):
        t = RR.triples(m, 10 ** 9)
        want = sum(third if 3 * third == m else m for third in range(m // 3, 0, -1))
        assert len(t) == len(set(t)) == want, m
        assert all(a < b < c < m for a, b, c in t)
        if m >= 3:
            g = m // 3
            assert t[0] == (0, g, 2 * g)                         # the widest spacing first
        assert RR.triples(m, 64) == t[:64] and RR.triples(m, 1) == t[:1]
        for k in range(len(t) + 3):
            assert _closed_form(k, m) == (t[k] if k < len(t) else None), (m, k)


@pytest.mark.parametrize("noise", [0.0, 1e-3])
def test_consensus_keeps_the_cameras_plain_resection_loses(dome, noise):
    P, ref = dome[noise]
    plain = T.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], bound=False)
    cand = plain["n_used"] >= 6
    n = int(cand.sum())
    got_plain, got = int((plain["status"][cand] == T.OK).sum()), int((ref["status"][cand] == RR.OK).sum())
    wrong, dropped = P["wrong"], ref["inlier"] == 0
    ok = ref["status"] == RR.OK
    Rt, _ = T.pose_of(O.camera_from_bal(P["true_bal9"]))
    ang = T.rotation_angle_deg(ref["R"][ok], Rt[ok])
    cam_of = np.repeat(np.arange(len(ok)), np.diff(P["row_ptr"].astype(np.int64)))
    print("RESECTROBUSTREF noise %g: %d of %d observations wrong; plain %s; consensus %s; outliers %d, right dropped %d, wrong kept %d; "
          "rotation error median %.3g worst %.3g deg; %s" % (noise, wrong.sum(), len(wrong), T.counts_of(plain["status"]), ref["counts"], dropped.sum(),
                                                           (dropped & ~wrong).sum(), (~dropped & wrong & ok[cam_of]).sum(), np.median(ang), ang.max(), ref["stats"]))
    assert n == 63 and wrong.sum() > 400
    assert got_plain <= 0.25 * n                                 # 7 of 63
    assert got >= 0.9 * n                                        # 62 of 63
    assert not (dropped & ~wrong).any()
    assert ang.max() <= (2.0 if noise else 0.2)                  # 0.71 and 0.087 degrees


@pytest.mark.parametrize("noise", [0.0, 1e-3])
def test_no_camera_of_the_dome_is_excused(dome, noise):
    P, ref = dome[noise]
    assert ref["excused"] == []
    assert ref["stats"]["margin"] > 1e-5                         # every inlier decision far from max_error^2
    st = ref["stats"]                                            # the conditioning measure: DESIGN 4.12's figures, a factor of two each way
    assert 6e-4 < st["cond_median"] < 2.4e-3 and 0 < st["cond_rejected"] < 0.03 * st["solutions"], st
    capped = _reference(P, max_hypotheses=4, bound=False)
    assert capped["excused"] == [] and (capped["hyp"] < 4).all()


def test_the_refit_is_the_plain_reference_on_the_restricted_list(dome):
    P, ref = dome[1e-3]
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], ref["inlier"].astype(bool))
    plain = T.reference(P["cams15"], P["pts"], rp, ri, ruv, bound=False)
    ok = ref["status"] == RR.OK
    assert (plain["status"][ok] == T.OK).all() and (plain["n_used"][ok] == ref["n_inl"][ok]).all()
    assert np.array_equal(plain["R"][ok], ref["R"][ok]) and np.array_equal(plain["t"][ok], ref["t"][ok])
    assert np.isnan(ref["R"][~ok].astype(np.float64)).all()


@pytest.mark.parametrize("state,noise", RR.DOME_CASES)
def test_bal_and_state_mode_give_the_same_reference_whatever_the_starting_pose(dome, state, noise):
    """the four dome cases the GPU tests load: the reference reads the intrinsics, the points and the list, which the mode
    and the starting pose do not touch -- held here by running it on each case's own arrays"""
    P, ref = dome[noise]
    Q = RR.wrong_match_dome_cameras(state, noise, start_seed=18)
    assert np.array_equal(Q["pt_idx"], P["pt_idx"]) and np.array_equal(Q["uv"], P["uv"]) and np.array_equal(Q["cams15"][:, 12:], P["cams15"][:, 12:])
    assert np.array_equal(Q["pts"], P["pts"]) and not np.array_equal(Q["cams15"][:, :12], P["cams15"][:, :12])
    got = _reference(Q, bound=False, twin=False)                 # (the float64 twin is the fixture's business)
    assert got["excused"] == []
    for key in ("status", "hyp", "n_inl", "inlier"):
        assert np.array_equal(got[key], ref[key]), key
    ok = ref["status"] == RR.OK
    assert np.array_equal(got["R"][ok], ref["R"][ok]) and np.array_equal(got["t"][ok], ref["t"][ok])


def test_edge_set():
    P = RR.edge_problem()
    assert RR.edge_larger_depth_seed() == RR.LARGER_DEPTH_SEED
    ref = _reference(P, cam_mask=P["cam_mask"])
    status, hyp, n_inl, zeros = RR.edge_expected()
    assert ref["excused"] == []
    assert np.array_equal(ref["status"], status), ref["status"]
    assert all(ref["hyp"][c] == k for c, k in hyp.items()) and all(ref["n_inl"][c] == k for c, k in n_inl.items()), (ref["hyp"], ref["n_inl"])
    e = RR.EDGE
    assert ref["hyp"][e["collinear_first"]] > 0 and ref["hyp"][e["coplanar"]] >= 0 and ref["hyp"][e["five_right"]] >= 0
    assert ref["n_inl"][e["five_right"]] < 6 and ref["n_inl"][e["late"]] < 6
    assert np.array_equal(np.flatnonzero(ref["inlier"] == 0), zeros)
    Rt, tt = T.pose_of(P["true_cams15"])
    for name in ("two_wrong", "larger_depth", "collinear_first", "two_sets"):
        c = e[name]
        assert np.abs((ref["R"][c] - Rt[c]).astype(np.float64)).max() <= ref["bound_R"][c], name
        assert np.linalg.norm((ref["t"][c] - tt[c]).astype(np.float64)) <= ref["bound_t"][c], name
    c = e["coplanar"]                                            # the consensus pose itself is the true one; only the refit gives up
    assert np.abs((ref["R_hyp"][c] - Rt[c]).astype(np.float64)).max() < 1e-9


def test_the_end_to_end_problem_has_no_excused_camera_and_the_host_loop_shows_the_ordering():
    P = RR.e2e_problem()
    cams15 = O.camera_from_bal(P["bal9"])
    ref = RR.reference(cams15, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], RR.MAX_ERROR, bound=False)
    assert ref["excused"] == []
    plain = T.reference(cams15, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], bound=False)
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], ref["inlier"].astype(bool))
    host_rob, _ = T.host_cameras_lm(dict(P, row_ptr=rp, pt_idx=ri, uv=ruv, bal9=T.resected_bal9(P["bal9"], ref)), 10)
    host_plain, _ = T.host_cameras_lm(dict(P, bal9=T.resected_bal9(P["bal9"], plain)), 10)
    print("RESECTROBUSTREF e2e: %s, plain %s; host loop %.6g -> %.6g on the filtered list, %.6g -> %.6g from plain resection"
          % (ref["counts"], T.counts_of(plain["status"]), host_rob[0], host_rob[-1], host_plain[0], host_plain[-1]))
    assert host_plain[-1] > 100.0 * host_rob[-1]
