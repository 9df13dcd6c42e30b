"""Consensus triangulation on the device (BAProblem.triangulate_points_robust / c2b_problem_triangulate_consensus /
c2b_triangulate_consensus_rows) against tests/_triangrobustref.py: status, selected hypothesis, inlier count and
inlier mask with == and the points within the reference's own bound on the wrong-match dome (rows from 0 to more than 64
entries, wrong matches on both sides of entry 64, a workgroup tail, mixed k2, duplicated pairs; bal and state mode) and on
the hand-placed edge set; the hypothesis cap; the refit bit for bit plain triangulation of the inliers; determinism and the
Level-0 entry; the list after drop_outliers and the state around it; refusals.  tests/test_triangrobustref.py asserts that
no point of these problems is excused, and every test here asserts it again for the cameras the device holds."""
import ctypes as C

import numpy as np
import pytest

import _triangref as T
import _triangrobustref as RR
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)
from test_gpu_triangulate import _level0_inputs, _load

pytestmark = pytest.mark.gpu
ONE_DEGREE = float(np.deg2rad(1.0))


def _reference(ba, pt_mask=None, max_error=RR.MAX_ERROR, **kw):
    """the reference on the device's own cameras and list (the state it holds, downloaded)"""
    cams = ba.cameras()
    ref = RR.reference(cams, T.centers_of(cams), ba.row_ptr, ba.pt_idx, ba.observations().reshape(-1, 2), ba.num_points(), ONE_DEGREE,
                       max_error, pt_mask=pt_mask, **kw)
    assert ref["excused"] == [], ref["excused"]
    return ref


def _check(ba, ref, before, out, status, hyp, inlier, tag):
    after = ba.points()
    assert np.array_equal(status, ref["status"]), (tag, np.flatnonzero(status != ref["status"]), status[status != ref["status"]])
    assert np.array_equal(hyp, ref["hyp"]), (tag, np.flatnonzero(hyp != ref["hyp"]))
    assert np.array_equal(inlier, ref["inlier"]), (tag, np.flatnonzero(inlier != ref["inlier"]))
    ok = status == RR.OK
    err = np.linalg.norm((after[ok].astype(T.LD) - ref["X"][ok]).astype(np.float64), axis=1)
    over = err / ref["bound"][ok] if ok.any() else np.zeros(1)
    print("TRIANGULATE ROBUST %s: %s; worst |X - X_ref| %.3g, worst |err| / bound %.3g" % (tag, out, err.max() if ok.any() else 0.0, over.max()))
    assert (over <= 1.0).all(), (tag, float(over.max()))
    assert _bits(after[~ok], before[~ok]), (tag, "a point whose status is not 0 moved")
    counts = {k: out[k] for k in RR.STATUS}
    assert counts == RR.counts_of(status) == ref["counts"], (tag, out)
    assert out["outliers"] == int((inlier == 0).sum()) and out["removed"] == 0
    return after


def _level0(env, ba, bal, pt_mask=None, **kw):
    """c2b_triangulate_consensus_rows on the handle's exported state: (pts4, status, hyp, n_inl, inlier, counts) with canaries"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    camblk, pts4, rows, prows, pt_idx, uv = _level0_inputs(env, ba, bal)
    n, no = prows.n_pts, prows.n_obs
    pts4 = pts4.clone()
    pts4[:, 3] = 7.25                                            # the fourth lane keeps its value
    status = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    hyp = torch.full((n + 64,), -7, dtype=torch.int32, device=dev)
    n_inl = torch.full((n + 64,), -7, dtype=torch.int32, device=dev)
    inlier = torch.full((no + 64,), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((6,), -1, dtype=torch.int64, device=dev)
    mask = None if pt_mask is None else torch.from_numpy(np.asarray(pt_mask, dtype=np.uint8)).to(dev)
    D.triangulate_consensus_rows(camblk, pts4, prows, uv, status, counts, ONE_DEGREE, RR.MAX_ERROR, pt_mask=mask, hyp=hyp, n_inl=n_inl,
                                 inlier=inlier, **kw)
    torch.cuda.synchronize()
    status, hyp, n_inl, inlier = _np(status), _np(hyp), _np(n_inl), _np(inlier)
    assert (status[n:] == 9).all() and (hyp[n:] == -7).all() and (n_inl[n:] == -7).all() and (inlier[no:] == 9).all()      # nothing past the end
    got = _np(pts4)
    assert (got[:, 3] == 7.25).all()
    return got[:, :3], status[:n], hyp[:n], n_inl[:n], inlier[:no], _np(counts)


# ---- 1. the wrong-match dome --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,obs_noise", RR.DOME_CASES)
def test_dome_matches_the_reference(env, state, obs_noise):
    P = RR.wrong_match_dome(state, obs_noise)
    ba = _load(P)
    before = ba.points()
    ref = _reference(ba)
    _, _, _, n_inl, _, _ = _level0(env, ba, not state)           # the inlier counts are a Level-0 output
    out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, return_status=True, return_inliers=True)
    after = _check(ba, ref, before, out, status, hyp, inlier, "dome state=%d obs_noise=%g" % (state, obs_noise))
    assert np.array_equal(n_inl, ref["n_inl"]), np.flatnonzero(n_inl != ref["n_inl"])
    ok = status == RR.OK
    assert out["triangulated"] > 250 and out["no_consensus"] > 10 and out["too_few"] >= 60 and out["outliers"] > 300
    far = np.linalg.norm(after[ok] - P["true_pts"][ok], axis=1)
    assert (far > 0.05).mean() <= 0.02                           # (the reference's own figure, asserted on it in test_triangrobustref)
    ba.close()


def test_the_hypothesis_cap(env):
    P = RR.wrong_match_dome(False, 1e-3)
    ba = _load(P)
    before = ba.points()
    ref, full = _reference(ba, max_hypotheses=4), _reference(ba, bound=False)
    assert (ref["hyp"] < 4).all() and not np.array_equal(ref["status"], full["status"])       # the cap decides something here
    out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, max_hypotheses=4, return_status=True, return_inliers=True)
    _check(ba, ref, before, out, status, hyp, inlier, "dome max_hypotheses=4")
    ba.close()


def test_the_refit_is_plain_triangulation_of_the_inliers_bit_for_bit(env):
    import city2ba_amd as c2b
    P = RR.wrong_match_dome(False, 1e-3)
    ba = _load(P)
    out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, return_status=True, return_inliers=True)
    got = ba.points()
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], inlier.astype(bool))
    plain = c2b.BAProblem.from_bal(P["bal9"], P["pts"], rp, ri, ruv, device=0)
    _, s_plain = plain.triangulate_points(return_status=True)
    ok = status == RR.OK
    assert ok.sum() > 250 and (s_plain[ok] == T.OK).all()
    assert _bits(got[ok], plain.points()[ok])
    plain.close()
    ba.close()


# ---- 2. the edge set and the point mask ---------------------------------------------------------------------------------
@pytest.mark.parametrize("min_inliers", [2, 3])
def test_edge_set(env, min_inliers):
    P = RR.edge_problem()
    ba = _load(P)
    ba.set_constant(points=P["pt_mask"])
    before = ba.points()
    ref = _reference(ba, pt_mask=P["pt_mask"], min_inliers=min_inliers)
    want_status, want_hyp, zeros = RR.edge_expected(min_inliers)
    assert np.array_equal(ref["status"], want_status)
    out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, min_inliers=min_inliers, return_status=True, return_inliers=True)
    _check(ba, ref, before, out, status, hyp, inlier, "edge set at min_inliers=%d" % min_inliers)
    assert np.array_equal(status, want_status) and all(hyp[p] == k for p, k in want_hyp.items())
    assert np.array_equal(np.flatnonzero(inlier == 0), zeros)
    _, l0_status, l0_hyp, n_inl, l0_inlier, _ = _level0(env, ba, False, pt_mask=P["pt_mask"], min_inliers=min_inliers)
    assert np.array_equal(n_inl, ref["n_inl"]) and np.array_equal(l0_status, status) and np.array_equal(l0_inlier, inlier)
    ba.close()


def test_constant_points_keep_their_bits_and_the_rest_is_the_unmasked_run(env):
    from _problems import DOME_CROWDED
    P = RR.wrong_match_dome(False, 1e-3)
    free = _load(P)
    _, s_free, h_free, i_free = free.triangulate_points_robust(RR.MAX_ERROR, return_status=True, return_inliers=True)
    x_free = free.points()
    free.close()
    mask = np.zeros(len(P["pts"]), dtype=bool)
    mask[[DOME_CROWDED, 5, 100, 255, 256, 379, 399]] = True
    ba = _load(P)
    before = ba.points()
    ba.set_constant(points=mask)
    out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, return_status=True, return_inliers=True)
    after = ba.points()
    assert (status[mask] == RR.CONSTANT).all() and (hyp[mask] == -1).all() and out["constant"] == mask.sum()
    assert (status[~mask] == s_free[~mask]).all() and (hyp[~mask] == h_free[~mask]).all()
    assert _bits(after[mask], before[mask]) and _bits(after[~mask], x_free[~mask])
    of_masked = mask[P["pt_idx"].astype(np.int64)]
    assert (inlier[of_masked] == 1).all() and np.array_equal(inlier[~of_masked], i_free[~of_masked])
    ba.close()


# ---- 3. determinism and Level 0 -----------------------------------------------------------------------------------------
def test_two_handles_give_the_same_bits(env):
    P = RR.wrong_match_dome(True, 1e-3)
    outs = []
    for _ in range(2):
        ba = _load(P)
        out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, return_status=True, return_inliers=True)
        outs.append((out, status, hyp, inlier, ba.points()))
        ba.close()
    assert outs[0][0] == outs[1][0] and all(_bits(a, b) for a, b in zip(outs[0][1:], outs[1][1:]))


@pytest.mark.parametrize("state", [False, True])
def test_level0_gives_the_problem_level_bits(env, state):
    P = RR.wrong_match_dome(state, 1e-3)
    ba = _load(P)
    mask = np.zeros(len(P["pts"]), dtype=np.uint8)
    mask[[3, 300]] = 1
    x, status, hyp, n_inl, inlier, counts = _level0(env, ba, not state, pt_mask=mask)
    ba.set_constant(points=mask.astype(bool))
    ref = _reference(ba, pt_mask=mask.astype(bool), bound=False)
    out, want_status, want_hyp, want_inlier = ba.triangulate_points_robust(RR.MAX_ERROR, return_status=True, return_inliers=True)
    assert _bits(status, want_status) and _bits(hyp, want_hyp) and _bits(inlier, want_inlier) and _bits(x, ba.points())
    assert dict(zip(RR.STATUS, (int(v) for v in counts))) == {k: out[k] for k in RR.STATUS}
    assert np.array_equal(n_inl, ref["n_inl"])
    ba.close()


def test_level0_without_the_optional_outputs(env):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = RR.wrong_match_dome(False, 1e-3)
    ba = _load(P)
    camblk, pts4, rows, prows, pt_idx, uv = _level0_inputs(env, ba, True)
    status = torch.zeros(prows.n_pts, dtype=torch.uint8, device=dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    D.triangulate_consensus_rows(camblk, pts4, prows, uv, status, counts, ONE_DEGREE, RR.MAX_ERROR)
    torch.cuda.synchronize()
    out, want = ba.triangulate_points_robust(RR.MAX_ERROR, return_status=True)[:2]
    assert _bits(_np(status), want) and _bits(_np(pts4)[:, :3], ba.points())
    ba.close()


# ---- 4. drop_outliers ---------------------------------------------------------------------------------------------------
def test_drop_outliers_compacts_the_list_by_the_mask_and_leaves_an_uploads_state(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    P = RR.wrong_match_dome(False, 1e-3)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    ba.set_constant(cm, pm)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-2)                                          # rows, transpose and solve buffers of the OLD list exist
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    ref = _reference(ba, pt_mask=pm, bound=False)
    out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, drop_outliers=True, return_status=True, return_inliers=True)
    assert np.array_equal(status, ref["status"]) and np.array_equal(inlier, ref["inlier"])
    zeros = int((inlier == 0).sum())
    assert out["removed"] == out["outliers"] == zeros > 200
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], inlier.astype(bool))
    assert ba.num_observations() == len(ri) == len(P["pt_idx"]) - zeros
    assert _bits(ba.row_ptr, rp) and _bits(ba.pt_idx, ri) and _bits(ba.observations().reshape(-1, 2), ruv)
    assert ba.num_cameras() == len(P["bal9"]) and ba.num_points() == len(P["pts"])             # nothing renumbered
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    p1 = ba.points()
    assert _bits(ba.cameras_bal(), b0) and not _bits(p1, p0)
    twin = c2b.BAProblem.from_bal(b0, p1, rp, ri, ruv, device=0)
    twin.set_constant(cm, pm)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    assert ba.total_reprojection_error(2.0) == twin.total_reprojection_error(2.0)
    twin.close()
    # a second call on that state removes what the reference says it removes there: nothing at the same bound (and then no
    # list changes hands), some at the tighter one
    for bound in (RR.MAX_ERROR, RR.SECOND_MAX_ERROR):
        ref2 = _reference(ba, pt_mask=pm, max_error=bound, bound=False)
        out2, status2, _, inlier2 = ba.triangulate_points_robust(bound, drop_outliers=True, return_status=True, return_inliers=True)
        assert np.array_equal(status2, ref2["status"]) and np.array_equal(inlier2, ref2["inlier"])
        assert out2["removed"] == int((ref2["inlier"] == 0).sum()) and (out2["removed"] > 0) == (bound != RR.MAX_ERROR)
    assert ba.num_observations() == len(ri) - out2["removed"]
    ba.rollback()                                                # the checkpoint taken before the first call
    assert _bits(ba.points(), p0) and _bits(ba.cameras_bal(), b0)
    ba.close()


def test_drop_outliers_with_nothing_to_drop_changes_no_list(env):
    P = T.dome_case(False, 0.0)                                  # exact observations, no wrong match
    ba = _load(P)
    out = ba.triangulate_points_robust(RR.MAX_ERROR, drop_outliers=True)
    assert out["outliers"] == 0 and out["removed"] == 0 and out["triangulated"] > 200
    assert ba.num_observations() == len(P["pt_idx"]) and _bits(ba.pt_idx, P["pt_idx"])
    ba.close()


# ---- 5. the state around the call, refusals, no observations ------------------------------------------------------------
def test_checkpoint_masks_loss_and_preconditioner_survive_and_nothing_stale_stays(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    P = RR.wrong_match_dome(False, 1e-3)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    ba.set_constant(cm, pm)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-2)
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    out = ba.triangulate_points_robust(RR.MAX_ERROR)
    assert out["triangulated"] > 200 and out["constant"] == pm.sum() and out["removed"] == 0
    p1 = ba.points()
    assert not _bits(p1, p0) and _bits(ba.cameras_bal(), b0)
    assert ba.num_observations() == len(P["pt_idx"]) and _bits(ba.pt_idx, P["pt_idx"])
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    twin = c2b.BAProblem.from_bal(b0, p1, P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    twin.set_constant(cm, pm)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    twin.close()
    ba.rollback()
    assert _bits(ba.points(), p0) and _bits(ba.cameras_bal(), b0)
    ba.close()


def test_state_mode_stays_state_mode(env):
    P = RR.wrong_match_dome(True, 1e-3)
    ba = _load(P)
    c0 = ba.cameras()
    ba.triangulate_points_robust(RR.MAX_ERROR)
    assert _bits(ba.cameras(), c0)
    ba.close()


def test_refusals_leave_the_problem_unchanged(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    P = RR.wrong_match_dome(False, 1e-3)
    ba = _load(P)
    before = ba.points()
    counts = (C.c_int64 * 6)(*([-7] * 6))
    removed = C.c_int64(-7)
    call = lambda angle, err, mi, mh, flags: L.lib().c2b_problem_triangulate_consensus(ba._h, angle, err, mi, mh, flags, None, None, None, counts,
                                                                                       C.byref(removed))
    inf, nan = float("inf"), float("nan")
    for args, word in (((-1.0, 0.01, 3, 64, 0), b"min_angle"), ((nan, 0.01, 3, 64, 0), b"min_angle"), ((2.0, 0.01, 3, 64, 0), b"min_angle"),
                       ((ONE_DEGREE, -1e-300, 3, 64, 0), b"max_error"), ((ONE_DEGREE, nan, 3, 64, 0), b"max_error"),
                       ((ONE_DEGREE, inf, 3, 64, 0), b"max_error"), ((ONE_DEGREE, 0.01, 1, 64, 0), b"min_inliers"),
                       ((ONE_DEGREE, 0.01, -3, 64, 0), b"min_inliers"), ((ONE_DEGREE, 0.01, 3, 0, 0), b"max_hypotheses"),
                       ((ONE_DEGREE, 0.01, 3, 65, 0), b"max_hypotheses"), ((ONE_DEGREE, 0.01, 3, 64, 2), b"flag"), ((ONE_DEGREE, 0.01, 3, 64, -1), b"flag")):
        assert call(*args) == L.ERR_INVALID_ARGUMENT, args
        assert word in L.lib().c2b_last_error() and list(counts) == [-7] * 6 and removed.value == -7, (args, L.lib().c2b_last_error())
        assert _bits(ba.points(), before) and ba.num_observations() == len(P["pt_idx"])
    for kw in (dict(min_angle_deg=91.0), dict(min_inliers=1), dict(max_hypotheses=65)):
        with pytest.raises(c2b.City2baError) as ei:
            ba.triangulate_points_robust(RR.MAX_ERROR, drop_outliers=True, **kw)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(c2b.City2baError):
        ba.triangulate_points_robust(-1.0)
    L.check(L.lib().c2b_problem_set_shard(ba._h, 0, ba.num_cameras() + 5, 0))       # a shard is refused
    assert call(ONE_DEGREE, 0.01, 3, 64, 1) == L.ERR_INVALID_ARGUMENT
    assert b"shard" in L.lib().c2b_last_error() and list(counts) == [-7] * 6
    assert _bits(ba.points(), before) and ba.num_observations() == len(P["pt_idx"])
    ba.close()
    ba = _load(P)                                                # the refused handle's twin still triangulates
    assert ba.triangulate_points_robust(RR.MAX_ERROR)["triangulated"] > 250
    ba.close()


def test_a_problem_without_observations_returns_too_few_and_writes_nothing(env):
    import city2ba_amd as c2b
    P = T.dome_case(False, 0.0)
    n_cam = len(P["bal9"])
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)), device=0)
    before = ba.points()
    out, status, hyp, inlier = ba.triangulate_points_robust(RR.MAX_ERROR, drop_outliers=True, return_status=True, return_inliers=True)
    assert (status == RR.TOO_FEW).all() and (hyp == -1).all() and len(inlier) == 0
    assert {k: out[k] for k in RR.STATUS} == RR.counts_of(status) and out["too_few"] == len(P["pts"]) and out["outliers"] == out["removed"] == 0
    assert _bits(ba.points(), before)
    ba.close()
