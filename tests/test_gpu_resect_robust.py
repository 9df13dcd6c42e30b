"""Consensus resection on the device (BAProblem.resect_cameras_robust / c2b_problem_resect_consensus /
c2b_resect_consensus_rows) against tests/_resectrobustref.py: status, selected triple, inlier count and inlier
mask with == and the poses within the refit's own bounds on the wrong-match dome (rows of 0 to 257 observations: every chunk
and window edge of a 64-lane wave, wrong matches on both sides of entry 64, duplicated pairs, mixed k2; bal and state mode)
and on the hand-placed edge set; the hypothesis cap; the refit bit for bit plain resection of the inliers; determinism and
the Level-0 entry; the list after drop_outliers and the state around it; refusals; and a solve from the robust start.
tests/test_resectrobustref.py asserts that no camera of these problems is excused, and every test here asserts it again on
the reference it compares with."""
import ctypes as C

import numpy as np
import pytest

import _resectref as T
import _resectrobustref as RR
import oracle as O
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)
from test_gpu_resect import _level0_inputs, _load

pytestmark = pytest.mark.gpu
_refs = {}


def _dome_reference(obs_noise, **kw):
    """the reference of the wrong-match dome at this observation noise, computed once per argument set: it reads the
    intrinsics, the points and the list, which the mode and the starting pose do not touch"""
    key = (obs_noise, tuple(sorted(kw.items())))
    if key not in _refs:
        P = RR.wrong_match_dome_cameras(False, obs_noise)
        _refs[key] = RR.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], RR.MAX_ERROR, **kw)
        assert _refs[key]["excused"] == [], _refs[key]["excused"]
    return _refs[key]


def _check(ba, ref, before, out, status, hyp, n_inl, inlier, tag):
    """before: bal9 rows"""
    after = ba.cameras_bal()
    assert np.array_equal(status, ref["status"]), (tag, np.flatnonzero(status != ref["status"]), status[status != ref["status"]])
    assert np.array_equal(hyp, ref["hyp"]), (tag, np.flatnonzero(hyp != ref["hyp"]), hyp[hyp != ref["hyp"]], ref["hyp"][hyp != ref["hyp"]])
    assert np.array_equal(n_inl, ref["n_inl"]), (tag, np.flatnonzero(n_inl != ref["n_inl"]))
    assert np.array_equal(inlier, ref["inlier"]), (tag, np.flatnonzero(inlier != ref["inlier"]))
    ok = status == RR.OK
    Rd, td = T.pose_of(O.camera_from_bal(np.ascontiguousarray(after)))     # from_bal of the written row
    eR = np.abs((Rd[ok].astype(T.LD) - ref["R"][ok]).astype(np.float64)).max(axis=(1, 2)) if ok.any() else np.zeros(1)
    et = np.linalg.norm((td[ok].astype(T.LD) - ref["t"][ok]).astype(np.float64), axis=1) if ok.any() else np.zeros(1)
    oR, ot = (eR / ref["bound_R"][ok], et / ref["bound_t"][ok]) if ok.any() else (np.zeros(1), np.zeros(1))
    print("RESECT ROBUST %s: %s; worst |R - R_ref| %.3g (%.3g of its bound), worst |t - t_ref| %.3g (%.3g of its bound)"
          % (tag, out, eR.max(), oR.max(), et.max(), ot.max()))
    assert (oR <= 1.0).all() and (ot <= 1.0).all(), (tag, float(oR.max()), float(ot.max()))
    assert _bits(after[:, 6:9], before[:, 6:9]), (tag, "an intrinsic moved")
    assert _bits(after[~ok], before[~ok]), (tag, "a camera whose status is not 0 moved")
    counts = {k: out[k] for k in RR.STATUS}
    assert counts == RR.counts_of(status) == ref["counts"], (tag, out)
    assert out["outliers"] == int((inlier == 0).sum()) and out["removed"] == 0
    return after


def _run(ba, **kw):
    return ba.resect_cameras_robust(RR.MAX_ERROR, return_status=True, return_inliers=True, **kw)


# ---- 1. the wrong-match dome --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,obs_noise", RR.DOME_CASES)
def test_dome_matches_the_reference(env, state, obs_noise):
    P = RR.wrong_match_dome_cameras(state, obs_noise)
    ref = _dome_reference(obs_noise)
    ba = _load(P)
    before = ba.cameras_bal()
    out, status, hyp, n_inl, inlier = _run(ba)
    _check(ba, ref, before, out, status, hyp, n_inl, inlier, "dome state=%d obs_noise=%g" % (state, obs_noise))
    ok = status == RR.OK
    assert out["resected"] >= 57 and out["too_few"] == 18 and out["outliers"] > 300
    assert not (inlier == 0)[~P["wrong"]].any()                  # no right observation is dropped
    Rt, _ = T.pose_of(O.camera_from_bal(P["true_bal9"]))
    Rd, _ = T.pose_of(ba.cameras())
    assert T.rotation_angle_deg(Rd[ok], Rt[ok]).max() < (0.2 if obs_noise == 0.0 else 2.0)
    ba.close()


@pytest.mark.parametrize("state", [False, True])
def test_the_result_does_not_depend_on_the_starting_pose(env, state):
    outs = []
    for seed in (17, 18):
        ba = _load(RR.wrong_match_dome_cameras(state, 1e-3, start_seed=seed))
        outs.append(_run(ba) + (ba.cameras_bal(),))
        ba.close()
    ok = outs[0][1] == RR.OK
    assert outs[0][0] == outs[1][0] and all(_bits(outs[0][k], outs[1][k]) for k in (1, 2, 3, 4)) and _bits(outs[0][5][ok], outs[1][5][ok])
    assert not _bits(outs[0][5][~ok][:, :6], outs[1][5][~ok][:, :6])           # the kept cameras are the two starts'


def test_the_hypothesis_cap(env):
    P = RR.wrong_match_dome_cameras(False, 1e-3)
    ref, full = _dome_reference(1e-3, max_hypotheses=4), _dome_reference(1e-3)
    assert (ref["hyp"] < 4).all() and not np.array_equal(ref["hyp"], full["hyp"])             # the cap decides something here
    ba = _load(P)
    before = ba.cameras_bal()
    out, status, hyp, n_inl, inlier = _run(ba, max_hypotheses=4)
    _check(ba, ref, before, out, status, hyp, n_inl, inlier, "dome max_hypotheses=4")
    ba.close()


def test_the_refit_is_plain_resection_of_the_inliers_bit_for_bit(env):
    import city2ba_amd as c2b
    P = RR.wrong_match_dome_cameras(False, 1e-3)
    ba = _load(P)
    out, status, hyp, n_inl, inlier = _run(ba)
    got = ba.cameras_bal()
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], inlier.astype(bool))
    plain = c2b.BAProblem.from_bal(P["bal9"], P["pts"], rp, ri, ruv, device=0)
    _, s_plain = plain.resect_cameras(return_status=True)
    ok = status == RR.OK
    assert ok.sum() >= 57 and (s_plain[ok] == T.OK).all()
    assert _bits(got[ok], plain.cameras_bal()[ok])
    plain.close()
    ba.close()


# ---- 2. the edge set and the camera mask --------------------------------------------------------------------------------
def test_edge_set(env):
    P = RR.edge_problem()
    ref = RR.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], RR.MAX_ERROR, cam_mask=P["cam_mask"])
    assert ref["excused"] == []
    want_status, want_hyp, want_n, zeros = RR.edge_expected()
    assert np.array_equal(ref["status"], want_status)
    ba = _load(P)
    ba.set_constant(cameras=P["cam_mask"])
    before = ba.cameras_bal()
    out, status, hyp, n_inl, inlier = _run(ba)
    _check(ba, ref, before, out, status, hyp, n_inl, inlier, "edge set")
    assert np.array_equal(status, want_status) and all(hyp[c] == k for c, k in want_hyp.items()) and all(n_inl[c] == k for c, k in want_n.items())
    assert hyp[RR.EDGE["collinear_first"]] > 0 and hyp[RR.EDGE["coplanar"]] >= 0
    assert np.array_equal(np.flatnonzero(inlier == 0), zeros)
    ba.close()


def test_pose_bits_keep_a_camera_and_the_rest_is_the_unmasked_run(env):
    P = RR.wrong_match_dome_cameras(False, 1e-3)
    free = _load(P)
    _, s_free, h_free, n_free, i_free = _run(free)
    b_free = free.cameras_bal()
    free.close()
    rows = np.diff(P["row_ptr"].astype(np.int64))
    long = np.flatnonzero(rows >= 6)
    held, intr_only = long[[0, 5, 20, 40]], long[[1, 6, 21]]
    mask = np.zeros(len(rows), dtype=np.uint16)
    mask[held] = 0x001, 0x020, 0x03f, 0x1ff
    mask[intr_only] = 0x040, 0x180, 0x1c0
    ba = _load(P)
    before = ba.cameras_bal()
    ba.set_constant(cameras=mask)
    out, status, hyp, n_inl, inlier = _run(ba)
    after = ba.cameras_bal()
    rest = np.ones(len(rows), dtype=bool)
    rest[held] = False
    assert (status[held] == RR.CONSTANT).all() and (hyp[held] == -1).all() and (n_inl[held] == 0).all() and out["constant"] == len(held)
    assert np.array_equal(status[rest], s_free[rest]) and np.array_equal(hyp[rest], h_free[rest]) and np.array_equal(n_inl[rest], n_free[rest])
    assert _bits(after[held], before[held]) and _bits(after[rest], b_free[rest])
    cam_of = np.repeat(np.arange(len(rows)), rows)
    of_held = ~rest[cam_of]
    assert (inlier[of_held] == 1).all() and np.array_equal(inlier[~of_held], i_free[~of_held])
    ba.close()


# ---- 3. determinism and Level 0 -----------------------------------------------------------------------------------------
def test_two_handles_give_the_same_bits(env):
    P = RR.wrong_match_dome_cameras(True, 1e-3)
    outs = []
    for _ in range(2):
        ba = _load(P)
        outs.append(_run(ba) + (ba.cameras_bal(), ba.cameras()))
        ba.close()
    assert outs[0][0] == outs[1][0] and all(_bits(a, b) for a, b in zip(outs[0][1:], outs[1][1:]))


@pytest.mark.parametrize("state", [False, True])
def test_level0_gives_the_problem_level_bits(env, state):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = RR.wrong_match_dome_cameras(state, 1e-3)
    ba = _load(P)
    bal9, pts4, rows, pt_idx, uv = _level0_inputs(env, ba)
    n, no = rows.n_cam, rows.n_obs
    status = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    hyp = torch.full((n + 64,), -7, dtype=torch.int32, device=dev)
    n_inl = torch.full((n + 64,), -7, dtype=torch.int32, device=dev)
    inlier = torch.full((no + 64,), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((8,), -1, dtype=torch.int64, device=dev)
    bal9 = torch.cat([bal9, torch.full((8, 9), 7.25, dtype=torch.float64, device=dev)])
    lengths = np.diff(P["row_ptr"].astype(np.int64))
    mask = np.zeros(n, dtype=np.uint16)
    mask[np.flatnonzero(lengths >= 6)[[2, 30]]] = 0x008, 0x1c7
    D.resect_consensus_rows(bal9, pts4, rows, pt_idx, uv, status, counts, RR.MAX_ERROR, cam_mask=torch.from_numpy(mask.view(np.int16)).to(dev),
                            hyp=hyp, n_inl=n_inl, inlier=inlier)
    torch.cuda.synchronize()
    status, hyp, n_inl, inlier, bal9 = _np(status), _np(hyp), _np(n_inl), _np(inlier), _np(bal9)
    counts = _np(counts)
    assert (counts[6:] == -1).all()
    assert (status[n:] == 9).all() and (hyp[n:] == -7).all() and (n_inl[n:] == -7).all() and (inlier[no:] == 9).all() and (bal9[n:] == 7.25).all()
    ba.set_constant(cameras=mask)
    out, want_status, want_hyp, want_n, want_inlier = _run(ba)
    assert _bits(status[:n], want_status) and _bits(hyp[:n], want_hyp) and _bits(n_inl[:n], want_n) and _bits(inlier[:no], want_inlier)
    assert dict(zip(RR.STATUS, (int(v) for v in counts[:6]))) == {k: out[k] for k in RR.STATUS} and out["constant"] == 2
    assert _bits(bal9[:n], ba.cameras_bal())
    ba.close()


def test_level0_without_the_optional_outputs(env):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = RR.wrong_match_dome_cameras(False, 1e-3)
    ba = _load(P)
    bal9, pts4, rows, pt_idx, uv = _level0_inputs(env, ba)
    status = torch.zeros(rows.n_cam, dtype=torch.uint8, device=dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    D.resect_consensus_rows(bal9, pts4, rows, pt_idx, uv, status, counts, RR.MAX_ERROR)
    torch.cuda.synchronize()
    out, want = ba.resect_cameras_robust(RR.MAX_ERROR, return_status=True)[:2]
    assert _bits(_np(status), want) and _bits(_np(bal9), ba.cameras_bal())
    ba.close()


# ---- 4. drop_outliers and the state around the call ---------------------------------------------------------------------
def test_drop_outliers_compacts_the_list_by_the_mask_and_leaves_an_uploads_state(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    P = RR.wrong_match_dome_cameras(False, 1e-3)
    ref = _dome_reference(1e-3)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    cm = (cm & ~np.uint16(T.POSE_BITS)).astype(np.uint16)        # intrinsics bits only: every camera is still resected
    ba.set_constant(cm, pm)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-2)                                          # rows, transpose and solve buffers of the OLD list exist
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    out, status, hyp, n_inl, inlier = _run(ba, drop_outliers=True)
    assert np.array_equal(status, ref["status"]) and np.array_equal(inlier, ref["inlier"])
    zeros = int((inlier == 0).sum())
    assert out["removed"] == out["outliers"] == zeros > 300
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], inlier.astype(bool))
    assert ba.num_observations() == len(ri) == len(P["pt_idx"]) - zeros
    assert _bits(ba.row_ptr, rp) and _bits(ba.pt_idx, ri) and _bits(ba.observations().reshape(-1, 2), ruv)
    assert ba.num_cameras() == len(P["bal9"]) and ba.num_points() == len(P["pts"])             # nothing renumbered
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    b1 = ba.cameras_bal()
    assert not _bits(b1, b0) and _bits(ba.points(), p0)
    twin = c2b.BAProblem.from_bal(b1, p0, rp, ri, ruv, device=0)
    twin.set_constant(cm, pm)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    assert ba.total_reprojection_error(2.0) == twin.total_reprojection_error(2.0)
    twin.close()
    ba.rollback()                                                # the checkpoint taken before the call rolls the cameras back
    assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), p0)
    assert ba.num_observations() == len(ri)                      # (the list is not part of a checkpoint)
    ba.close()


def test_drop_outliers_with_nothing_to_drop_changes_no_list(env):
    P = T.dome_case(False, 0.0)                                  # exact observations, no wrong match
    ba = _load(P)
    out = ba.resect_cameras_robust(RR.MAX_ERROR, drop_outliers=True)
    assert out["outliers"] == 0 and out["removed"] == 0 and out["resected"] == 63
    assert ba.num_observations() == len(P["pt_idx"]) and _bits(ba.pt_idx, P["pt_idx"])
    ba.close()


def test_without_drop_outliers_the_list_and_the_settings_stay_and_the_checkpoint_rolls_back(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    P = RR.wrong_match_dome_cameras(False, 1e-3)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    cm = (cm & ~np.uint16(T.POSE_BITS)).astype(np.uint16)
    ba.set_constant(cm, pm)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-2)
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    out = ba.resect_cameras_robust(RR.MAX_ERROR)
    assert out["resected"] >= 57 and out["removed"] == 0
    b1 = ba.cameras_bal()
    assert not _bits(b1, b0) and _bits(ba.points(), p0)
    assert ba.num_observations() == len(P["pt_idx"]) and _bits(ba.pt_idx, P["pt_idx"])
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    twin = c2b.BAProblem.from_bal(b1, p0, P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    twin.set_constant(cm, pm)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    twin.close()
    ba.rollback()
    assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), p0)
    ba.close()


def test_state_mode_becomes_bal_mode_as_after_a_camera_step(env):
    import city2ba_amd as c2b
    P = RR.wrong_match_dome_cameras(True, 1e-3)
    ba = _load(P)
    ba.resect_cameras_robust(RR.MAX_ERROR)
    twin = c2b.BAProblem.from_bal(ba.cameras_bal(), P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    assert _bits(ba.cameras(), twin.cameras())                   # the state is from_vec of bal9: bal9 is the truth
    twin.close()
    ba.close()


# ---- 5. refusals, no observations ---------------------------------------------------------------------------------------
def test_refusals_leave_the_problem_unchanged(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = RR.wrong_match_dome_cameras(False, 1e-3)
    ba = _load(P)
    before = ba.cameras_bal()
    counts = (C.c_int64 * 6)(*([-7] * 6))
    removed = C.c_int64(-7)
    call = lambda err, mi, gap, mh, flags: L.lib().c2b_problem_resect_consensus(ba._h, err, mi, gap, mh, flags, None, None, None, None, counts,
                                                                                C.byref(removed))
    inf, nan = float("inf"), float("nan")
    for args, word in (((-1e-300, 6, 1e-4, 64, 0), b"max_error"), ((nan, 6, 1e-4, 64, 0), b"max_error"), ((inf, 6, 1e-4, 64, 0), b"max_error"),
                       ((0.01, 5, 1e-4, 64, 0), b"min_inliers"), ((0.01, -3, 1e-4, 64, 0), b"min_inliers"), ((0.01, 6, -1e-9, 64, 0), b"min_gap"),
                       ((0.01, 6, nan, 64, 0), b"min_gap"), ((0.01, 6, 1.0, 64, 0), b"min_gap"), ((0.01, 6, 1e-4, 0, 0), b"max_hypotheses"),
                       ((0.01, 6, 1e-4, 65, 0), b"max_hypotheses"), ((0.01, 6, 1e-4, 64, 2), b"flag"), ((0.01, 6, 1e-4, 64, -1), b"flag")):
        assert call(*args) == L.ERR_INVALID_ARGUMENT, args
        assert word in L.lib().c2b_last_error() and list(counts) == [-7] * 6 and removed.value == -7, (args, L.lib().c2b_last_error())
        assert _bits(ba.cameras_bal(), before) and ba.num_observations() == len(P["pt_idx"])
    for kw in (dict(min_inliers=5), dict(min_gap=1.0), dict(max_hypotheses=65)):
        with pytest.raises(c2b.City2baError) as ei:
            ba.resect_cameras_robust(RR.MAX_ERROR, drop_outliers=True, **kw)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(c2b.City2baError):
        ba.resect_cameras_robust(-1.0)
    assert L.lib().c2b_problem_resect_consensus(None, 0.01, 6, 1e-4, 64, 0, None, None, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    L.check(L.lib().c2b_problem_set_shard(ba._h, 0, ba.num_cameras() + 5, 0))       # a shard is refused
    assert call(0.01, 6, 1e-4, 64, 1) == L.ERR_INVALID_ARGUMENT
    assert b"shard" in L.lib().c2b_last_error() and list(counts) == [-7] * 6
    assert _bits(ba.cameras_bal(), before) and ba.num_observations() == len(P["pt_idx"])
    ba.close()
    ba = _load(P)                                                # Level 0 refuses the same values
    bal9, pts4, rows, pt_idx, uv = _level0_inputs(env, ba)
    st, cn = torch.zeros(rows.n_cam, dtype=torch.uint8, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
    for args, kw in (((RR.MAX_ERROR,), dict(min_inliers=5)), ((RR.MAX_ERROR,), dict(min_gap=-1.0)), ((RR.MAX_ERROR,), dict(max_hypotheses=0)),
                     ((nan,), dict())):
        with pytest.raises(c2b.City2baError) as ei:
            D.resect_consensus_rows(bal9, pts4, rows, pt_idx, uv, st, cn, *args, **kw)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert _bits(_np(bal9), before)
    assert ba.resect_cameras_robust(RR.MAX_ERROR)["resected"] >= 57          # the refused handle's twin still resects
    ba.close()


def test_a_problem_without_observations_returns_too_few_and_writes_nothing(env):
    import city2ba_amd as c2b
    P = T.dome_case(False, 0.0)
    n_cam = len(P["bal9"])
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)), device=0)
    before = ba.cameras_bal()
    out, status, hyp, n_inl, inlier = _run(ba, drop_outliers=True)
    assert (status == RR.TOO_FEW).all() and (hyp == -1).all() and (n_inl == 0).all() and len(inlier) == 0
    assert {k: out[k] for k in RR.STATUS} == RR.counts_of(status) and out["too_few"] == n_cam and out["outliers"] == out["removed"] == 0
    assert _bits(ba.cameras_bal(), before)
    ba.close()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------
def test_a_solve_from_the_robust_start_on_the_filtered_list_ends_lower_than_from_plain_resection(env):
    """RR.e2e_problem: _resectref.e2e_problem with a tenth of every row's matches swapped.  Ten iterations with the points
    and the intrinsics constant: from resect_cameras_robust(drop_outliers=True) on the list it leaves, against the same
    loop from resect_cameras() on the unfiltered list.  The ordering is asserted first for the host loop alone
    (T.host_cameras_lm from the references' poses); the device's final cost from the robust start is within 10 % (DESIGN
    4.6's margin) of the host loop's from the reference's poses on the reference's filtered list."""
    import city2ba_amd as c2b
    from city2ba_amd import solve
    import _solvecheck as SC
    P = RR.e2e_problem()
    cams15 = O.camera_from_bal(P["bal9"])
    ref = RR.reference(cams15, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], RR.MAX_ERROR, bound=False)
    assert ref["excused"] == []
    plain = T.reference(cams15, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], bound=False)
    rp, ri, ruv = RR.restrict(P["row_ptr"], P["pt_idx"], P["uv"], ref["inlier"].astype(bool))
    F = dict(P, row_ptr=rp, pt_idx=ri, uv=ruv)
    host_rob, _ = T.host_cameras_lm(dict(F, bal9=T.resected_bal9(P["bal9"], ref)), 10)
    host_plain, _ = T.host_cameras_lm(dict(P, bal9=T.resected_bal9(P["bal9"], plain)), 10)
    print("RESECT ROBUST e2e reference: %s, plain %s; host loop from the robust poses on the filtered list %.6g -> %.6g, from plain "
          "resection on the whole list %.6g -> %.6g" % (ref["counts"], T.counts_of(plain["status"]), host_rob[0], host_rob[-1], host_plain[0], host_plain[-1]))
    assert host_plain[-1] > 100.0 * host_rob[-1]                 # the ordering holds for the reference alone, widely

    fixed = (np.full(len(P["bal9"]), SC.INTRINSICS, dtype=np.uint16), np.ones(len(P["pts"]), dtype=bool))

    def load():
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    ba = load()
    ba.resect_cameras()
    _, s_plain = solve.levenberg_marquardt_device(ba, iterations=10, constant=fixed)
    ba.close()
    ba = load()
    out, status, hyp, n_inl, inlier = _run(ba, drop_outliers=True)
    assert np.array_equal(status, ref["status"]) and np.array_equal(inlier, ref["inlier"]) and out["removed"] == int((ref["inlier"] == 0).sum())
    _, s_rob = solve.levenberg_marquardt_device(ba, iterations=10, constant=fixed)
    ba.close()
    print("RESECT ROBUST e2e device: %s; final cost from plain resection %.6g, from the robust start %.6g -> %.6g"
          % (out, s_plain["final_cost"], s_rob["initial_cost"], s_rob["final_cost"]))
    assert abs(s_rob["final_cost"] - host_rob[-1]) <= 0.1 * host_rob[-1]
    assert s_rob["final_cost"] < s_plain["final_cost"]
