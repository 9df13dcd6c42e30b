"""Triangulation on the device (BAProblem.triangulate_points / c2b_problem_triangulate_points / c2b_triangulate_rows, DESIGN
4.9) against tests/_triangref.py: status for status and point by point within the reference's own bound on dome_problem
(ragged rows from 0 to more than 64 observations, two workgroups with a tail, mixed k2, duplicated pairs; bal and state
mode) and on the hand-placed edge set; masks and refusals; determinism; the Level-0 entry; what survives the call and that
nothing stale stays cached; a solve from the triangulated start; and the figures the reference gives for it.
tests/test_triangref.py asserts, with the oracle's numbers, that no point of these problems sits at the parallax threshold,
so every point's status is compared."""
import ctypes as C

import numpy as np
import pytest

import _triangref as T
from test_gpu_schur_step import _bits, _make, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
ONE_DEGREE = float(np.deg2rad(1.0))


def _load(P):
    import city2ba_amd as c2b
    if P.get("bal", True):
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    return c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


def _reference(ba, min_angle=ONE_DEGREE, **kw):
    """the reference on the device's own cameras (the state it holds, downloaded)"""
    cams = ba.cameras()
    return T.reference(cams, T.centers_of(cams), ba.row_ptr, ba.pt_idx, ba.observations().reshape(-1, 2), ba.num_points(), min_angle, **kw)


def _check(ba, ref, before, counts, status, tag):
    after = ba.points()
    assert np.array_equal(status, ref["status"]), (tag, np.flatnonzero(status != ref["status"]), status[status != ref["status"]])
    ok = status == T.OK
    err = np.linalg.norm((after[ok].astype(T.LD) - ref["X"][ok]).astype(np.float64), axis=1)
    over = err / ref["bound"][ok] if ok.any() else np.zeros(1)
    print("TRIANGULATE %s: %s; worst |X - X_ref| %.3g, worst |err| / bound %.3g (point %d)"
          % (tag, counts, err.max() if ok.any() else 0.0, over.max(), int(np.flatnonzero(ok)[over.argmax()]) if ok.any() else -1))
    assert (over <= 1.0).all(), (tag, float(over.max()))
    assert _bits(after[~ok], before[~ok]), (tag, "a point whose status is not 0 moved")
    assert counts == T.counts_of(status), (tag, counts)
    return after


# ---- 1. dome_problem ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,obs_noise", T.DOME_CASES)
def test_dome_matches_the_reference_point_by_point(env, state, obs_noise):
    P = T.dome_case(state, obs_noise)
    ba = _load(P)
    before = ba.points()
    ref = _reference(ba)
    assert len(T.cap_violations(ref)) == 0
    counts, status = ba.triangulate_points(return_status=True)
    after = _check(ba, ref, before, counts, status, "dome state=%d obs_noise=%g" % (state, obs_noise))
    ok = status == T.OK
    assert counts["triangulated"] > 200 and counts["too_few"] >= 60 and counts["constant"] == 0
    far = np.linalg.norm(after[ok] - P["true_pts"][ok], axis=1)
    assert far.max() < (1e-9 if obs_noise == 0.0 else 0.5)      # from 0.5 away to the truth (to the noise's reach)
    assert ba.triangulate_points() == counts                     # without the status array
    ba.close()


# ---- 2. the edge set ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [1.0, 0.1])
def test_edge_set(env, deg):
    P = T.edge_problem()
    ba = _load(P)
    before = ba.points()
    ref = _reference(ba, float(np.deg2rad(deg)))
    assert np.array_equal(ref["status"], T.edge_expected(deg))
    counts, status = ba.triangulate_points(min_angle_deg=deg, return_status=True)
    _check(ba, ref, before, counts, status, "edge set at %g degrees" % deg)
    assert np.array_equal(status, T.edge_expected(deg))
    ba.close()


# ---- 3. masks and bad arguments -----------------------------------------------------------------------------------------
def test_constant_points_keep_their_bits_and_the_rest_is_the_unmasked_run(env):
    from _problems import DOME_CROWDED
    P = T.dome_case(False, 1e-3)
    free = _load(P)
    _, s_free = free.triangulate_points(return_status=True)
    x_free = free.points()
    free.close()
    mask = np.zeros(len(P["pts"]), dtype=bool)
    mask[[DOME_CROWDED, 5, 100, 255, 256, 379, 399]] = True
    ba = _load(P)
    before = ba.points()
    ba.set_constant(points=mask)
    counts, status = ba.triangulate_points(return_status=True)
    after = ba.points()
    assert (status[mask] == T.CONSTANT).all() and (status[~mask] == s_free[~mask]).all() and counts["constant"] == mask.sum()
    assert _bits(after[mask], before[mask]) and _bits(after[~mask], x_free[~mask])
    assert counts == T.counts_of(status)
    got_c, got_p = ba.constant()
    assert np.array_equal(got_p.astype(bool), mask)
    ba.close()


def test_refusals_leave_the_problem_unchanged(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    P = T.dome_case(False, 1e-3)
    ba = _load(P)
    before = ba.points()
    counts = (C.c_int64 * 5)(*([-7] * 5))
    for bad in (-1.0, float("nan"), 2.0, -1e-300, float("inf")):
        assert L.lib().c2b_problem_triangulate_points(ba._h, bad, None, counts) == L.ERR_INVALID_ARGUMENT, bad
        assert b"min_angle" in L.lib().c2b_last_error() and list(counts) == [-7] * 5
        assert _bits(ba.points(), before)
    for bad_deg in (-1.0, float("nan"), 91.0):
        with pytest.raises(c2b.City2baError) as ei:
            ba.triangulate_points(min_angle_deg=bad_deg)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    assert L.lib().c2b_problem_triangulate_points(None, 0.1, None, None) == L.ERR_INVALID_ARGUMENT
    L.check(L.lib().c2b_problem_set_shard(ba._h, 0, ba.num_cameras() + 5, 0))       # a shard is refused
    assert L.lib().c2b_problem_triangulate_points(ba._h, ONE_DEGREE, None, counts) == L.ERR_INVALID_ARGUMENT
    assert b"shard" in L.lib().c2b_last_error() and list(counts) == [-7] * 5
    assert _bits(ba.points(), before)
    ba.close()
    ba = _load(P)                                                # Level 0 refuses the same angles
    torch, D, dev = env["torch"], env["D"], env["dev"]
    camblk, pts4, rows, prows, pt_idx, uv = _level0_inputs(env, ba, True)
    st, cn = torch.zeros(prows.n_pts, dtype=torch.uint8, device=dev), torch.zeros(5, dtype=torch.int64, device=dev)
    for bad in (-1.0, float("nan"), 2.0):
        with pytest.raises(c2b.City2baError) as ei:
            D.triangulate_rows(camblk, pts4, prows, uv, st, cn, bad)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    assert ba.triangulate_points()["triangulated"] > 200           # the refused handle's twin still triangulates
    ba.close()


def test_a_problem_without_observations_returns_too_few_and_writes_nothing(env):
    import city2ba_amd as c2b
    P = T.dome_case(False, 0.0)
    n_cam = len(P["bal9"])
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)), device=0)
    before = ba.points()
    counts, status = ba.triangulate_points(return_status=True)
    assert (status == T.TOO_FEW).all() and counts == T.counts_of(status) and counts["too_few"] == len(P["pts"])
    assert _bits(ba.points(), before)
    ba.close()


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
def test_two_handles_give_the_same_bits(env):
    P = T.dome_case(True, 1e-3)
    out = []
    for _ in range(2):
        ba = _load(P)
        counts, status = ba.triangulate_points(return_status=True)
        out.append((counts, status, ba.points()))
        ba.close()
    assert out[0][0] == out[1][0] and _bits(out[0][1], out[1][1]) and _bits(out[0][2], out[1][2])


# ---- 5. Level 0 ---------------------------------------------------------------------------------------------------------
def _level0_inputs(env, ba, bal):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ex = ba.export_device()
    camblk = D.cameras_prepare_bal(torch.from_numpy(ba.cameras_bal()).to(dev)) if bal else D.cameras_prepare_state(ex["cam15"])
    rows = D.Rows(ex["row_ptr"], ex["n_obs"])
    prows = D.PointRows(rows, ex["pt_idx"], ba.num_points())
    return camblk, ex["pts4"], rows, prows, ex["pt_idx"], ex["uv"]


@pytest.mark.parametrize("state", [False, True])
def test_level0_gives_the_problem_level_bits(env, state):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = T.dome_case(state, 1e-3)
    ba = _load(P)
    camblk, pts4, rows, prows, pt_idx, uv = _level0_inputs(env, ba, not state)
    n = prows.n_pts
    pts4 = pts4.clone()
    pts4[:, 3] = 7.25                                            # the fourth lane keeps its value
    status = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    mask = np.zeros(n, dtype=np.uint8)
    mask[[3, 300]] = 1
    D.triangulate_rows(camblk, pts4, prows, uv, status, counts, ONE_DEGREE, pt_mask=torch.from_numpy(mask).to(dev))
    torch.cuda.synchronize()
    ba.set_constant(points=mask.astype(bool))
    want_counts, want_status = ba.triangulate_points(return_status=True)
    got = _np(pts4)
    assert _bits(_np(status)[:n], want_status) and (_np(status)[n:] == 9).all()
    assert dict(zip(T.STATUS, (int(v) for v in _np(counts)))) == want_counts
    assert _bits(got[:, :3], ba.points()) and (got[:, 3] == 7.25).all()
    ba.close()


# ---- 6. the state around the call ---------------------------------------------------------------------------------------
def test_checkpoint_masks_loss_and_preconditioner_survive_and_nothing_stale_stays(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    P = T.dome_case(False, 1e-3)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    ba.set_constant(cm, pm)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-2)                                          # rows, transpose and solve buffers exist
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    counts = ba.triangulate_points()
    assert counts["triangulated"] > 200 and counts["constant"] == pm.sum()
    p1 = ba.points()
    assert not _bits(p1, p0) and _bits(ba.cameras_bal(), b0)
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    # a solve_step after the call is the solve_step of a fresh handle uploaded with the triangulated points
    twin = c2b.BAProblem.from_bal(b0, p1, P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    twin.set_constant(cm, pm)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    assert np.abs(_np(dp)).max() > 0.0
    twin.close()
    ba.rollback()                                                # the checkpoint taken before the call
    assert _bits(ba.points(), p0) and _bits(ba.cameras_bal(), b0)
    ba.close()


def test_state_mode_stays_state_mode(env):
    P = T.dome_case(True, 1e-3)
    ba = _load(P)
    c0 = ba.cameras()
    ba.triangulate_points()
    assert _bits(ba.cameras(), c0)
    ba.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------
def test_a_solve_from_the_triangulated_start_ends_lower_than_from_the_noisy_points(env):
    """ "small grid culled" with point noise T.E2E_POINT_STD (the grid's blocks are 5 long: points land behind their
    cameras and in other blocks).  Ten iterations with every camera constant from the noisy points end at a higher cost
    than the same solve from triangulate_points().  The noise is one at which the reference alone shows that ordering:
    T.host_points_lm (the host loop of _solvecheck.host_lm with the cameras constant: host_lm itself frees the cameras, and
    the 9 parameters per camera it fits put its optimum below any the constant-camera solve can reach) from the noisy
    points against the same loop from the reference's triangulation -- asserted first.  The device's final cost from the
    triangulated start is within 10 % of that host loop's from the same start."""
    from city2ba_amd import noise as N
    from city2ba_amd import solve
    import _solvecheck as SC

    def noisy():
        ba, _ = _make("small grid culled")
        return N.add_noise(ba, 0.0, 0.0, T.E2E_POINT_STD, 0.0, seed=9)
    ba = noisy()
    P = dict(bal9=ba.cameras_bal(), pts=ba.points(), row_ptr=ba.row_ptr.copy(), pt_idx=ba.pt_idx.copy(), uv=ba.observations().reshape(-1, 2).copy())
    ref = _reference(ba, bound=False)
    assert len(T.cap_violations(ref)) == 0
    ok = ref["status"] == T.OK
    tri = np.where(ok[:, None], ref["X"].astype(np.float64), P["pts"])
    host_noisy, _ = T.host_points_lm(P, 10)
    host_tri, _ = T.host_points_lm(dict(P, pts=tri), 10)
    print("TRIANGULATE e2e reference: %d of %d points triangulated; host loop from the noisy points %.6g -> %.6g, from the triangulated ones %.6g -> %.6g"
          % (ok.sum(), len(ok), host_noisy[0], host_noisy[-1], host_tri[0], host_tri[-1]))
    assert host_noisy[-1] > host_tri[-1]                         # the ordering holds for the reference alone

    fixed = (np.full(ba.num_cameras(), SC.ALL, dtype=np.uint16), None)
    _, s_noisy = solve.levenberg_marquardt_device(ba, iterations=10, constant=fixed)
    ba.close()
    ba = noisy()
    counts, status = ba.triangulate_points(return_status=True)
    assert np.array_equal(status, ref["status"])
    start = ba.points()
    _, s_tri = solve.levenberg_marquardt_device(ba, iterations=10, constant=fixed)
    ba.close()
    host_same, _ = T.host_points_lm(dict(P, pts=start), 10)
    full = SC.host_lm(dict(P, pts=start), 10)
    print("TRIANGULATE e2e device: %s; final cost from the noisy points %.6g, from the triangulated ones %.6g -> %.6g; host loop from the same start %.6g (with the cameras free: %.6g)"
          % (counts, s_noisy["final_cost"], s_tri["initial_cost"], s_tri["final_cost"], host_same[-1], full[-1]))
    assert s_noisy["final_cost"] > s_tri["final_cost"]
    assert abs(s_tri["final_cost"] - host_same[-1]) <= 0.1 * host_same[-1]
