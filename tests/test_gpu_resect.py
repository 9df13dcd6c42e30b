"""Resection on the device (BAProblem.resect_cameras / c2b_problem_resect_cameras / c2b_resect_rows) against
tests/_resectref.py: status for status and camera by camera within the reference's own bounds on dome_problem (rows of 0 to
257 observations: every chunk edge of a 64-lane wave, empty rows, duplicated pairs, mixed k2; bal and state mode; exact and
noisy observations) and on the hand-placed edge set; the camera mask and refusals; determinism and independence of the
starting pose; the Level-0 entry; what survives the call; and a solve from the resected start against the reference's
figures.  tests/test_resectref.py asserts on the CPU that no camera of these problems sits at a threshold, and each test
here asserts it on the problem it compares statuses on, so every camera's status is compared."""
import ctypes as C

import numpy as np
import pytest

import _resectref as T
import oracle as O
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
_refs = {}


def _load(P):
    import city2ba_amd as c2b
    if P.get("bal", True):
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    return c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


def _dome_reference(obs_noise):
    """the reference of the dome at this observation noise, computed once: it reads the intrinsics, the points and the
    observations, which the mode and the starting pose do not touch"""
    if obs_noise not in _refs:
        P = T.dome_case(False, obs_noise)
        _refs[obs_noise] = T.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
        assert len(T.cap_violations(_refs[obs_noise])) == 0
    return _refs[obs_noise]


def _check(after, ref, before, counts, status, tag):
    """after / before: bal9 rows"""
    assert np.array_equal(status, ref["status"]), (tag, np.flatnonzero(status != ref["status"]), status[status != ref["status"]])
    ok = status == T.OK
    Rd, td = T.pose_of(O.camera_from_bal(np.ascontiguousarray(after)))     # from_bal of the written row: Rodrigues vectors are not unique at pi
    eR = np.abs((Rd[ok].astype(T.LD) - ref["R"][ok]).astype(np.float64)).max(axis=(1, 2)) if ok.any() else np.zeros(1)
    et = np.linalg.norm((td[ok].astype(T.LD) - ref["t"][ok]).astype(np.float64), axis=1) if ok.any() else np.zeros(1)
    oR, ot = (eR / ref["bound_R"][ok], et / ref["bound_t"][ok]) if ok.any() else (np.zeros(1), np.zeros(1))
    print("RESECT %s: %s; worst |R - R_ref| %.3g (%.3g of its bound), worst |t - t_ref| %.3g (%.3g of its bound)"
          % (tag, counts, eR.max(), oR.max(), et.max(), ot.max()))
    assert (oR <= 1.0).all() and (ot <= 1.0).all(), (tag, float(oR.max()), float(ot.max()))
    assert _bits(after[:, 6:9], before[:, 6:9]), (tag, "an intrinsic moved")
    assert _bits(after[~ok], before[~ok]), (tag, "a camera whose status is not 0 moved")
    assert counts == T.counts_of(status), (tag, counts)


# ---- 1. dome_problem ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,obs_noise", T.DOME_CASES)
def test_dome_matches_the_reference_camera_by_camera(env, state, obs_noise):
    P = T.dome_case(state, obs_noise)
    ref = _dome_reference(obs_noise)
    ba = _load(P)
    before = ba.cameras_bal()
    counts, status = ba.resect_cameras(return_status=True)
    after = ba.cameras_bal()
    _check(after, ref, before, counts, status, "dome state=%d obs_noise=%g" % (state, obs_noise))
    ok = status == T.OK
    assert counts == dict(resected=63, too_few=18, degenerate=0, behind=0, constant=0)
    Rt, _ = T.pose_of(O.camera_from_bal(P["true_bal9"]))
    Rd, _ = T.pose_of(ba.cameras())
    ang = T.rotation_angle_deg(Rd[ok], Rt[ok])
    assert ang.max() < (1e-5 if obs_noise == 0.0 else 1.0)       # from 0.3 rad away to the truth (to the noise's reach)
    assert ba.resect_cameras() == counts                         # without the status array, from the resected poses:
    assert _bits(ba.cameras_bal(), after)                        # the start does not enter
    ba.close()


@pytest.mark.parametrize("state", [False, True])
def test_the_result_does_not_depend_on_the_starting_pose(env, state):
    out = []
    for seed in (17, 18):
        ba = _load(T.dome_case(state, 1e-3, start_seed=seed))
        counts, status = ba.resect_cameras(return_status=True)    # (state mode: to_vec is made by the call itself)
        out.append((counts, status, ba.cameras_bal()))
        ba.close()
    ok = out[0][1] == T.OK
    assert out[0][0] == out[1][0] and _bits(out[0][1], out[1][1]) and _bits(out[0][2][ok], out[1][2][ok])
    assert not _bits(out[0][2][~ok][:, :6], out[1][2][~ok][:, :6])            # the kept cameras are the two starts'


# ---- 2. the edge set ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_gap", [1e-4, 1e-7])
def test_edge_set(env, min_gap):
    P = T.edge_problem()
    ref = T.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], min_gap=min_gap)
    assert np.array_equal(ref["status"], T.edge_expected(min_gap)) and len(T.cap_violations(ref)) == 0
    ba = _load(P)
    before = ba.cameras_bal()
    counts, status = ba.resect_cameras(min_gap=min_gap, return_status=True)
    _check(ba.cameras_bal(), ref, before, counts, status, "edge set at min_gap %g" % min_gap)
    assert np.array_equal(status, T.edge_expected(min_gap))
    ba.close()


# ---- 3. the mask and bad arguments --------------------------------------------------------------------------------------
def test_pose_bits_keep_a_camera_and_intrinsics_bits_do_not(env):
    P = T.dome_case(False, 1e-3)
    free = _load(P)
    _, s_free = free.resect_cameras(return_status=True)
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
    counts, status = ba.resect_cameras(return_status=True)
    after = ba.cameras_bal()
    rest = np.ones(len(rows), dtype=bool)
    rest[held] = False
    assert (status[held] == T.CONSTANT).all() and (status[intr_only] == T.OK).all() and np.array_equal(status[rest], s_free[rest])
    assert counts["constant"] == len(held) and counts == T.counts_of(status)
    assert _bits(after[held], before[held]) and _bits(after[rest], b_free[rest])
    got_c, _ = ba.constant()
    import _solvecheck as SC
    assert np.array_equal(got_c, SC.unpack(mask))
    ba.close()


def test_refusals_leave_the_problem_unchanged(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = T.dome_case(False, 1e-3)
    ba = _load(P)
    before = ba.cameras_bal()
    counts = (C.c_int64 * 5)(*([-7] * 5))
    for pts, gap, word in ((5, 1e-4, b"min_points"), (0, 1e-4, b"min_points"), (-3, 1e-4, b"min_points"), (6, -1e-9, b"min_gap"),
                           (6, float("nan"), b"min_gap"), (6, 1.0, b"min_gap"), (6, float("inf"), b"min_gap")):
        assert L.lib().c2b_problem_resect_cameras(ba._h, pts, gap, None, counts) == L.ERR_INVALID_ARGUMENT, (pts, gap)
        assert word in L.lib().c2b_last_error() and list(counts) == [-7] * 5
        assert _bits(ba.cameras_bal(), before)
    for kw in (dict(min_points=5), dict(min_gap=-1.0), dict(min_gap=float("nan")), dict(min_gap=1.0)):
        with pytest.raises(c2b.City2baError) as ei:
            ba.resect_cameras(**kw)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    assert L.lib().c2b_problem_resect_cameras(None, 6, 1e-4, None, None) == L.ERR_INVALID_ARGUMENT
    L.check(L.lib().c2b_problem_set_shard(ba._h, 0, ba.num_cameras() + 5, 0))       # a shard is refused
    assert L.lib().c2b_problem_resect_cameras(ba._h, 6, 1e-4, None, counts) == L.ERR_INVALID_ARGUMENT
    assert b"shard" in L.lib().c2b_last_error() and list(counts) == [-7] * 5
    assert _bits(ba.cameras_bal(), before)
    ba.close()
    ba = _load(P)                                                # Level 0 refuses the same values
    bal9, pts4, rows, pt_idx, uv = _level0_inputs(env, ba)
    st, cn = torch.zeros(rows.n_cam, dtype=torch.uint8, device=dev), torch.zeros(5, dtype=torch.int64, device=dev)
    for kw in (dict(min_points=5), dict(min_gap=-1.0), dict(min_gap=float("nan")), dict(min_gap=1.0)):
        with pytest.raises(c2b.City2baError) as ei:
            D.resect_rows(bal9, pts4, rows, pt_idx, uv, st, cn, **kw)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert _bits(_np(bal9), before)
    assert ba.resect_cameras()["resected"] == 63                 # the refused handle's twin still resects
    ba.close()


def test_a_problem_without_observations_returns_too_few_and_writes_nothing(env):
    import city2ba_amd as c2b
    P = T.dome_case(False, 0.0)
    n_cam = len(P["bal9"])
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)), device=0)
    before = ba.cameras_bal()
    counts, status = ba.resect_cameras(return_status=True)
    assert (status == T.TOO_FEW).all() and counts == T.counts_of(status) and counts["too_few"] == n_cam
    assert _bits(ba.cameras_bal(), before)
    ba.close()


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
def test_two_handles_give_the_same_bits(env):
    P = T.dome_case(True, 1e-3)
    out = []
    for _ in range(2):
        ba = _load(P)
        counts, status = ba.resect_cameras(return_status=True)
        out.append((counts, status, ba.cameras_bal(), ba.cameras()))
        ba.close()
    assert out[0][0] == out[1][0] and all(_bits(out[0][k], out[1][k]) for k in (1, 2, 3))


# ---- 5. Level 0 ---------------------------------------------------------------------------------------------------------
def _level0_inputs(env, ba):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ex = ba.export_device()
    rows = D.Rows(ex["row_ptr"], ex["n_obs"])
    return torch.from_numpy(ba.cameras_bal()).to(dev), ex["pts4"], rows, ex["pt_idx"], ex["uv"]


@pytest.mark.parametrize("state", [False, True])
def test_level0_gives_the_problem_level_bits(env, state):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = T.dome_case(state, 1e-3)
    ba = _load(P)
    bal9, pts4, rows, pt_idx, uv = _level0_inputs(env, ba)
    n = rows.n_cam
    status = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    lengths = np.diff(P["row_ptr"].astype(np.int64))
    mask = np.zeros(n, dtype=np.uint16)
    mask[np.flatnonzero(lengths >= 6)[[2, 30]]] = 0x008, 0x1c7
    D.resect_rows(bal9, pts4, rows, pt_idx, uv, status, counts, cam_mask=torch.from_numpy(mask.view(np.int16)).to(dev))
    torch.cuda.synchronize()
    ba.set_constant(cameras=mask)
    want_counts, want_status = ba.resect_cameras(return_status=True)
    assert _bits(_np(status)[:n], want_status) and (_np(status)[n:] == 9).all()
    assert dict(zip(T.STATUS, (int(v) for v in _np(counts)))) == want_counts and want_counts["constant"] == 2
    assert _bits(_np(bal9), ba.cameras_bal())
    ba.close()


# ---- 6. the state around the call ---------------------------------------------------------------------------------------
def test_checkpoint_masks_loss_and_preconditioner_survive_and_nothing_stale_stays(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    P = T.dome_case(False, 1e-3)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    cm = (cm & ~np.uint16(T.POSE_BITS)).astype(np.uint16)        # intrinsics bits only: every camera is still resected
    ba.set_constant(cm, pm)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-2)                                          # rows, transpose and solve buffers exist
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    counts = ba.resect_cameras()
    assert counts["resected"] == 63 and counts["constant"] == 0
    b1 = ba.cameras_bal()
    assert not _bits(b1, b0) and _bits(ba.points(), p0)
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    # a solve_step after the call is the solve_step of a fresh handle uploaded with the resected cameras
    twin = c2b.BAProblem.from_bal(b1, p0, P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    twin.set_constant(cm, pm)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    assert np.abs(_np(dc)).max() > 0.0
    twin.close()
    ba.rollback()                                                # the checkpoint taken before the call
    assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), p0)
    ba.close()


def test_state_mode_becomes_bal_mode_as_after_a_camera_step(env):
    import city2ba_amd as c2b
    P = T.dome_case(True, 1e-3)
    ba = _load(P)
    ba.resect_cameras()
    b1 = ba.cameras_bal()
    twin = c2b.BAProblem.from_bal(b1, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    assert _bits(ba.cameras(), twin.cameras())                   # the state is from_vec of bal9: bal9 is the truth
    twin.close()
    ba.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------
def test_a_solve_from_the_resected_start_ends_lower_than_from_the_noisy_poses(env):
    """T.e2e_problem: every twelfth camera of the parity grid, true points, observation noise 1e-3, pose noise 0.3 rad /
    1.0.  Ten iterations with the points and the intrinsics constant from the noisy poses end at a higher cost than the
    same solve from resect_cameras().  The noise is one at which the reference alone shows that ordering with a wide gap:
    T.host_cameras_lm (the host loop of _solvecheck.host_lm with the points and intrinsics constant) from the noisy poses
    against the same loop from the reference's resection -- asserted first.  The device's final cost from the resected
    start is within 10 % of that host loop's from the same start."""
    import city2ba_amd as c2b
    from city2ba_amd import solve
    import _solvecheck as SC
    P = T.e2e_problem()

    def load():
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    ref = T.reference(O.camera_from_bal(P["bal9"]), P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], bound=False)
    assert len(T.cap_violations(ref)) == 0
    host_noisy, _ = T.host_cameras_lm(P, 10)
    host_res, _ = T.host_cameras_lm(dict(P, bal9=T.resected_bal9(P["bal9"], ref)), 10)
    print("RESECT e2e reference: %s; host loop from the noisy poses %.6g -> %.6g, from the resected ones %.6g -> %.6g"
          % (T.counts_of(ref["status"]), host_noisy[0], host_noisy[-1], host_res[0], host_res[-1]))
    assert host_noisy[-1] > 100.0 * host_res[-1]                 # the ordering holds for the reference alone, widely

    fixed = (np.full(len(P["bal9"]), SC.INTRINSICS, dtype=np.uint16), np.ones(len(P["pts"]), dtype=bool))
    ba = load()
    _, s_noisy = solve.levenberg_marquardt_device(ba, iterations=10, constant=fixed)
    ba.close()
    ba = load()
    counts, status = ba.resect_cameras(return_status=True)
    assert np.array_equal(status, ref["status"])
    start = ba.cameras_bal()
    _, s_res = solve.levenberg_marquardt_device(ba, iterations=10, constant=fixed)
    ba.close()
    host_same, _ = T.host_cameras_lm(dict(P, bal9=start), 10)
    print("RESECT e2e device: %s; final cost from the noisy poses %.6g, from the resected ones %.6g -> %.6g; host loop from the same start %.6g"
          % (counts, s_noisy["final_cost"], s_res["initial_cost"], s_res["final_cost"], host_same[-1]))
    assert s_noisy["final_cost"] > s_res["final_cost"]
    assert abs(s_res["final_cost"] - host_same[-1]) <= 0.1 * host_same[-1]
