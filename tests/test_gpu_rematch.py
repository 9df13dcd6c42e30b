"""Guided re-matching on the device (BAProblem.rematch_observations / c2b_problem_rematch_observations / c2b_rematch_rows,
DESIGN 4.15) against tests/_rematchref.py with ==: choice, status, the counts and the list after the call, through both
levels, on the dome with wrong labels and on the hand-built edge set (tests/test_rematchref.py lists it and holds the
reference to the outputs written out); and the state around the call.  The device's projection is bit-exact with the
oracle's, so no tolerance enters; the reference reports every observation with a decision within CAP of its threshold, and
every comparison demands that there is none."""
import ctypes as C
import functools

import numpy as np
import pytest

import _rematchref as R
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)
from test_gpu_triangulate import _level0_inputs, _load

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _dome(state, obs_noise):
    return R.wrong_label_dome(state, obs_noise)


def _state(ba):
    """the device's own state, downloaded: what the reference runs on"""
    return ba.cameras(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations().reshape(-1, 2).copy()


def _level0(env, ba, bal, radius, max_error, trusted):
    """c2b_rematch_rows on the handle's exported state, fits from c2b_residual_keep_rows: (choice, status, counts), with canaries
    past every output's end"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    camblk, pts4, rows, prows, pt_idx, uv = _level0_inputs(env, ba, bal)
    n = rows.n_obs
    before = pts4.clone(), pt_idx.clone(), uv.clone()
    fits = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    D.residual_keep_rows(camblk, pts4, rows, pt_idx, uv, max_error, fits, in_front=True)
    choice = torch.full((n + 64,), -7, dtype=torch.int32, device=dev)
    status = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((4 + 8,), -1, dtype=torch.int64, device=dev)
    t = None if trusted is None else torch.from_numpy(np.asarray(trusted, dtype=np.uint8)).to(dev)
    D.rematch_rows(camblk, pts4, rows, pt_idx, uv, fits, choice, status, counts, radius, max_error, pt_trusted=t)
    torch.cuda.synchronize()
    choice, status, counts, fits = _np(choice), _np(status), _np(counts), _np(fits)
    assert (choice[n:] == -7).all() and (status[n:] == 9).all() and (counts[4:] == -1).all() and (fits[n:] == 9).all()      # nothing past the end
    assert _bits(_np(pts4), _np(before[0])) and _bits(_np(pt_idx), _np(before[1])) and _bits(_np(uv), _np(before[2]))      # inputs only read
    return choice[:n], status[:n], counts[:4], fits[:n]


def _both_levels_equal_the_reference(env, ba, bal, radius, max_error, min_fits, on_purpose=(), tag=""):
    """Level 0 (given the reference's trusted bytes; at min_fits = 0 also with NULL) and Level 1 against the reference on the
    device's own state; returns (reference, device dict)"""
    cams, pts, row_ptr, pt_idx, uv = _state(ba)
    ref = R.reference(cams, pts, row_ptr, pt_idx, uv, radius, max_error, min_fits, on_purpose=on_purpose)
    assert ref["excused"] == [], (tag, "a decision within CAP of its threshold", ref["excused"][:10])
    for trusted in [ref["trusted"]] + ([None] if min_fits == 0 else []):
        choice, status, counts, fits = _level0(env, ba, bal, radius, max_error, trusted)
        assert np.array_equal(fits.astype(bool), ref["fits"]), (tag, np.flatnonzero(fits.astype(bool) != ref["fits"])[:10])
        assert np.array_equal(choice, ref["choice"]), (tag, np.flatnonzero(choice != ref["choice"])[:10])
        assert np.array_equal(status, ref["status"]), (tag, np.flatnonzero(status != ref["status"])[:10])
        assert dict(zip(R.STATUS, (int(v) for v in counts))) == ref["counts"], tag
    out, status = ba.rematch_observations(radius, max_error, min_fits=min_fits, return_status=True)
    print("REMATCH %s: device %s" % (tag, out))
    assert out == ref["counts"], (tag, out, ref["counts"])
    assert status.dtype == np.uint8 and np.array_equal(status, ref["status"]), (tag, np.flatnonzero(status != ref["status"])[:10])
    assert np.array_equal(ba.pt_idx.astype(np.uint64), ref["pt_idx"]), tag
    assert _bits(ba.row_ptr.astype(np.uint64), ref["row_ptr"]) and _bits(ba.observations().reshape(-1, 2), ref["uv"]), tag
    assert ba.num_observations() == len(ref["pt_idx"]) and ba.num_points() == len(pts) and _bits(ba.points(), pts) and _bits(ba.cameras(), cams), tag
    return ref, out


# ---- 1. the dome ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,obs_noise", R.DOME_CASES)
def test_both_levels_equal_the_reference_on_the_dome(env, state, obs_noise):
    P = _dome(state, obs_noise)
    ba = _load(P)
    ref, out = _both_levels_equal_the_reference(env, ba, not state, P["radius"], R.MAX_ERROR, R.MIN_FITS, tag="dome state=%s noise=%g" % (state, obs_noise))
    assert out["reassigned"] > 300 and out["removed"] > 10 and out["skipped"] > 10 and len(ref["several"]) > 10
    true = P["true_pt_idx"].astype(np.int64)[ref["keep"]]
    assert (ba.pt_idx.astype(np.int64) == true).sum() > (P["pt_idx"] == P["true_pt_idx"]).sum() + 300      # the labels came back
    ba.close()


# ---- 2. the edge set -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", R.EDGE_RUNS)
def test_both_levels_equal_the_reference_on_the_edge_set(env, name, variant):
    P, radius, max_error, min_fits, on_purpose = R.edge_run(name, variant)
    ba = _load(P)
    ref, _ = _both_levels_equal_the_reference(env, ba, False, radius, max_error, min_fits, on_purpose=on_purpose, tag="%s/%s" % (name, variant))
    status, choice = P["want"][variant]                          # and the outputs written out
    assert np.array_equal(ref["status"], status) and np.array_equal(ref["choice"], choice)
    ba.close()


def test_no_observations_launch_nothing_and_count_nothing(env):
    import city2ba_amd as c2b
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = _dome(False, 0.0)
    n_cam = len(P["bal9"])
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)), device=0)
    out, status = ba.rematch_observations(0.5, 1e-2, return_status=True)
    assert out == dict(fits=0, skipped=0, reassigned=0, removed=0) and len(status) == 0 and _bits(ba.points(), P["pts"])
    ba.close()
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    rows = D.Rows(torch.zeros(n_cam + 1, dtype=torch.int64, device=dev), 0)
    pts4 = torch.zeros((5, 4), dtype=torch.float64, device=dev)
    D.rematch_rows(None, pts4, rows, None, None, None, None, None, counts, 0.5, 1e-2)
    torch.cuda.synchronize()
    assert _np(counts).tolist() == [0, 0, 0, 0]


# ---- 3. the state around the call ------------------------------------------------------------------------------------------
def test_masks_priors_loss_preconditioner_and_checkpoint_survive_and_nothing_stale_stays(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    P = _dome(False, 1e-3)
    ba = _load(P)
    cm = np.zeros(len(P["bal9"]), dtype=np.uint16)
    cm[:3] = 0x1c0                                               # f, k1, k2 of three cameras
    pm = np.zeros(len(P["pts"]), dtype=bool)
    pm[[7, 300]] = True
    cw = np.zeros((len(P["bal9"]), 3))
    cw[5] = 0.25
    ba.set_constant(cm, pm)
    ba.set_priors(camera_center_weights=cw)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-2)                                          # rows, transpose and solve buffers of the OLD list exist
    ba.checkpoint()
    b0, p0, n0 = ba.cameras_bal(), ba.points(), ba.num_observations()
    pri0 = ba.priors
    out = ba.rematch_observations(P["radius"], R.MAX_ERROR)
    assert out["reassigned"] > 300 and out["removed"] > 10 and ba.num_observations() == n0 - out["removed"]
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    pri1 = ba.priors
    assert all(_bits(pri1[k], pri0[k]) for k in pri0 if k != "active") and pri1["active"] == pri0["active"]
    assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), p0)
    twin = c2b.BAProblem.from_bal(b0, p0, ba.row_ptr, ba.pt_idx, ba.observations().reshape(-1, 2), device=0)
    twin.set_constant(cm, pm)
    twin.set_priors(camera_centers=pri0["camera_centers"], camera_center_weights=cw)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)      # the list's caches were rebuilt, not reused
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    assert ba.total_reprojection_error(2.0) == twin.total_reprojection_error(2.0)
    twin.close()
    # a second call on the result changes nothing and moves no bit, and the next step is the last one
    i1, r1, u1 = ba.pt_idx.copy(), ba.row_ptr.copy(), ba.observations().copy()
    again = ba.rematch_observations(P["radius"], R.MAX_ERROR)
    assert again["reassigned"] == 0 and again["removed"] == 0 and again["fits"] + again["skipped"] == len(i1)
    assert _bits(ba.pt_idx, i1) and _bits(ba.row_ptr, r1) and _bits(ba.observations(), u1) and _bits(ba.points(), p0)
    dc3, dp3, info3 = ba.solve_step(1e-2)
    assert _bits(_np(dc3), _np(dc)) and _bits(_np(dp3), _np(dp)) and info3 == info
    ba.apply_step(dc3, dp3)
    ba.rollback()                                                # the checkpoint taken before the call: the entities of then, the list of now
    assert _bits(ba.points(), p0) and _bits(ba.cameras_bal(), b0) and _bits(ba.pt_idx, i1)
    ba.close()


def test_labels_alone_change_when_nothing_is_removed(env):
    """a call that reassigns and removes nothing keeps the count, the row pointer and the pixels, and still rebuilds what was
    derived from the list"""
    import city2ba_amd as c2b
    P, radius, max_error, min_fits, _ = R.edge_run("swaps", "base")
    ba = _load(P)
    ba.solve_step(1e-2)
    out = ba.rematch_observations(radius, max_error, min_fits=min_fits)
    assert out["reassigned"] == 7 and out["removed"] == 0
    assert _bits(ba.row_ptr.astype(np.uint64), P["row_ptr"]) and _bits(ba.observations().reshape(-1, 2), P["uv"])
    assert not np.array_equal(ba.pt_idx.astype(np.uint64), P["pt_idx"])
    twin = c2b.BAProblem.from_visibility(ba.cameras(), ba.points(), ba.row_ptr, ba.pt_idx, ba.observations().reshape(-1, 2), device=0)
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2
    twin.close()
    ba.close()


def test_two_calls_on_equal_inputs_give_equal_bits(env):
    P = _dome(True, 1e-3)
    res = []
    for _ in range(2):
        ba = _load(P)
        out, status = ba.rematch_observations(P["radius"], R.MAX_ERROR, return_status=True)
        res.append((out, status, ba.pt_idx.copy(), ba.row_ptr.copy(), ba.observations().copy()))
        ba.close()
    assert res[0][0] == res[1][0] and all(_bits(a, b) for a, b in zip(res[0][1:], res[1][1:]))


def test_refusals_leave_the_problem_unchanged(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    P = _dome(False, 0.0)
    ba = _load(P)
    before = ba.points()
    reassigned, removed = C.c_int64(-7), C.c_int64(-7)
    call = lambda radius, err, min_fits: L.lib().c2b_problem_rematch_observations(ba._h, radius, err, min_fits, None, C.byref(reassigned), C.byref(removed))
    inf, nan = float("inf"), float("nan")
    for args, word in (((-1.0, 1e-2, 2), b"radius"), ((nan, 1e-2, 2), b"radius"), ((inf, 1e-2, 2), b"radius"), ((0.5, -1e-300, 2), b"max_error"),
                       ((0.5, nan, 2), b"max_error"), ((0.5, inf, 2), b"max_error"), ((0.5, 1e-2, -1), b"min_fits")):
        assert call(*args) == L.ERR_INVALID_ARGUMENT, args
        assert word in L.lib().c2b_last_error() and reassigned.value == -7 and removed.value == -7, (args, L.lib().c2b_last_error())
        assert _bits(ba.points(), before) and _bits(ba.pt_idx, P["pt_idx"]) and ba.num_observations() == len(P["pt_idx"])
    with pytest.raises(c2b.City2baError) as ei:
        ba.rematch_observations(0.5, 1e-2, min_fits=-1)
    assert ei.value.status == L.ERR_INVALID_ARGUMENT
    L.check(L.lib().c2b_problem_set_shard(ba._h, 0, ba.num_cameras() + 5, 0))       # a shard is refused
    assert call(0.5, 1e-2, 2) == L.ERR_INVALID_ARGUMENT and b"shard" in L.lib().c2b_last_error() and reassigned.value == -7
    assert _bits(ba.points(), before)
    ba.close()
