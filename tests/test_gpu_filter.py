"""Outlier rejection on the device (BAProblem.filter_observations / c2b_problem_filter_observations) against
tests/_filterref.py: the filtered lists index for index and bit for bit on dome_problem (ragged rows, mixed k2, duplicated
pairs; bal and state mode; with points behind their cameras), around every count edge of the launch, with NaN and infinite
observations; the state a filter leaves is the state of a problem uploaded with the filtered lists; what belongs to the
entities survives; bad arguments change nothing; and solve.solve_filtered is the pipeline run by hand."""
import ctypes as C

import numpy as np
import pytest

import _filterref as F
from test_gpu_schur_step import _bits, _make, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
INF = float("inf")
SIGMA = 1e-2                                 # the observation noise of "small grid culled" (tests/test_gpu_schur_step.py)
# the end-to-end run: reject beyond 10 sigma (the issue's bound); the Cauchy scale is 2 sigma -- an inlier's |r| is Rayleigh
# with that sigma, so 86 % of the inliers keep a weight above 1/2 while a wrong match (|r| of the order of the image) gets ~1e-3
E2E = dict(max_error=10 * SIGMA, loss="cauchy", loss_scale=2 * SIGMA)


def _load(P):
    import city2ba_amd as c2b
    if P.get("bal", True):
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    return c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


def _same_lists(ba, rows, pi, uv):
    assert ba.num_observations() == len(pi)
    assert _bits(ba.row_ptr, rows) and _bits(ba.pt_idx, pi), "row_ptr / pt_idx differ from the reference"
    assert _bits(ba.observations().reshape(-1, 2), uv.reshape(-1, 2)), "the observations' bits differ from the reference"


def _filter_and_check(P, max_error, in_front=False):
    keep, rows, pi, uv, removed = F.case_reference(P, max_error, in_front)
    ba = _load(P)
    got = ba.filter_observations(max_error, in_front=in_front)
    print("FILTER n_obs %d max_error %.6g in_front %d: removed %d (reference %d)" % (len(keep), max_error, in_front, got, removed))
    assert got == removed
    _same_lists(ba, rows, pi, uv)
    assert ba.num_cameras() == len(P["row_ptr"]) - 1 and ba.num_points() == len(P["pts"])       # nothing renumbered
    return ba, removed


# ---- 1. dome_problem --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup,state,behind", F.DOME_CASES)
def test_dome_lists_equal_the_reference(env, dup, state, behind):
    P = F.dome_case(dup, state, behind)
    for t in P["thresholds"]:
        counts = []
        for in_front in (False, True):
            ba, removed = _filter_and_check(P, t, in_front)
            ba.close()
            counts.append(removed)
        assert 0 < counts[0] < len(P["pt_idx"])
        # the moved points' exact observations pass the residual test and fall to the in-front test alone
        assert counts[1] - counts[0] == (F.BEHIND if behind else 0), counts
    if behind:                                               # r2 == 0 == max_error^2 exactly: `<=` keeps those six and nothing else
        ba, removed = _filter_and_check(P, 0.0)
        assert ba.num_observations() == F.BEHIND
        ba.close()


def test_level0_mask_is_the_reference_mask(env):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = F.dome_case(True, False, True)
    ba = _load(P)
    ex = ba.export_device()
    camblk = D.cameras_prepare_bal(torch.from_numpy(ba.cameras_bal()).to(dev))
    rows = D.Rows(ex["row_ptr"], ex["n_obs"])
    for t in P["thresholds"] + (0.0, INF):
        for in_front in (False, True):
            keep = torch.full((ex["n_obs"] + 64,), 7, dtype=torch.uint8, device=dev)
            D.residual_keep_rows(camblk, ex["pts4"], rows, ex["pt_idx"], ex["uv"], t, keep, in_front=in_front)
            torch.cuda.synchronize()
            got = _np(keep)
            assert np.array_equal(got[:ex["n_obs"]].astype(bool), F.keep_mask(P["r2"], P["qz"], t, in_front)), (t, in_front)
            assert set(np.unique(got[:ex["n_obs"]])) <= {0, 1} and np.all(got[ex["n_obs"]:] == 7)    # bytes 0 / 1, nothing past the end
    ba.close()


# ---- 2. count edges of the launch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obs", F.COUNT_EDGES)
def test_count_edges(env, n_obs):
    P = F.count_case(n_obs)
    for t in ([P["threshold"]] if P["threshold"] is not None else []) + [INF, 0.0]:
        ba, removed = _filter_and_check(P, t)
        if t == INF:
            assert removed == 0
        if t == 0.0:
            assert removed == n_obs and ba.num_observations() == 0 and not ba.row_ptr.any()
            assert ba.total_reprojection_error(2.0) == 0.0 and ba.filter_observations(1.0) == 0     # an empty list: 0
        ba.close()


# ---- 3. NaN and infinite observations; inf with finite data -----------------------------------------------------------------
def test_nan_and_infinite_observations_are_removed(env):
    P = dict(F.dome_case(True, False))
    n = len(P["pt_idx"])
    i, j = 5, n - 3
    uv = P["uv"].copy()
    uv[i] = np.nan
    uv[j, 0] = np.inf
    P["uv"] = uv
    P["r2"], P["qz"] = F.residuals(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], uv)
    assert np.isnan(P["r2"][i]) and np.isinf(P["r2"][j])
    big = 1e3                                                # finite, above every finite residual: exactly those two go
    keep = F.keep_mask(P["r2"], P["qz"], big)
    assert not keep[i] and not keep[j] and keep.sum() == n - 2
    ba, removed = _filter_and_check(P, big)
    assert removed == 2
    ba.close()
    ba, removed = _filter_and_check(P, INF)                  # inf <= inf: the reference keeps the infinite one; the NaN goes
    assert removed == 1
    ba.close()


def test_inf_with_finite_data_removes_nothing(env):
    P = F.dome_case(True, False)
    ba = _load(P)
    assert ba.filter_observations(INF) == 0 and ba.filter_observations(INF, in_front=True) == 0
    _same_lists(ba, P["row_ptr"], P["pt_idx"], P["uv"])
    ba.close()


# ---- 4. the state after a filter --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_state_after_a_filter_is_an_upload_of_the_filtered_lists(env, which):
    import city2ba_amd as c2b
    P = F.dome_case(True, False)
    t = P["thresholds"][which]
    _, rows, pi, uv, removed = F.case_reference(P, t)
    ba = _load(P)
    ba.total_reprojection_error(2.0)
    ba.normal_equations()
    ba.solve_step(1e-2)                                      # rows, transpose and solve buffers of the OLD list exist
    assert ba.filter_observations(t) == removed
    twin = c2b.BAProblem.from_bal(P["bal9"], P["pts"], rows, pi, uv, device=0)
    assert ba.total_reprojection_error(2.0) == twin.total_reprojection_error(2.0)
    a, b = ba.normal_equations(), twin.normal_equations()
    for x, y in zip(a[:4], b[:4]):
        assert _bits(_np(x), _np(y))
    assert a[4] == b[4]
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    assert np.abs(_np(dc)).max() > 0.0
    ba.close()
    twin.close()


# ---- 5. what survives -------------------------------------------------------------------------------------------------------
def test_masks_loss_preconditioner_and_checkpoint_survive(env):
    import _solvecheck as SC
    torch, dev = env["torch"], env["dev"]
    P = F.dome_case(True, False)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    ba.set_constant(cm, pm)
    ba.set_loss("cauchy", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.checkpoint()
    b0, p0, c0 = ba.cameras_bal(), ba.points(), ba.cameras()
    want_c, want_p = ba.constant()
    assert want_c.any() and want_p.any()
    ba.set_constant(None, None)                              # so that the step below moves every entry ...
    rng = np.random.default_rng(5)
    ba.apply_step(torch.from_numpy(rng.normal(scale=1e-4, size=b0.shape)).to(dev), torch.from_numpy(rng.normal(scale=1e-4, size=p0.shape)).to(dev))
    ba.set_constant(cm, pm)                                  # ... and the masks are in force across the filter
    assert not _bits(ba.cameras_bal(), b0) and not _bits(ba.points(), p0)
    t = P["thresholds"][1]
    removed = ba.filter_observations(t)                      # at the moved state: some go, whichever they are
    assert 0 < removed < len(P["pt_idx"])
    got_c, got_p = ba.constant()
    assert _bits(got_c, want_c) and _bits(got_p, want_p)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    ba.rollback()
    assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), p0) and _bits(ba.cameras(), c0)
    ba.close()


def test_a_filter_that_removes_nothing_changes_nothing(env):
    P = F.dome_case(True, False)
    ba = _load(P)
    dc, dp, info = ba.solve_step(1e-2)
    dc, dp = _np(dc).copy(), _np(dp).copy()
    n = C.c_int64(-1)
    from city2ba_amd import _lib as L
    assert L.lib().c2b_problem_filter_observations(ba._h, INF, 0, C.byref(n)) == 0 and n.value == 0
    assert ba.filter_observations(INF, in_front=True) == 0
    dc2, dp2, info2 = ba.solve_step(1e-2)
    assert _bits(_np(dc2), dc) and _bits(_np(dp2), dp) and info2 == info
    _same_lists(ba, P["row_ptr"], P["pt_idx"], P["uv"])
    ba.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_problem_unchanged(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    P = F.dome_case(True, False)
    ba = _load(P)
    t = P["thresholds"][0]
    for bad in (-1.0, -0.0 - 1e-300, float("nan"), -INF):
        with pytest.raises(c2b.City2baError) as ei:
            ba.filter_observations(bad)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT, bad
        _same_lists(ba, P["row_ptr"], P["pt_idx"], P["uv"])
    n = C.c_int64(-1)
    for flags in (2, 3, 0x100, -2):                          # an unknown flag bit
        assert L.lib().c2b_problem_filter_observations(ba._h, t, flags, C.byref(n)) == L.ERR_INVALID_ARGUMENT and n.value == 0
        assert b"flag" in L.lib().c2b_last_error()
    assert L.lib().c2b_problem_filter_observations(None, t, 0, None) == L.ERR_INVALID_ARGUMENT
    nc = ba.num_cameras()
    L.check(L.lib().c2b_problem_set_shard(ba._h, 0, nc + 5, 0))                # a shard is refused
    assert L.lib().c2b_problem_filter_observations(ba._h, t, 0, C.byref(n)) == L.ERR_INVALID_ARGUMENT and n.value == 0
    assert b"shard" in L.lib().c2b_last_error()
    sizes = [C.c_int64() for _ in range(3)]
    L.check(L.lib().c2b_problem_sizes(ba._h, *[C.byref(s) for s in sizes]))
    assert sizes[2].value == len(P["pt_idx"])
    _same_lists(ba, P["row_ptr"], P["pt_idx"], P["uv"])
    ba.close()
    ba = _load(P)                                            # Level 0 refuses the same arguments
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ex = ba.export_device()
    camblk = D.cameras_prepare_bal(torch.from_numpy(ba.cameras_bal()).to(dev))
    rows = D.Rows(ex["row_ptr"], ex["n_obs"])
    keep = torch.zeros(ex["n_obs"], dtype=torch.uint8, device=dev)
    for bad in (-1.0, float("nan")):
        with pytest.raises(c2b.City2baError) as ei:
            D.residual_keep_rows(camblk, ex["pts4"], rows, ex["pt_idx"], ex["uv"], bad, keep)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    assert ba.filter_observations(t) == F.case_reference(P, t)[4]               # the refused handle's twin still filters
    ba.close()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def corrupted_problem():
    """"small grid culled" (observation noise SIGMA) with 5 % wrong matches; (problem, labels): labels[o] = observation o's
    point index was changed"""
    from city2ba_amd import noise as N
    g, _ = _make("small grid culled")
    before = g.pt_idx.copy()
    ba = N.add_incorrect_correspondences(g, 0.05, seed=1)
    g.close()
    return ba, ba.pt_idx != before


def test_solve_filtered_is_the_pipeline_by_hand(env):
    from city2ba_amd import solve
    ba, labels = corrupted_problem()
    n = ba.num_observations()
    assert 0 < labels.sum() < n
    hand, _ = corrupted_problem()
    solve.levenberg_marquardt(hand, loss=E2E["loss"], loss_scale=E2E["loss_scale"])        # the Python loop, then the reference filter
    before = hand.total_reprojection_error(2.0) ** 2
    keep, rows, pi, uv, removed = F.reference(hand.cameras(), hand.points(), hand.row_ptr, hand.pt_idx, hand.observations(), E2E["max_error"])
    hand.close()

    solves, counts = solve.solve_filtered(ba, rounds=1, **E2E)
    assert len(solves) == 2 and counts == [removed]
    _same_lists(ba, rows, pi, uv)                            # the removed sets are identical
    assert ba.loss[0] is None                                # the last solve cleared the loss
    gone = ~keep
    hit = int((gone & labels).sum())
    recall, precision = hit / labels.sum(), hit / max(int(gone.sum()), 1)
    final = solves[-1][1]["final_cost"]
    print("FILTER end to end: %d observations, %d corrupted, %d removed (%d corrupted): recall %.4f precision %.4f; sum |r|^2 %.6g before the filter, %.6g final"
          % (n, labels.sum(), gone.sum(), hit, recall, precision, before, final))
    assert hit >= 1
    assert final == ba.total_reprojection_error(2.0) ** 2 or abs(final - ba.total_reprojection_error(2.0) ** 2) <= 1e-12 * final
    assert final < before
    ba.close()
