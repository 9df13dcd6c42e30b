"""Landmark merging on the device (BAProblem.merge_points / c2b_problem_merge_points / c2b_merge_partner_rows)
against tests/_mergeref.py with ==: the split dome is put back together (recovery), the device equals the reference bit for
bit where the reference merges truly, falsely and under jitter, through both levels; hand-built rows, clusters and cell
layouts at the edges of a wave and of the cell grid; and the state around the call.  The device's projection is bit-exact
with the oracle's, so no tolerance enters; a draw in which the reference meets a predicate value within 4 ulp of max_error^2
would be dropped and counted (none of these draws has one, and the tests assert that).

What cannot be observed through the interface -- that a call which merges nothing keeps the cached transpose -- is pinned by
its visible half: such a call changes no bit of the list or the points and the next solve step is the one before it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _mergeref as M
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)
from test_gpu_triangulate import _level0_inputs, _load

pytestmark = pytest.mark.gpu
RADIUS, MAX_ERROR = 0.5, 1e-4
# (jitter of the copies, max_error): (a) the recovery case, (b) a bound at which the reference merges falsely too, (c) moved twins
SETTINGS = {"recovery": (0.0, 1e-4), "false_merges": (0.0, 1e-2), "jitter": (1e-4, 1e-3)}


@functools.lru_cache(maxsize=None)
def _split(jitter):
    return M.split_dome(jitter=jitter)


def _state(ba):
    """the device's own state, downloaded: what the reference runs on"""
    return ba.cameras(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations().reshape(-1, 2)


def _level0(env, ba, bal, radius, max_error, held=None):
    """c2b_merge_partner_rows on the handle's exported state: (partner, status, counts) with canaries"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    camblk, pts4, rows, prows, pt_idx, uv = _level0_inputs(env, ba, bal)
    n = prows.n_pts
    before = pts4.clone()
    partner = torch.full((n + 64,), -7, dtype=torch.int32, device=dev)
    status = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    h = None if held is None else torch.from_numpy(np.asarray(held, dtype=np.uint8)).to(dev)
    D.merge_partner_rows(camblk, pts4, prows, uv, partner, status, counts, radius, max_error, pt_held=h)
    torch.cuda.synchronize()
    partner, status = _np(partner), _np(status)
    assert (partner[n:] == -7).all() and (status[n:] == 9).all() and _bits(_np(pts4), _np(before))      # nothing past the end, pts4 only read
    return partner[:n], status[:n], _np(counts)


def _both_levels_equal_the_reference(env, ba, bal, radius, max_error, rounds, held=None, tag=""):
    """Level 0 against one round, Level 1 against the loop; returns (reference of the loop, device dict, device map)"""
    cams, pts, row_ptr, pt_idx, uv = _state(ba)
    first = M.one_round(cams, pts, row_ptr, pt_idx, uv, radius, max_error, held)
    ref = M.merge(cams, pts, row_ptr, pt_idx, uv, radius, max_error, rounds, held)
    assert ref["borderline"] == 0, (tag, "a borderline draw: drop it")
    partner, status, counts = _level0(env, ba, bal, radius, max_error, held)
    assert np.array_equal(partner, first["partner"]), (tag, np.flatnonzero(partner != first["partner"])[:10])
    assert np.array_equal(status, first["status"]), (tag, np.flatnonzero(status != first["status"])[:10])
    assert dict(zip(M.STATUS, (int(v) for v in counts))) == first["counts"], tag
    out, into = ba.merge_points(radius, max_error, rounds=rounds, return_map=True)
    print("MERGE %s: device %s, reference per round %s, %d pairs rejected" % (tag, out, ref["per_round"], ref["rejected"]))
    assert out == dict(merged=ref["merged"], rounds=ref["rounds"]), (tag, out, ref["per_round"])
    assert into.dtype == np.int32 and np.array_equal(into, ref["map"]), (tag, np.flatnonzero(into != ref["map"])[:10])
    assert np.array_equal(ba.pt_idx.astype(np.int64), ref["pt_idx"]), tag
    assert _bits(ba.points(), ref["pts"]), tag
    assert _bits(ba.row_ptr, row_ptr) and _bits(ba.observations().reshape(-1, 2), uv) and ba.num_points() == len(pts), tag
    return ref, out, into


# ---- 1. recovery --------------------------------------------------------------------------------------------------------
def test_the_split_dome_is_put_back_together(env):
    S = _split(0.0)
    P, n0 = S["P"], S["n_orig"]
    assert 0 in S["both"] and len(S["both"]) > 80
    ba = _load(P)
    out, into = ba.merge_points(RADIUS, MAX_ERROR, rounds=2, return_map=True)
    want = np.arange(len(P["pts"]))
    for a in S["both"]:
        want[S["twin_of"][a]] = a                               # every split point with both halves seen, onto the lower index
    assert np.array_equal(into, want)
    assert out == dict(merged=len(S["both"]), rounds=2)          # the second round merges nothing
    lost = np.array([a for a in S["twin_of"] if a not in S["both"]] + [-1])
    differs = ba.pt_idx != S["orig_pt_idx"]
    assert np.isin(S["orig_pt_idx"][differs].astype(np.int64), lost).all() and differs.sum() < 60
    assert _bits(ba.points()[:n0], P["pts"][:n0]) and _bits(ba.points()[n0:], P["pts"][n0:])
    assert _bits(ba.observations().reshape(-1, 2), P["uv"]) and _bits(ba.row_ptr, P["row_ptr"])
    assert ba.num_points() == len(P["pts"]) and ba.num_observations() == len(P["pt_idx"])
    ba.close()


# ---- 2. equality with the reference, both levels ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_both_levels_equal_the_reference_on_the_split_dome(env, name):
    jitter, max_error = SETTINGS[name]
    S = _split(jitter)
    ba = _load(S["P"])
    ref, out, _ = _both_levels_equal_the_reference(env, ba, True, RADIUS, max_error, 2, tag=name)
    assert ref["rejected"] > 100                                 # candidates are refused in every setting
    if name == "false_merges":
        assert out["merged"] > len(S["both"]) and out["rounds"] == 2 and ref["per_round"][1] > 0
    if name == "jitter":
        assert out["merged"] == len(S["both"]) and not _bits(ba.points()[:S["n_orig"]], S["P"]["pts"][:S["n_orig"]])
    ba.close()


def test_state_mode_equals_the_reference_too(env):
    S = _split(0.0)
    P = dict(S["P"])
    P.update(bal=False)                                          # loaded from cams15 instead of bal9
    ba = _load(P)
    c0 = ba.cameras()
    _both_levels_equal_the_reference(env, ba, False, RADIUS, 1e-2, 1, tag="state mode")
    assert _bits(ba.cameras(), c0)
    ba.close()


# ---- 3. wave and cell edges, hand-built ------------------------------------------------------------------------------------
def _hand(env, cams, pts, views, radius, max_error, rounds=1, seen_at=None, bend=None, held=None, tag=""):
    """a hand-built problem in state mode through both levels; bend = (camera, point, du): that pixel moved"""
    import city2ba_amd as c2b
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    row_ptr, pt_idx, uv = M.observe(cams, pts if seen_at is None else seen_at, views)
    if bend is not None:
        cam_of = np.repeat(np.arange(len(cams)), np.diff(row_ptr.astype(np.int64)))
        hit = np.flatnonzero((cam_of == bend[0]) & (pt_idx == bend[1]))
        assert len(hit) == 1
        uv[hit[0], 0] += bend[2]
    ba = c2b.BAProblem.from_visibility(cams, pts, row_ptr, pt_idx, uv, device=0)
    if held is not None:
        ba.set_constant(points=np.asarray(held).astype(bool))
    ref, out, into = _both_levels_equal_the_reference(env, ba, False, radius, max_error, rounds, held=held, tag=tag)
    ba.close()
    return ref, out, into


X = np.array([0.25, -0.5, 0.125])


def test_rows_longer_than_a_wave(env):
    cams = M.simple_cameras(150)
    far = lambda k: X + [3.0 * k, 0, 0]
    pts = [far(0), far(0), far(1), far(1), far(2), far(2), far(3), far(3)]
    views = ([(c, 0) for c in range(75)] + [(c, 1) for c in range(75, 150)]                 # 75 / 75: the union exceeds a wave
             + [(c, 2) for c in range(130)] + [(130, 3)]                                    # 130 / 1: one row alone does
             + [(c, 4) for c in range(75)] + [(c, 5) for c in range(74, 149)]               # camera 74 is entry 74 of both rows
             + [(c, 6) for c in range(70)] + [(c, 7) for c in range(70, 140)])              # entry 139 of the union misses
    ref, out, into = _hand(env, cams, pts, views, RADIUS, MAX_ERROR, bend=(139, 7, 1e-2), tag="long rows")
    assert into.tolist() == [0, 0, 2, 2, 4, 5, 6, 7] and out["merged"] == 2 and ref["rejected"] == 2
    _, out, into = _hand(env, cams, pts, views, RADIUS, MAX_ERROR, tag="long rows, no bent pixel")
    assert into.tolist() == [0, 0, 2, 2, 4, 5, 6, 6]


def test_more_than_a_wave_of_candidates_is_scanned_before_the_right_one(env):
    cams = M.simple_cameras(100)
    pts = [X + [k * 1e-8, 0, 0] for k in range(80)] + [X + [1e-5, 0, 0]]                   # 80 points that all see camera 0 ...
    views = [(0, k) for k in range(80)] + [(k + 1, k) for k in range(80)] + [(90, 80), (91, 80)]      # ... and one that does not
    ref, out, into = _hand(env, cams, pts, views, RADIUS, MAX_ERROR, tag="cluster of 80")
    cams_, pts_ = cams, np.asarray(pts)
    row_ptr, pt_idx, uv = M.observe(cams_, pts_, views)
    first = M.one_round(cams_, pts_, row_ptr, pt_idx, uv, RADIUS, MAX_ERROR)
    assert (first["partner"][:80] == 80).all() and first["partner"][80] == 79               # 79 refusals before the one that fits
    assert into.tolist() == list(range(79)) + [79, 79] and ref["rejected"] == 80 * 79 // 2


def test_candidates_in_each_of_the_nine_cells_and_points_on_the_extent(env):
    r = 0.01
    centre = np.array([1.5 * r, 0.0, 1.5 * r])
    ring = [(dx, dz) for dx in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dz) != (0, 0)]
    # points 0, 1 and 2, 3: twins exactly on the extent's minimum and maximum; 4: the centre of cell (1, 1); 5 .. 12: one per other cell
    pts = [[0, 0, 0], [0, 0, 0], [3 * r, 0, 3 * r], [3 * r, 0, 3 * r], centre] + [centre + [0.6 * r * dx, 0, 0.6 * r * dz] for dx, dz in ring]
    cams = M.simple_cameras(40)
    for free in range(8):                                        # every neighbour but one shares camera 20 with the centre
        views = [(0, 0), (1, 1), (2, 2), (3, 3), (20, 4), (21, 4)]
        for k in range(8):
            views += [(22 + k, 5 + k)] + ([] if k == free else [(20, 5 + k)])
        ref, out, into = _hand(env, cams, pts, views, r, 1e-2, tag="nine cells, free %d" % free)
        assert into[:4].tolist() == [0, 0, 2, 2]
        row_ptr, pt_idx, uv = M.observe(cams, np.asarray(pts, dtype=np.float64), views)
        first = M.one_round(cams, np.asarray(pts, dtype=np.float64), row_ptr, pt_idx, uv, r, 1e-2)
        assert first["partner"][4] == 5 + free                   # the one candidate left, whichever cell it lies in


def test_one_cell_tiny_problems_radius_zero_and_distance_equal_to_the_radius(env):
    cams = M.simple_cameras(8)
    four = [(0, 0), (1, 0), (2, 1), (3, 1)]
    _, out, into = _hand(env, cams, [X, X, -X, -X], four + [(4, 2), (5, 3)], 10.0, MAX_ERROR, tag="one cell")
    assert into.tolist() == [0, 0, 2, 2]
    _, out, _ = _hand(env, cams, [X], [(0, 0), (1, 0)], RADIUS, MAX_ERROR, tag="one point")
    assert out == dict(merged=0, rounds=1)
    _, out, into = _hand(env, cams, [X, X], four, RADIUS, MAX_ERROR, tag="two points")
    assert into.tolist() == [0, 0]
    _, out, into = _hand(env, cams, [X, X, X + [1e-9, 0, 0]], four + [(4, 2)], 0.0, MAX_ERROR, tag="radius 0")
    assert into.tolist() == [0, 0, 2]
    h = 2.0 ** -8
    pts = [[0, 0, 0], [h, 0, 0]]
    _, _, into = _hand(env, cams, pts, four, h, 1e-2, tag="distance == radius")
    assert into.tolist() == [0, 0]
    _, _, into = _hand(env, cams, pts, four, float(np.nextafter(h, 0.0)), 1e-2, tag="distance just above the radius")
    assert into.tolist() == [0, 1]
    bad = X.copy()
    bad[1] = np.nan
    _, _, into = _hand(env, cams, [X, bad, X], four + [(4, 2), (5, 2)], RADIUS, MAX_ERROR, seen_at=[X, X, X], tag="a NaN coordinate")
    assert into.tolist() == [0, 1, 0]
    _, _, into = _hand(env, M.simple_cameras(8, behind=(3,)), [X, X], four, RADIUS, MAX_ERROR, tag="behind a camera")
    assert into.tolist() == [0, 1]


# ---- 4. the state around the call ----------------------------------------------------------------------------------------
def test_held_and_prior_carrying_points_keep_their_bits_and_their_observations(env):
    S = _split(0.0)
    P = S["P"]
    ba = _load(P)
    both = sorted(S["both"])
    const, tied = both[0:6], both[6:12]                          # originals with both halves seen: they would merge
    pm = np.zeros(len(P["pts"]), dtype=bool)
    pm[const] = True
    w = np.zeros((len(P["pts"]), 3))
    w[tied, 1] = 2.0
    w[S["twin_of"][both[12]], 2] = 0.5                           # a copy tied instead of its original
    ba.set_constant(points=pm)
    ba.set_priors(point_weights=w)
    held = pm | (w != 0.0).any(axis=1)
    p0, i0 = ba.points(), ba.pt_idx.copy()
    # the Level-1 call takes `held` from the handle; Level 0 and the reference are given the same bytes
    ref, out, into = _both_levels_equal_the_reference(env, ba, True, RADIUS, MAX_ERROR, 2, held=held.astype(np.uint8), tag="held")
    assert out["merged"] == len(both) - 13
    hp = np.flatnonzero(held)
    assert _bits(ba.points()[hp], p0[hp]) and (into[hp] == hp).all()
    for a in const + tied + [both[12]]:
        b = S["twin_of"][a]
        assert into[a] == a and into[b] == b
        assert np.array_equal(ba.pt_idx == a, i0 == a) and np.array_equal(ba.pt_idx == b, i0 == b)
    got_c, got_p = ba.constant()
    assert np.array_equal(got_p, pm) and not got_c.any() and _bits(ba.priors["point_weights"], w)
    ba.close()


def test_masks_priors_loss_preconditioner_and_checkpoint_survive_and_nothing_stale_stays(env):
    import city2ba_amd as c2b
    import _solvecheck as SC
    from city2ba_amd.solve import levenberg_marquardt_device
    S = _split(0.0)
    P = S["P"]
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
    b0, p0 = ba.cameras_bal(), ba.points()
    pri0 = ba.priors
    out = ba.merge_points(RADIUS, MAX_ERROR, rounds=2)
    assert out["merged"] > 80 and out["rounds"] == 2
    got_c, got_p = ba.constant()
    assert np.array_equal(got_c, SC.unpack(cm)) and np.array_equal(got_p, pm)
    assert ba.loss == ("cauchy", 0.25) and ba.preconditioner == "schur_jacobi"
    pri1 = ba.priors
    assert all(_bits(pri1[k], pri0[k]) for k in pri0 if k != "active") and pri1["active"] == pri0["active"]
    assert _bits(ba.cameras_bal(), b0)
    twin = c2b.BAProblem.from_bal(b0, ba.points(), ba.row_ptr, ba.pt_idx, ba.observations().reshape(-1, 2), device=0)
    twin.set_constant(cm, pm)
    twin.set_priors(camera_centers=pri0["camera_centers"], camera_center_weights=cw)
    twin.set_loss("cauchy", 0.25)
    twin.set_preconditioner("schur_jacobi")
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)      # the list's caches were rebuilt, not reused
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    assert ba.total_reprojection_error(2.0) == twin.total_reprojection_error(2.0)
    twin.close()
    # a call that merges nothing: one round, no bit of the list or the points moves, and the next step is the last one
    i1, p1 = ba.pt_idx.copy(), ba.points()
    assert ba.merge_points(RADIUS, MAX_ERROR, rounds=3) == dict(merged=0, rounds=1)
    assert _bits(ba.pt_idx, i1) and _bits(ba.points(), p1)
    dc3, dp3, info3 = ba.solve_step(1e-2)
    assert _bits(_np(dc3), _np(dc)) and _bits(_np(dp3), _np(dp)) and info3 == info
    ba.rollback()                                                # the checkpoint taken before the merge: the entities of then
    assert _bits(ba.points(), p0) and _bits(ba.cameras_bal(), b0) and _bits(ba.pt_idx, i1)
    # the LM loop runs on the merged problem (it takes the checkpoint for itself); the absorbed points take a zero step
    absorbed = np.setdiff1d(np.arange(len(p0)), np.unique(ba.pt_idx.astype(np.int64)))
    assert len(absorbed) >= out["merged"]
    history, summary = levenberg_marquardt_device(ba, iterations=2)
    assert summary["iterations"] >= 1 and np.isfinite(summary["final_cost"]) and summary["final_cost"] <= summary["initial_cost"]
    assert _bits(ba.points()[absorbed], p0[absorbed])
    ba.close()


def test_two_calls_on_equal_inputs_give_equal_bits(env):
    S = _split(1e-4)
    res = []
    for _ in range(2):
        ba = _load(S["P"])
        out, into = ba.merge_points(RADIUS, 1e-2, rounds=3, return_map=True)
        res.append((out, into, ba.points(), ba.pt_idx.copy()))
        ba.close()
    assert res[0][0] == res[1][0] and all(_bits(a, b) for a, b in zip(res[0][1:], res[1][1:]))


def test_refusals_leave_the_problem_unchanged_and_no_observations_merge_nothing(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    S = _split(0.0)
    P = S["P"]
    ba = _load(P)
    before = ba.points()
    merged, run = C.c_int64(-7), C.c_int(-7)
    call = lambda radius, err, rounds: L.lib().c2b_problem_merge_points(ba._h, radius, err, rounds, None, C.byref(merged), C.byref(run))
    inf, nan = float("inf"), float("nan")
    for args, word in (((-1.0, 1e-4, 1), b"radius"), ((nan, 1e-4, 1), b"radius"), ((inf, 1e-4, 1), b"radius"), ((0.5, -1e-300, 1), b"max_error"),
                       ((0.5, nan, 1), b"max_error"), ((0.5, inf, 1), b"max_error"), ((0.5, 1e-4, 0), b"rounds"), ((0.5, 1e-4, -2), b"rounds")):
        assert call(*args) == L.ERR_INVALID_ARGUMENT, args
        assert word in L.lib().c2b_last_error() and merged.value == -7 and run.value == -7, (args, L.lib().c2b_last_error())
        assert _bits(ba.points(), before) and _bits(ba.pt_idx, P["pt_idx"])
    with pytest.raises(c2b.City2baError) as ei:
        ba.merge_points(0.5, 1e-4, rounds=0)
    assert ei.value.status == L.ERR_INVALID_ARGUMENT
    L.check(L.lib().c2b_problem_set_shard(ba._h, 0, ba.num_cameras() + 5, 0))       # a shard is refused
    assert call(0.5, 1e-4, 1) == L.ERR_INVALID_ARGUMENT and b"shard" in L.lib().c2b_last_error() and merged.value == -7
    assert _bits(ba.points(), before)
    ba.close()
    n_cam = len(P["bal9"])
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)), device=0)
    out, into = ba.merge_points(RADIUS, MAX_ERROR, rounds=2, return_map=True)
    assert out == dict(merged=0, rounds=0) and np.array_equal(into, np.arange(len(P["pts"]))) and _bits(ba.points(), P["pts"])
    ba.close()
