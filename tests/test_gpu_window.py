"""BAProblem.window, origin, write_back and solve.solve_window / solve_windows on the device against
tests/_subsetref.py: the windows of the locality grid and of the dome whose sizes tests/test_subsetref.py establishes on the
CPU, in both modes.  Structure and residuals bit for bit; the normal-equation blocks of the free entities within
_normref.bound at the block's own observation count (what catches a dropped observation); the cost reduction of a window
solve against the parent's within the summation bound of the four sums."""
import numpy as np
import pytest

import _normref as NR
import _subsetref as SR
from _problems import dome_problem

pytestmark = pytest.mark.gpu
HALO = [True, False]
U53 = 2.0 ** -53
_cache = {}


@pytest.fixture(scope="module")
def c2b():
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd
    assert city2ba_amd.device_count() > 0
    return city2ba_amd


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _problem(name):
    """dict(cams15, bal9, pts, row_ptr, pt_idx, uv, bal) of "grid" (bal mode), "grid moved" (the start moved, bal), "grid moved
    state", "dome bal", "dome state"; computed once"""
    import oracle as O
    if name not in _cache:
        if name.startswith("dome"):
            _cache[name] = dome_problem(dup=True, state=name.endswith("state"))
        else:
            cams, pts, row_ptr, pt_idx, uv = SR.locality_grid()
            bal9 = O.camera_to_bal(cams)
            if "moved" in name:                               # pose and point noise, as the coupled tests move their start
                rng = np.random.default_rng(9)
                bal9[:, :6] += rng.normal(scale=2e-3, size=(len(bal9), 6))
                pts = pts + rng.normal(scale=2e-3, size=pts.shape)
            _cache[name] = dict(cams15=O.camera_from_bal(bal9), bal9=bal9, pts=pts, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv,
                                bal=not name.endswith("state"))
    return _cache[name]


def _load(c2b, P):
    if P["bal"]:
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    return c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


CASES = [("grid", k) for k in SR.GRID_WINDOWS] + [("dome bal", k) for k in SR.DOME_WINDOWS] + [("dome state", k) for k in SR.DOME_WINDOWS]


def _seeds(problem, window, n_cam):
    table = SR.GRID_WINDOWS if problem.startswith("grid") else SR.DOME_WINDOWS
    return table[window][0](n_cam), table[window][1]


def _cost(ba):
    return ba.total_reprojection_error(2.0) ** 2


def _pts4_lane(c2b, ba):
    return ba.export_device()["pts4"].cpu().numpy()[:, 3].copy()


# ---- (a) structure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_state", [False, True], ids=["plain", "state"])
@pytest.mark.parametrize("halo", HALO, ids=["halo", "nohalo"])
@pytest.mark.parametrize("problem,window", CASES)
def test_structure_is_the_references(c2b, problem, window, halo, with_state):
    P = _problem(problem)
    ba = _load(c2b, P)
    n_cam, n_pts = ba.num_cameras(), ba.num_points()
    seeds, sizes = _seeds(problem, window, n_cam)
    wh = SR.window(P["row_ptr"], P["pt_idx"], n_pts, seeds, halo=True)
    wn = SR.window(P["row_ptr"], P["pt_idx"], n_pts, seeds, halo=False)
    SR.assert_sizes(SR.window_sizes(wh, wn), sizes)           # the sizes first
    w = wh if halo else wn
    cm = pm = None
    if with_state:                                            # a focal-constant seed camera, a constant point, a point prior
        cm = np.zeros(n_cam, np.uint16)
        cm[seeds[0]] = 1 << 6
        pm = np.zeros(n_pts, np.uint8)
        pm[P["pt_idx"][int(P["row_ptr"][seeds[0]])] if len(w["P"]) else 0] = 1
        ba.set_constant(cameras=cm, points=pm)
        xw = np.zeros((n_pts, 3))
        xw[::3] = 0.5
        ba.set_priors(points=P["pts"] + 0.01, point_weights=xw)
        ba.set_loss("cauchy", 0.5)
    child = ba.window(seeds if window != "every 7th" else SR.as_seed(seeds, n_cam), halo=halo)       # a list, or a bool mask
    assert child._sizes() == (len(w["cam_of"]), len(w["pt_of"]), len(w["pt_idx"]))
    o = child.origin()
    for k in ("cam_of", "pt_of", "cam_role", "pt_role"):
        assert _bits(o[k], w[k]), k
    cams, pts, uv = ba.cameras(), ba.points(), ba.observations()
    assert _bits(child.cameras(), cams[w["cam_of"]]) and _bits(child.points(), pts[w["pt_of"]])
    assert _bits(child.cameras_bal(), ba.cameras_bal()[w["cam_of"]])
    assert _bits(child.row_ptr, w["row_ptr"]) and _bits(child.pt_idx, w["pt_idx"]) and _bits(child.observations(), uv[w["obs_of"]])
    want_c, want_p = SR.window_masks(w, cm, pm)
    got_c, got_p = child.constant()
    assert _bits(got_c, ((want_c[:, None] >> np.arange(9, dtype=np.uint16)) & 1).astype(bool)) and _bits(got_p, want_p.astype(bool))
    pc, pp = child.priors, ba.priors
    for k in ("camera_centers", "camera_center_weights", "intrinsics", "intrinsics_weights"):
        assert _bits(pc[k], pp[k][w["cam_of"]]), k
    for k in ("points", "point_weights"):
        assert _bits(pc[k], pp[k][w["pt_of"]]), k
    assert child.loss == ba.loss and child.preconditioner == ba.preconditioner
    if window == "all":                                       # the child is the parent
        assert _bits(child.row_ptr, ba.row_ptr) and _bits(child.pt_idx, ba.pt_idx) and not o["cam_role"].any() and not o["pt_role"].any()
    child.close()
    ba.close()


# ---- (b) residual bits, (c) normal equations ----------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALO, ids=["halo", "nohalo"])
@pytest.mark.parametrize("problem,window", [c for c in CASES if c[1] != "77 alone"])
def test_residuals_are_the_parents_bits_and_the_free_blocks_are_the_parents(c2b, problem, window, halo):
    P = _problem(problem)
    ba = _load(c2b, P)
    n_cam, n_pts = ba.num_cameras(), ba.num_points()
    seeds, _ = _seeds(problem, window, n_cam)
    w = SR.window(P["row_ptr"], P["pt_idx"], n_pts, seeds, halo=halo)
    child = ba.window(seeds, halo=halo)
    r, Jc, Jp = ba.residual_jacobian()
    rc, _, _ = child.residual_jacobian()
    assert _bits(rc, r[w["obs_of"]])
    cam_of_obs = np.repeat(np.arange(n_cam), np.diff(P["row_ptr"].astype(np.int64)))
    ref = NR.blocks(r, Jc, Jp, cam_of_obs, P["pt_idx"].astype(np.int64), n_cam, n_pts)
    U, gc, V, gp, _ = child.normal_equations()
    U, gc, V, gp = (a.cpu().numpy() for a in (U, gc, V, gp))
    seed_rows = np.flatnonzero(w["cam_role"] == 0)
    free_pts = np.arange(len(w["pt_of"])) if halo else np.flatnonzero(w["pt_role"] == 0)
    pc, pq = w["cam_of"][seed_rows].astype(np.int64), w["pt_of"][free_pts].astype(np.int64)
    worst = {}
    for name, dev, rows, par, k in (("U", U, seed_rows, pc, "kc"), ("gc", gc, seed_rows, pc, "kc"), ("V", V, free_pts, pq, "kp"),
                                    ("gp", gp, free_pts, pq, "kp")):
        worst[name] = NR.excess(dev[rows], ref[name][par], ref["S" + name][par], ref[k][par])
    print("WINDOW blocks %s %s %s: |err| / bound %s" % (problem, window, "halo" if halo else "no-halo", {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    child.close()
    ba.close()


# ---- (d) solve and write back -------------------------------------------------------------------------------------------
LM = dict(iterations=4, lam=1e-4, max_iters=50, rel_tol=1e-8)


@pytest.mark.parametrize("halo", HALO, ids=["halo", "nohalo"])
@pytest.mark.parametrize("mode", ["bal", "state"])
def test_a_window_solve_written_back_moves_the_free_entities_alone_and_by_the_childs_cost(c2b, mode, halo):
    P = _problem("grid moved" if mode == "bal" else "grid moved state")
    ba, twin = _load(c2b, P), _load(c2b, P)
    twin.apply_step(None, None)                               # what a state-mode parent's untouched cameras become
    n_cam, n_pts, n_obs = ba._sizes()
    seeds = np.arange(37, 101)
    w = SR.window(P["row_ptr"], P["pt_idx"], n_pts, seeds, halo=halo)
    lane0 = _pts4_lane(c2b, ba)
    # The four costs are sums over the same terms only when all four are taken in bal mode: a state-mode handle's cameras are
    # its records, and from_vec(to_vec(.)) of them -- what apply_step, the LM loop and write_back leave -- differs in the last
    # bits, which moves every residual of those cameras, not just the order of a sum.  So on the state-mode parent the cost
    # before is the twin's, and the child (extracted from the state-mode parent as it is) takes the same apply_step of no
    # step before its cost is read -- the first thing the LM loop's checkpoint does anyway.
    Fp0 = _cost(ba if mode == "bal" else twin)
    child = ba.window(seeds, halo=halo)
    if mode == "state":
        assert _bits(child.cameras(), ba.cameras()[w["cam_of"]])
        child.apply_step(None, None)
    Fc0 = _cost(child)
    from city2ba_amd import solve as S
    history, summary = S.levenberg_marquardt_device(child, **LM)
    Fc1 = _cost(child)
    assert Fc1 < Fc0 and summary["final_cost"] < summary["initial_cost"]
    got = child.write_back(ba)
    Fp1 = _cost(ba)
    free_c = w["cam_of"][w["cam_role"] == 0].astype(np.int64)
    free_p = w["pt_of"][w["pt_role"] == 0].astype(np.int64)
    assert got == dict(cameras=len(free_c), points=len(free_p)) and len(free_c) == 64
    assert len(free_p) == (260 if halo else 260 - 179)
    bal, pts, tb, tp = ba.cameras_bal(), ba.points(), twin.cameras_bal(), twin.points()
    out_c, out_p = np.setdiff1d(np.arange(n_cam), free_c), np.setdiff1d(np.arange(n_pts), free_p)
    assert _bits(bal[out_c], tb[out_c]) and _bits(pts[out_p], tp[out_p]) and _bits(_pts4_lane(c2b, ba), lane0)
    seed_rows, pt_rows = np.flatnonzero(w["cam_role"] == 0), np.flatnonzero(w["pt_role"] == 0)
    assert _bits(bal[free_c], child.cameras_bal()[seed_rows]) and _bits(pts[free_p], child.points()[pt_rows])
    assert not _bits(bal[free_c], tb[free_c]) and not _bits(pts[free_p], tp[free_p])
    fresh = c2b.BAProblem.from_bal(bal, pts, P["row_ptr"], P["pt_idx"], P["uv"])
    assert _bits(ba.cameras(), fresh.cameras())              # bal mode, as after apply_step: the cameras are from_vec of bal9
    # the child's cost reduction is the parent's, to the rounding of the four sums (2 terms per observation, all >= 0)
    n_child = child.num_observations()
    bound = U53 * ((2 * n_obs + 4) * (Fp0 + Fp1) + (2 * n_child + 4) * (Fc0 + Fc1))
    diff = abs((Fp0 - Fp1) - (Fc0 - Fc1))
    print("WINDOW solve %s %s: parent %.17g -> %.17g, child %.17g -> %.17g, |difference of the reductions| %.3g, bound %.3g"
          % (mode, "halo" if halo else "no-halo", Fp0, Fp1, Fc0, Fc1, diff, bound))
    assert Fp1 < Fp0 and diff <= bound
    for x in (child, ba, twin, fresh):
        x.close()


@pytest.mark.parametrize("halo", HALO, ids=["halo", "nohalo"])
def test_a_state_mode_child_written_back_unsolved_is_an_apply_step_of_no_step(c2b, halo):
    """parent and child both in state mode: write_back gives both to_vec of their cameras, writes the child's free entries --
    to_vec of the same records, so the same bits -- and leaves both in bal mode, exactly as apply_step(None, None) leaves them"""
    P = _problem("dome state")
    ba, twin = _load(c2b, P), _load(c2b, P)
    twin.apply_step(None, None)
    child = ba.window(np.arange(10), halo=halo)
    assert child.write_back(ba) == dict(cameras=10, points=157 if halo else 157 - 149)
    assert _bits(ba.cameras_bal(), twin.cameras_bal()) and _bits(ba.cameras(), twin.cameras()) and _bits(ba.points(), twin.points())
    o = child.origin()
    assert _bits(child.cameras_bal(), twin.cameras_bal()[o["cam_of"]]) and _bits(child.cameras(), twin.cameras()[o["cam_of"]])
    for x in (child, ba, twin):
        x.close()


# ---- (e) write-back refusals --------------------------------------------------------------------------------------------
def test_write_back_refusals_and_a_mask_cleared_later(c2b):
    import torch
    from city2ba_amd import _lib as L
    P = _problem("grid moved")
    ba = _load(c2b, P)
    seeds = np.arange(0, 20)
    child = ba.window(seeds, halo=True)
    before = (ba.cameras_bal(), ba.points())
    with pytest.raises(L.City2baError):
        child.write_back(child)                               # onto itself
    plain = ba.subset(np.arange(5), np.arange(30))            # no origin
    assert plain.origin() is None
    with pytest.raises(L.City2baError):
        plain.write_back(ba)
    stranger = _load(c2b, P)                                  # the same counts, another handle
    with pytest.raises(L.City2baError):
        child.write_back(stranger)
    assert _bits(stranger.cameras_bal(), before[0]) and _bits(ba.cameras_bal(), before[0]) and _bits(ba.points(), before[1])
    # a mask cleared after the extraction: the halo cameras are free now and are written
    o = child.origin()
    assert o["cam_role"].sum() == 23
    child.set_constant(None, None)
    dc = torch.full((child.num_cameras(), 9), 1e-3, dtype=torch.float64, device="cuda:0")
    child.apply_step(dc, None)
    got = child.write_back(ba)
    assert got == dict(cameras=43, points=78)
    bal = ba.cameras_bal()
    assert _bits(bal[o["cam_of"]], child.cameras_bal()) and not _bits(bal[o["cam_of"]], before[0][o["cam_of"]])
    rest = np.setdiff1d(np.arange(len(bal)), o["cam_of"])
    assert _bits(bal[rest], before[0][rest])
    # the parent culled: its entities are renumbered, the origin no longer fits (the epoch)
    culled = _load(c2b, P)
    kid = culled.window(seeds, halo=True)
    culled.cull()
    with pytest.raises(L.City2baError):
        kid.write_back(culled)
    same = _load(c2b, P)                                      # an upload of the same counts replaces the entities too
    kid2 = same.window(seeds, halo=True)
    same._upload(P["bal9"], True, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    with pytest.raises(L.City2baError):
        kid2.write_back(same)
    for x in (child, plain, stranger, ba, culled, kid, same, kid2):
        x.close()


# ---- (f) solve_windows, (g) determinism ---------------------------------------------------------------------------------
def test_solve_windows_never_raises_the_cost_and_is_deterministic(c2b):
    from city2ba_amd import solve as S
    P = _problem("grid moved")
    ba, twin = _load(c2b, P), _load(c2b, P)
    n_cam, _, n_obs = ba._sizes()
    F0 = F = _cost(ba)
    seen = np.zeros(n_cam, bool)
    mine = []
    for sweep in range(2):                                    # solve_windows' loop, with the parent's cost read between windows
        for lo in range(0, n_cam, 32):
            hi = min(lo + 64, n_cam)
            s = S.solve_window(ba, range(lo, hi), halo=True, **LM)
            Fn = _cost(ba)
            bound = U53 * ((2 * n_obs + 4) * (F + Fn) + (2 * s["observations"] + 4) * (s["initial_cost"] + s["final_cost"]))
            assert s["final_cost"] <= s["initial_cost"] and Fn <= F + bound, (sweep, lo, F, Fn, bound)
            F = Fn
            seen[lo:hi] = True
            mine.append(s)
            if hi == n_cam:
                break
    assert F < F0 and seen.all()
    theirs = S.solve_windows(twin, 64, stride=32, sweeps=2, halo=True, **LM)
    assert [(s["sweep"], s["lo"], s["hi"]) for s in theirs] == [(k // 12, 32 * (k % 12), min(32 * (k % 12) + 64, 400)) for k in range(24)]
    assert len(mine) == len(theirs) and all(a["final_cost"] == b["final_cost"] and a["cameras"] == b["cameras"] for a, b in zip(mine, theirs))
    assert _bits(ba.cameras_bal(), twin.cameras_bal()) and _bits(ba.points(), twin.points())       # two runs, the same bits
    print("WINDOW sweeps: cost %.17g -> %.17g over %d windows" % (F0, F, len(mine)))
    # two extractions give the same bits
    a, b = ba.window(np.arange(37, 101), halo=False), ba.window(np.arange(37, 101), halo=False)
    for f in ("cameras", "points", "observations", "cameras_bal"):
        assert _bits(getattr(a, f)(), getattr(b, f)()), f
    assert _bits(a.pt_idx, b.pt_idx) and _bits(a.row_ptr, b.row_ptr)
    for x in (a, b, ba, twin):
        x.close()
