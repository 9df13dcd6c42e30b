"""Inner iterations of the LM loops (BAProblem.set_inner_iterations, levenberg_marquardt(inner_iterations=n)) on
tests/_problems.py's dome_problem: 0 is bit for bit a handle that never set it; with 2 the device loop is the Python loop
iteration for iteration and bit for bit (tests/test_gpu_lm_device.py's property); a refinement never raises the cost beyond the
cost's summation bound; a rejected iteration leaves the points of the last accepted state; constant points do not move."""
import numpy as np
import pytest

import _solvecheck as SC
from _problems import dome_problem
from test_gpu_schur_step import _bits, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
_cache = {}


def _dome(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _cache:
        _cache[key] = dome_problem(**kw)
    return _cache[key]


def _load(P):
    import city2ba_amd as c2b
    return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


def _cases():
    """name -> keyword arguments of both loops; the Cauchy scale is twice the median residual norm"""
    P = _dome()
    if "cauchy_scale" not in _cache:
        ba = _load(P)
        _cache["cauchy_scale"] = SC.cauchy_scale(ba.residual_jacobian()[0])
        ba.close()
    return {"plain": dict(lam=1e-4), "cauchy": dict(lam=1e-4, loss="cauchy", loss_scale=_cache["cauchy_scale"]),
            "centre_prior": dict(lam=1e-4, priors=dict(camera_center_weights=2.0)),
            "masked": dict(lam=1e-4, constant=SC.dome_mask(P))}


def _same(ha, hb):
    assert len(ha) == len(hb)
    for k, (a, b) in enumerate(zip(ha, hb)):
        for key in ("accepted", "pcg_iterations", "status", "error", "cost", "lam"):
            assert a[key] == b[key], (k, key, a[key], b[key])
    assert ha[-1]["error_after"] == hb[-1]["error_after"]


def test_zero_inner_iterations_is_a_handle_that_never_set_it(env):
    from city2ba_amd import solve
    from city2ba_amd import _lib as L
    import ctypes as C
    P = _dome()
    runs = []
    for prepare in (None, lambda ba: ba.set_inner_iterations(0), lambda ba: (ba.set_inner_iterations(2), ba.set_inner_iterations(0))):
        ba = _load(P)
        assert ba.inner_iterations() == 0
        if prepare is None:                                  # the library's entry itself: the Python wrapper would set the state
            opt = L.LmOptions(6, 100, 1e-4, 1e-6, 0.0, 0.0, 0.0)
            entries, s = (L.LmIteration * 6)(), L.LmSummary()
            L.check(L.lib().c2b_problem_levenberg_marquardt(ba._h, C.byref(opt), entries, 6, C.byref(s)))
            h = [(e.cost, e.cost_trial, e.lam, e.accepted, e.pcg_iterations, e.model_decrease, e.gradient_max, e.step_norm) for e in entries]
        else:
            prepare(ba)
            hist, s2 = solve.levenberg_marquardt_device(ba, 6, lam=1e-4)
            h = [(e["cost"], e["cost_trial"], e["lam"], int(e["accepted"]), e["pcg_iterations"], e["model_decrease"], e["gradient_max"], e["step_norm"]) for e in hist]
        assert ba.inner_iterations() == 0
        runs.append((h, ba.cameras_bal(), ba.points()))
        ba.close()
    for other in runs[1:]:
        assert other[0] == runs[0][0] and _bits(other[1], runs[0][1]) and _bits(other[2], runs[0][2])


def test_the_loops_leave_the_handles_setting_alone_unless_told(env):
    from city2ba_amd import solve
    P = _dome()
    ends = []
    for how in ("argument", "handle"):
        ba = _load(P)
        if how == "handle":
            ba.set_inner_iterations(2)
        h, s = solve.levenberg_marquardt_device(ba, 3, lam=1e-4, **(dict(inner_iterations=2) if how == "argument" else {}))
        assert ba.inner_iterations() == 2
        ends.append((ba.cameras_bal(), ba.points(), s["final_cost"]))
        ba.close()
    assert _bits(ends[0][0], ends[1][0]) and _bits(ends[0][1], ends[1][1]) and ends[0][2] == ends[1][2]
    ba = _load(P)
    ba.set_inner_iterations(2)
    hp = solve.levenberg_marquardt(ba, 3, lam=1e-4)          # the Python loop reads the handle's setting too
    assert ba.inner_iterations() == 2 and _bits(ba.points(), ends[0][1]) and hp[-1]["error_after"] == ends[0][2]
    solve.levenberg_marquardt_device(ba, 1, inner_iterations=0)
    assert ba.inner_iterations() == 0
    ba.close()


@pytest.mark.parametrize("name", ["plain", "cauchy", "centre_prior", "masked"])
def test_device_loop_with_inner_iterations_is_the_python_loop(env, name):
    from city2ba_amd import solve
    P, kw = _dome(), _cases()[name]
    ba = _load(P)
    hp = solve.levenberg_marquardt(ba, 6, inner_iterations=2, **kw)
    bp, pp = ba.cameras_bal(), ba.points()
    ba.close()
    ba = _load(P)
    hd, s = solve.levenberg_marquardt_device(ba, 6, inner_iterations=2, **kw)
    bd, pd = ba.cameras_bal(), ba.points()
    assert ba.inner_iterations() == 2
    ba.close()
    plain = _load(P)
    h0, s0 = solve.levenberg_marquardt_device(plain, 6, **kw)
    p0 = plain.points()
    plain.close()
    print("LMINNER %s: accepted %s cost %.9g -> %.9g (without inner iterations: %s -> %.9g)"
          % (name, "".join("A" if e["accepted"] else "R" for e in hd), hd[0]["error"], s["final_cost"], "".join("A" if e["accepted"] else "R" for e in h0), s0["final_cost"]))
    _same(hp, hd)
    assert _bits(bp, bd) and _bits(pp, pd) and s["iterations"] == 6
    assert not _bits(pd, p0)                                 # the option did something
    assert s["final_cost"] < s["initial_cost"]
    if name == "masked":
        cm, pm = kw["constant"]
        assert _bits(bd[SC.unpack(cm)], P["bal9"][SC.unpack(cm)]) and _bits(pd[pm], P["pts"][pm])          # constant points do not move


@pytest.mark.parametrize("name", ["plain", "cauchy"])
def test_a_refinement_never_raises_the_cost(env, name):
    """the Python loop's steps by hand: the cost before and after every refinement.  Bound: each of the two evaluations
    rounds within cost x 2^-52 x (depth + 16), depth = 18 + ceil(n_blocks / 256) (tests/test_gpu_robust_loss.py's
    test_robust_cost)."""
    P, kw = _dome(), _cases()[name]
    ba = _load(P)
    if "loss" in kw:
        ba.set_loss(kw["loss"], kw["loss_scale"])
    cost = (lambda: ba.robust_cost()) if "loss" in kw else (lambda: ba.total_reprojection_error(2.0) ** 2)
    depth = 18 + -(-(-(-ba.num_observations() // 256)) // 256)
    lam, best = 1e-4, np.inf
    for k in range(5):
        dc, dp, info = ba.solve_step(lam)
        ba.apply_step(dc, dp)
        before = cost()
        counts = ba.refine_points(rounds=2)
        after = cost()
        bound = (before + after) * EPS * (depth + 16)
        best = min(best, (after - before) / bound)
        print("LMINNER %s step %d: cost %.17g -> %.17g after refine_points (%d moved)" % (name, k, before, after, counts["moved"]))
        assert after <= before + bound, (name, k, before, after, bound)
        lam = max(lam / 3.0, 1e-20)
    assert best < -1.0                                       # and at least once it lowered it, by more than rounding
    ba.close()


def test_a_rejected_iteration_leaves_the_points_of_the_last_accepted_state(env):
    """at convergence a step no longer lowers the cost and is rejected: the run that ends with that rejected iteration holds,
    bit for bit, the cameras and the points of the run that ends one iteration earlier -- the refined trial points went back
    through the checkpoint"""
    from city2ba_amd import solve
    P = _dome()
    ba = _load(P)
    h, s = solve.levenberg_marquardt_device(ba, 14, lam=1e-4, inner_iterations=2)
    ba.close()
    rejected = [k for k, e in enumerate(h) if not e["accepted"]]
    print("LMINNER rollback: accepted %s" % "".join("A" if e["accepted"] else "R" for e in h))
    assert rejected and rejected[0] > 0, [e["accepted"] for e in h]
    k = rejected[0]
    ends = []
    for n in (k, k + 1):
        ba = _load(P)
        hn, sn = solve.levenberg_marquardt_device(ba, n, lam=1e-4, inner_iterations=2)
        ends.append((ba.cameras_bal(), ba.points(), sn["final_cost"]))
        assert [e["accepted"] for e in hn] == [e["accepted"] for e in h[:n]]
        ba.close()
    assert _bits(ends[0][0], ends[1][0]) and _bits(ends[0][1], ends[1][1]) and ends[0][2] == ends[1][2]
    assert h[k]["cost_trial"] >= h[k]["cost"] or h[k]["model_decrease"] <= 0.0
