"""Levenberg-Marquardt inside the library (c2b_problem_levenberg_marquardt) on tests/_problems.py's dome_problem
and smaller: the device-side checkpoint and rollback are exact, the device loop is city2ba_amd.solve.levenberg_marquardt
iteration for iteration and bit for bit, the quantities its stopping tests read are what the handle's own gradient, step
and state give, every stopping test fires at the iteration its tolerance was placed at and at no other, and bad arguments
and the empty problem end as specified."""
import ctypes as C

import numpy as np
import pytest

import _solvecheck as SC
from _problems import dome_problem, random_problem
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
# The start whose history holds rejected and accepted steps, picked with _solvecheck.host_lm on the CPU: from
# dome_problem(start_noise=0.3) at lam = 1e-4 the host loop's ten steps are A R A A A R R R A A (the second step
# overshoots: 13.84 is kept while the trial cost rises), against A A A A A A R R A R at start_noise = 1e-2, where the
# only rejections are rounding at convergence.
REJECTING = dict(start_noise=0.3)
REJECTING_LAM = 1e-4
_cache = {}


def _dome(mode="bal", **kw):
    key = ("dome", mode, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = dome_problem(state=mode == "state", **kw)
    return _cache[key]


def _load(P):
    import city2ba_amd as c2b
    if P.get("bal", True):
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    return c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


def _cases():
    """name -> (problem, keyword arguments of both loops); the Cauchy scale is twice the median residual norm"""
    P = _dome()
    if "cauchy_scale" not in _cache:
        ba = _load(P)
        _cache["cauchy_scale"] = SC.cauchy_scale(ba.residual_jacobian()[0])
        ba.close()
    return {"plain": (P, dict(lam=1e-4)),
            "cauchy": (P, dict(lam=1e-4, loss="cauchy", loss_scale=_cache["cauchy_scale"])),
            "schur_jacobi_masked": (P, dict(lam=1e-4, preconditioner="schur_jacobi", constant=SC.dome_mask(P))),
            "rejecting": (_dome(**REJECTING), dict(lam=REJECTING_LAM))}


def _device_run(name, iterations=10, **tols):
    """(history, summary, cameras_bal, points) of levenberg_marquardt_device on a fresh handle; computed once per argument set"""
    from city2ba_amd import solve
    key = ("run", name, iterations, tuple(sorted(tols.items())))
    if key not in _cache:
        P, kw = _cases()[name]
        ba = _load(P)
        h, s = solve.levenberg_marquardt_device(ba, iterations, **kw, **tols)
        _cache[key] = (h, s, ba.cameras_bal(), ba.points())
        ba.close()
    return _cache[key]


# ---- 1. rollback is exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("mode", ["bal", "state"])
def test_rollback_is_exact(env, mode, masked):
    import city2ba_amd as c2b
    torch, dev = env["torch"], env["dev"]
    P = _dome(mode)
    ba = _load(P)
    with pytest.raises(c2b.City2baError):
        ba.rollback()                                        # no checkpoint yet
    if masked:
        ba.set_constant(*SC.dome_mask(P))
    ba.checkpoint()
    b0, p0, c0 = ba.cameras_bal(), ba.points(), ba.cameras()
    dc0, dp0, info0 = ba.solve_step(1e-4, 25, 0.0)
    dc0, dp0 = _np(dc0), _np(dp0)
    rng = np.random.default_rng(11)
    for _ in range(2):                                       # the checkpoint survives apply_step and a rollback
        ba.apply_step(torch.from_numpy(rng.normal(scale=0.5, size=b0.shape)).to(dev),
                      torch.from_numpy(rng.normal(scale=0.5, size=p0.shape)).to(dev))
        assert not _bits(ba.cameras_bal(), b0) and not _bits(ba.points(), p0)
        ba.rollback()
        assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), p0) and _bits(ba.cameras(), c0)
        dc1, dp1, info1 = ba.solve_step(1e-4, 25, 0.0)
        assert _bits(_np(dc1), dc0) and _bits(_np(dp1), dp0) and info1 == info0, (info0, info1)
    if masked:
        cm, pm = ba.constant()
        assert _bits(cm, SC.unpack(SC.dome_mask(P)[0])) and _bits(pm, SC.dome_mask(P)[1])
    ba.drop_checkpoint()
    with pytest.raises(c2b.City2baError):
        ba.rollback()
    ba.checkpoint()
    ba._upload(b0, True, p0, ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())     # any upload drops it
    with pytest.raises(c2b.City2baError):
        ba.rollback()
    ba.close()


# ---- 2. the device loop is the Python loop ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "cauchy", "schur_jacobi_masked", "rejecting"])
def test_device_loop_is_the_python_loop(env, name):
    from city2ba_amd import solve
    P, kw = _cases()[name]
    ba = _load(P)
    hp = solve.levenberg_marquardt(ba, 10, **kw)
    bp, pp = ba.cameras_bal(), ba.points()
    ba.close()
    hd, s, bd, pd = _device_run(name)
    print("LMDEV %s: accepted %s cost %.6g -> %.6g" % (name, "".join("A" if e["accepted"] else "R" for e in hd), hd[0]["error"], s["final_cost"]))
    assert len(hp) == len(hd) == s["iterations"] == 10 and s["termination"] == 0
    for k, (a, b) in enumerate(zip(hp, hd)):
        for key in ("accepted", "pcg_iterations", "status", "error", "cost", "lam"):
            assert a[key] == b[key], (name, k, key, a[key], b[key])
    assert hp[-1]["error_after"] == hd[-1]["error_after"] == s["final_cost"] and s["initial_cost"] == hp[0]["error"]
    assert _bits(bp, bd) and _bits(pp, pd)
    if name == "rejecting":                                  # both kinds of step: the rollback and the checkpoint both ran
        acc = [e["accepted"] for e in hd]
        assert any(acc) and not all(acc), acc
    if name == "schur_jacobi_masked":
        cm, pm = SC.dome_mask(P)
        assert _bits(bd[SC.unpack(cm)], P["bal9"][SC.unpack(cm)]) and _bits(pd[pm], P["pts"][pm])


# ---- 3. the recorded quantities -------------------------------------------------------------------------------------------
def _check_quantities(P, lam, constant=None):
    from city2ba_amd import solve
    ba, twin = _load(P), _load(P)
    if constant is not None:
        twin.set_constant(*constant)
    h, s = solve.levenberg_marquardt_device(ba, 1, lam=lam, constant=constant)
    assert s["iterations"] == 1 and len(h) == 1
    e = h[0]
    U, gc, V, gp, _ = twin.normal_equations()
    gc, gp = _np(gc), _np(gp)
    want = max(float(np.abs(gc).max()) if gc.size else 0.0, float(np.abs(gp).max()) if gp.size else 0.0)
    assert e["gradient_max"] == want, (e["gradient_max"], want)
    dc, dp, info = twin.solve_step(lam, 100, 1e-6)
    dc, dp = _np(dc).astype(LD), _np(dp).astype(LD)
    x = np.concatenate([twin.cameras_bal().ravel(), twin.points().ravel()]).astype(LD)
    n = x.size                                               # 9 n_cam + 3 n_pts entries: the sums' own bound, 4 n eps relative
    step = float(np.sqrt(np.sum(dc * dc) + np.sum(dp * dp)))
    xn = float(np.sqrt(np.sum(x * x)))
    print("LMDEV quantities n=%d: step_norm rel err %.3g, x_norm rel err %.3g (bound %.3g)"
          % (n, abs(e["step_norm"] - step) / step if step else 0.0, abs(e["x_norm"] - xn) / xn, 4 * n * EPS))
    assert abs(e["step_norm"] - step) <= 4 * n * EPS * step, (e["step_norm"], step)
    assert abs(e["x_norm"] - xn) <= 4 * n * EPS * xn, (e["x_norm"], xn)
    assert e["pcg_iterations"] == info["iterations"] and e["status"] == info["status"] and e["model_decrease"] == info["model_decrease"]
    assert e["pcg_rel_residual"] == info["rel_residual"]
    ba.close()
    twin.close()


def test_recorded_quantities_on_the_dome(env):
    """The pad lane of pts4 cannot show here: every route into a resident problem (the uploads through k_points_pad, the
    layouts and the point sampler) writes 0.0 there and no entry point lets a caller set it, so no load can make it differ;
    k_lm_norms never adds it all the same."""
    _check_quantities(_dome(), 1e-4)
    _check_quantities(_dome(), 1e-4, constant=SC.dome_mask(_dome()))


@pytest.mark.parametrize("n_cam,n_pts", [(1, 63), (63, 64), (64, 65), (65, 1)])
def test_recorded_quantities_around_a_wave(env, n_cam, n_pts):
    """n_cam and n_pts at 1, 63, 64, 65: the tail wave of both kernels on either array"""
    P = random_problem(n_cam, n_pts, 8, seed=100 + n_cam, noise=1e-3)
    _check_quantities(P, 1e-2)
    cm = np.zeros(n_cam, dtype=np.uint16)
    cm[::2] = SC.INTRINSICS                                  # a camera-only mask
    _check_quantities(P, 1e-2, constant=(cm, None))


# ---- 4. each stopping test fires at the right iteration and nowhere else -----------------------------------------------
def _gradient_fires(e, tol):
    return e["gradient_max"] <= tol


def _parameter_fires(e, tol):
    return e["step_norm"] <= tol * (e["x_norm"] + tol)


def _function_fires(e, tol):
    return e["accepted"] and e["cost"] - e["cost_trial"] <= tol * e["cost"]


def _place(h, value, fires, usable=lambda e: True):
    """(K, tol): tol the geometric mean of value(h[k]) and value(h[K]) for consecutive usable entries k < K between which the
    value falls, such that the test fires at K and at no earlier entry; the latest such K >= 2"""
    for K in range(len(h) - 1, 1, -1):
        before = [j for j in range(K) if usable(h[j])]
        if not usable(h[K]) or not before or not value(h[K]) < value(h[before[-1]]):
            continue
        tol = float(np.sqrt(value(h[before[-1]]) * value(h[K])))
        if fires(h[K], tol) and not any(fires(h[j], tol) for j in range(K)):
            return K, tol
    raise AssertionError("no iteration of this history isolates the test")


_SOLVE_KEYS = ("error", "cost", "lam", "model_decrease", "gradient_max", "step_norm", "x_norm", "pcg_rel_residual", "pcg_iterations", "status")


def _same_entries(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        for key in _SOLVE_KEYS + ("accepted", "cost_trial"):
            assert x[key] == y[key], (k, key, x[key], y[key])


@pytest.mark.parametrize("which", ["gradient", "parameter"])
def test_gradient_and_parameter_tolerances_stop_before_the_step(env, which):
    h = _device_run("plain")[0]
    if which == "gradient":
        K, tol = _place(h, lambda e: e["gradient_max"], _gradient_fires)
        hs, s, b, p = _device_run("plain", gradient_tol=tol)
    else:
        K, tol = _place(h, lambda e: e["step_norm"] / e["x_norm"], _parameter_fires)
        hs, s, b, p = _device_run("plain", parameter_tol=tol)
    print("LMDEV %s tolerance %.6g placed at iteration %d" % (which, tol, K))
    assert s["termination"] == (2 if which == "gradient" else 3) and s["iterations"] == K + 1 == len(hs), (s, K)
    _same_entries(hs[:K], h[:K])
    for key in _SOLVE_KEYS:                                  # the entry that stopped the run: solved, not applied
        assert hs[K][key] == h[K][key], (key, hs[K][key], h[K][key])
    assert hs[K]["accepted"] is False and hs[K]["cost_trial"] == hs[K]["cost"] == s["final_cost"]
    _, s0, b0, p0 = _device_run("plain", iterations=K)       # the state iteration K started from
    assert _bits(b, b0) and _bits(p, p0) and s["final_cost"] == s0["final_cost"]


def test_function_tolerance_stops_after_an_accepted_step(env):
    h = _device_run("plain")[0]
    K, tol = _place(h, lambda e: (e["cost"] - e["cost_trial"]) / e["cost"], _function_fires, usable=lambda e: e["accepted"])
    hs, s, b, p = _device_run("plain", function_tol=tol)
    print("LMDEV function tolerance %.6g placed at iteration %d" % (tol, K))
    assert s["termination"] == 1 and s["iterations"] == K + 1 == len(hs), (s, K)
    _same_entries(hs, h[:K + 1])
    assert hs[K]["accepted"] is True and s["final_cost"] == hs[K]["cost_trial"]
    _, s0, b0, p0 = _device_run("plain", iterations=K + 1)   # the step is kept
    assert _bits(b, b0) and _bits(p, p0)


def test_a_rejected_step_does_not_trigger_the_function_test(env):
    """cost - cost_trial <= 0 on a rejected step: below every positive tolerance.  With a tolerance under the smallest
    relative decrease of the accepted steps nothing may fire, so the run is the untoleranced one."""
    h = _device_run("rejecting")[0]
    acc = [e["accepted"] for e in h]
    assert any(acc) and not all(acc), acc
    tol = 0.5 * min((e["cost"] - e["cost_trial"]) / e["cost"] for e in h if e["accepted"])
    assert tol > 0.0 and not any(_function_fires(e, tol) for e in h)
    hs, s, b, p = _device_run("rejecting", function_tol=tol)
    assert s["termination"] == 0 and s["iterations"] == 10
    _same_entries(hs, h)
    assert _bits(b, _device_run("rejecting")[2]) and _bits(p, _device_run("rejecting")[3])


# ---- 5. argument errors and the empty problem ----------------------------------------------------------------------------
def test_argument_errors(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L, solve
    ba = _load(_dome())
    b0 = ba.cameras_bal()
    for bad in (dict(function_tol=-1e-3), dict(gradient_tol=-1e-3), dict(parameter_tol=-1e-3), dict(parameter_tol=float("nan")),
                dict(lam=1e-21), dict(lam=1e33), dict(iterations=-1), dict(max_iters=-1)):
        with pytest.raises(c2b.City2baError) as ei:
            solve.levenberg_marquardt_device(ba, **bad)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT, bad
    opt = L.LmOptions(5, 100, 1e-4, 1e-6, 0.0, 0.0, 0.0)
    short = (L.LmIteration * 4)()
    assert L.lib().c2b_problem_levenberg_marquardt(ba._h, C.byref(opt), short, 4, None) == L.ERR_INVALID_ARGUMENT
    assert _bits(ba.cameras_bal(), b0)                       # a refused call changes nothing
    s = L.LmSummary()
    assert L.lib().c2b_problem_levenberg_marquardt(ba._h, C.byref(opt), None, 0, C.byref(s)) == 0      # history may be NULL
    assert s.iterations == 5 and s.final_cost < s.initial_cost
    assert L.lib().c2b_problem_levenberg_marquardt(ba._h, C.byref(opt), None, 0, None) == 0             # ... and the summary
    with pytest.raises(c2b.City2baError):
        ba.rollback()                                        # the loop's checkpoint is gone
    ba.close()


@pytest.mark.parametrize("n_cam,n_pts", [(5, 7), (0, 0), (3, 0), (0, 4)])
def test_a_problem_without_observations_stops_on_the_gradient(env, n_cam, n_pts):
    import city2ba_amd as c2b
    from city2ba_amd import solve
    P = random_problem(max(n_cam, 1), max(n_pts, 1), 1, seed=3)
    bal9, pts = P["bal9"][:n_cam], P["pts"][:n_pts]
    ba = c2b.BAProblem.from_bal(bal9, pts, np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)), device=0)
    h, s = solve.levenberg_marquardt_device(ba, 10, gradient_tol=1e-10)
    assert s["termination"] == 2 and s["iterations"] == 1 and len(h) == 1, s
    e = h[0]
    assert all(np.isfinite(v) for v in e.values()) and all(np.isfinite(v) for v in s.values() if not isinstance(v, str))
    assert e["gradient_max"] == 0.0 and e["step_norm"] == 0.0 and e["cost"] == 0.0 and s["final_cost"] == 0.0
    x = np.concatenate([bal9.ravel(), pts.ravel()]).astype(LD)
    assert abs(e["x_norm"] - float(np.sqrt(np.sum(x * x)))) <= 4 * max(x.size, 1) * EPS * e["x_norm"]
    assert _bits(ba.cameras_bal(), bal9) and _bits(ba.points(), pts)
    ba.close()
