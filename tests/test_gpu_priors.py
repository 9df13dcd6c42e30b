"""Priors on camera centres, intrinsics and points in the device step (BAProblem.set_priors / priors / prior_cost /
prior_residual_jacobian, levenberg_marquardt(priors=...)) against the longdouble references: tests/_priorref.py
for the prior rows themselves, and for everything else the references the solver's tests already use (_normref, _schurref,
_precondref, _robustref, _solvecheck) on the STACKED system -- the device's own Jacobian (BAProblem.residual_jacobian) with
the device's own prior rows appended as pseudo-observations (_priorref.stack).  Every bound is one a reference returns.

One set of priors serves the tests (_priors): targets a seeded perturbation of the current values; weights from 1e-3 to
1e3 with single zeros, whole cameras and most points without any, intrinsics priors on two cameras in three, and on
"random bal" a prior on a camera whose row is empty.  The targets under zero weights are NaN / inf: they may be anything."""
import numpy as np
import pytest

import _normref as N
import _precondref as PR
import _priorref as PRI
import _schurref as R
import _solvecheck as SC
import test_gpu_schur_jacobi as SJ
from test_gpu_schur_pcg import KS
from test_gpu_schur_step import EPS, _bits, _cam_of, _kappa, _level0, _make, _np, env  # noqa: F401  (env is the module fixture)
from test_priorref import DRIFT, DRIFT_GRADIENT_TOL, DRIFT_ITERATIONS, DRIFT_SIGMA

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _priors(ba, name, seed=3):
    """the keywords of ba.set_priors for the module's one set of priors on this problem"""
    rng = np.random.default_rng(seed)
    nc, npt = ba.num_cameras(), ba.num_points()
    C, I, X = ba._camera_centers(), ba.cameras_bal()[:, 6:9].copy(), ba.points()
    cw = 10.0 ** rng.uniform(-3, 3, size=(nc, 3))
    cw[rng.random((nc, 3)) < 0.2] = 0.0
    cw[1::4] = 0.0                                               # whole cameras without a centre prior
    cw[2], cw[3] = (1e3, 1e-3, 1.0), (1e-3, 0.0, 1e3)            # the span, whatever the draw
    iw = 10.0 ** rng.uniform(-3, 3, size=(nc, 3))
    iw[::3] = 0.0
    if name == "random bal":
        empty = [c for c in np.flatnonzero(np.diff(ba.row_ptr.astype(np.int64)) == 0) if 0 < c < nc - 1]
        assert empty, "no empty row"
        cw[empty[0]], iw[empty[0]] = (1e3, 1e-3, 2.0), (0.5, 0.0, 0.0)
    xw = 10.0 ** rng.uniform(-3, 3, size=(npt, 3))
    xw[rng.random(npt) < 0.7] = 0.0
    xw[rng.random((npt, 3)) < 0.1] = 0.0
    c0 = C + rng.normal(scale=1e-2, size=C.shape)
    i0 = I + np.array([1e-3, 1e-4, 1e-5]) * rng.normal(size=I.shape)
    x0 = X + rng.normal(scale=1e-2, size=X.shape)
    c0[cw == 0], i0[iw == 0], x0[xw == 0] = np.nan, np.inf, -np.inf
    assert (cw > 0).any(axis=1).sum() < nc and 0 < (xw > 0).any(axis=1).sum() < npt
    span = np.concatenate([cw[cw > 0], iw[iw > 0], xw[xw > 0]])
    assert span.min() <= 1e-3 and span.max() >= 1e3
    return dict(camera_centers=c0, camera_center_weights=cw, intrinsics=i0, intrinsics_weights=iw, points=x0, point_weights=xw)


def _with_priors(name, kind="block_jacobi"):
    ba, bal = _make(name)
    kw = _priors(ba, name)
    ba.set_preconditioner(kind)
    ba.set_priors(**kw)
    return ba, bal, kw


def _prior_rows(ba, kw):
    """the device's own prior rows as _priorref.stack takes them"""
    r_cam, A_cam, r_pt = ba.prior_residual_jacobian()
    return dict(r_cam=r_cam, A_cam=A_cam, iw=kw.get("intrinsics_weights"), r_pt=r_pt, xw=kw.get("point_weights"))


def _lin(ba):
    r, Jc, Jp = ba.residual_jacobian()
    return r, Jc, Jp, _cam_of(ba.row_ptr), ba.pt_idx.astype(np.int64), ba.num_cameras(), ba.num_points()


def _stacked(ba, kw, dtype=np.float64, loss=None, mask=None):
    return PRI.stacked_problem(*_lin(ba), _prior_rows(ba, kw), loss=loss, mask=mask, dtype=dtype)


# ---- 1. the prior rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random bal", "random state", "mixed k2"])
def test_prior_residuals_and_jacobian_follow_the_longdouble_reference(env, name):
    """r_C, r_I, r_X and A against _priorref evaluated from the camera records the device read (device.camblk_records of the
    table of the problem's mode).  First-order bounds with the kernel's operation counts (prior_kernels.hpp states them next
    to the kernel; _priorref.DEVICE_OPS_*): 6 + 1 roundings x 2^-53 x w (|R^T| |[t]x| |J_l|) for the rotation columns, 1 + 1
    for the translation columns, 2 + 1 for a residual -- the + 1 is the reference's own rounding to f64."""
    D = env["D"]
    ba, bal, kw = _with_priors(name)
    camblk = _level0(env, ba, bal)[0]
    rec = _np(D.camblk_records(camblk))
    ref = PRI.camera_rows_from_records(rec, kw["camera_centers"], kw["camera_center_weights"], kw["intrinsics"], kw["intrinsics_weights"])
    refp = PRI.point_rows(ba.points(), kw["points"], kw["point_weights"])
    r_cam, A_cam, r_pt = ba.prior_residual_jacobian()
    assert np.isfinite(r_cam).all() and np.isfinite(A_cam).all() and np.isfinite(r_pt).all()
    worst = {}
    for key, dev, want, E in (("r_cam", r_cam, ref["r"], ref["E_r"]), ("A", A_cam, ref["A"], ref["E_A"]), ("r_pt", r_pt, refp["r"], refp["E_r"])):
        err = np.abs(dev.astype(LD) - want).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / E)
        worst[key] = float(q.max())
        assert (err <= E).all(), (name, key, worst[key])
    print("PRIOR rows %s: worst |err| / bound %s" % (name, {k: "%.3g" % v for k, v in worst.items()}))
    off = kw["camera_center_weights"] == 0
    assert not r_cam[:, :3][off].any() and not A_cam[np.broadcast_to(off[:, :, None], A_cam.shape)].any()
    assert not r_cam[:, 3:][kw["intrinsics_weights"] == 0].any() and not r_pt[kw["point_weights"] == 0].any()
    assert r_cam.any() and A_cam.any() and r_pt.any()
    ba.close()


# ---- 2. the blocks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random bal", "random state", "mixed k2", "small grid culled"])
def test_normal_equations_are_those_of_the_stacked_system(env, name):
    ba, _, kw = _with_priors(name)
    plain = [_np(t).copy() for t in _make(name)[0].normal_equations()[:4]]
    U, gc, V, gp, ss = ba.normal_equations()
    ref = PRI.stacked_blocks(*_lin(ba), _prior_rows(ba, kw))
    N.check((_np(U), _np(gc), _np(V), _np(gp)), ref, "priors " + name)
    assert not _bits(_np(U), plain[0]) and not _bits(_np(V), plain[2])           # the priors did something
    # sum_sq is the stacked system's, by _solvecheck.check_iterates' tolerance, whichever passes the call runs
    want = float(ref["sum_sq"])
    for s in (ss, ba.normal_equations(out=(None, None, None, None))[4], ba.normal_equations(out=(U, gc, None, None))[4],
              ba.normal_equations(out=(None, None, V, gp))[4]):
        assert abs(s - want) <= 1e-13 * want, (s, want)
    ba.close()


# ---- 3. every iterate -------------------------------------------------------------------------------------------------------
def _iterates(monkeypatch, ba, kw, lam, ks, kind, tag, runs=8, loss=None, mask=None):
    """test_gpu_schur_jacobi._check_iterates, its bounds as they are, on the stacked reference problem"""
    monkeypatch.setattr(SJ, "_ref", lambda p, dtype=np.float64: _stacked(p, kw, dtype=dtype, loss=loss, mask=mask))
    return SJ._check_iterates(ba, lam, ks, runs=runs, tag="priors " + tag, kind=kind)


@pytest.mark.parametrize("name", ["random bal", "random state", "mixed k2", "small grid culled"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_block_jacobi_iterates_follow_the_stacked_reference(env, monkeypatch, name, lam):
    ba, _, kw = _with_priors(name)
    _iterates(monkeypatch, ba, kw, lam, KS, "block_jacobi", name)
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_schur_jacobi_iterates_follow_the_stacked_reference(env, monkeypatch, lam):
    ba, _, kw = _with_priors("small grid culled", "schur_jacobi")
    _iterates(monkeypatch, ba, kw, lam, KS, "schur_jacobi", "small grid culled")
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


# ---- 4. the converged step against a dense solve ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small grid culled", "random bal"])
def test_converged_step_is_the_dense_solution_of_the_stacked_problem(env, name):
    """test_gpu_schur_step.test_solve_accuracy's tolerances, on the stacked Problem"""
    lam = 1.0
    ba, _, kw = _with_priors(name)
    ref = _stacked(ba, kw)
    dc, dp, info = ba.solve_step(lam, max_iters=5000, rel_tol=1e-12)
    dc, dp = _np(dc), _np(dp)
    assert info["status"] == 0 and info["rel_residual"] <= 1e-12, info
    kappa = _kappa(ref, lam)
    tol_res = max(1e-9, 1e3 * EPS * kappa)
    res, g = ref.damped_residual(lam, dc, dp)
    assert np.linalg.norm(res) <= tol_res * np.linalg.norm(g), (name, kappa, np.linalg.norm(res) / np.linalg.norm(g))
    wc, wp = ref.direct(lam)
    d, w = np.concatenate([dc.ravel(), dp.ravel()]), np.concatenate([wc.ravel(), wp.ravel()])
    print("PRIOR dense %s: |d - w| / |w| %.3g, kappa %.3g, iterations %d" % (name, np.linalg.norm(d - w) / np.linalg.norm(w), kappa, info["iterations"]))
    assert np.linalg.norm(d - w) <= max(1e-8, kappa * tol_res) * np.linalg.norm(w), (name, kappa)
    md = float(_stacked(ba, kw, dtype=LD).model_decrease(dc, dp))
    assert md > 0 and abs(info["model_decrease"] - md) <= 1e-10 * md, (info["model_decrease"], md)
    e2 = ba.total_reprojection_error(2.0) ** 2 + ba.prior_cost()
    assert abs(info["sum_sq"] - e2) <= 1e-12 * e2
    ba.close()


# ---- 5. the priors reach the operator -----------------------------------------------------------------------------------------
def test_step_with_priors_is_not_the_step_without(env):
    """the form of test_gpu_constant.test_masked_step_is_not_the_unmasked_step_with_entries_overwritten"""
    name, lam, k = "small grid culled", 1.0, max(KS)
    ba, _, kw = _with_priors(name)
    tied = PR.pcg(_stacked(ba, kw, dtype=LD), lam, k, 0.0, kind="block_jacobi", runs=3)
    dct = _np(ba.solve_step(lam, max_iters=k, rel_tol=0.0)[0]).copy()
    ba.set_priors()
    plain = PR.pcg(SJ._ref(ba, R.LD), lam, k, 0.0, kind="block_jacobi", runs=3)
    dcu = _np(ba.solve_step(lam, max_iters=k, rel_tol=0.0)[0]).copy()
    gap = float(np.linalg.norm(dct - dcu))
    bound = tied["bound"]["x"][k] + plain["bound"]["x"][k]
    ref_gap = float(np.linalg.norm((tied["x"][k] - plain["x"][k]).astype(np.float64)))
    print("PRIOR operator: |dc with - dc without| %.3g (reference %.3g), both bounds %.3g" % (gap, ref_gap, bound))
    assert gap > bound, (gap, bound)
    ba.close()


# ---- 6. masks and a loss --------------------------------------------------------------------------------------------------------
def test_iterates_under_priors_a_mask_and_cauchy(env, monkeypatch):
    from test_gpu_constant import _mask
    name, lam = "random bal", 1e-2
    ba, _, kw = _with_priors(name)
    cm, pm = _mask(ba, name)
    assert (kw["camera_center_weights"][SC.unpack(cm)[:, 3:6].any(axis=1)] > 0).any() and (kw["point_weights"][pm] > 0).any()
    ba.set_constant(cm, pm)
    r = ba.residual_jacobian()[0]
    a = 3.0 * float(np.sqrt(np.mean(r * r)))
    ba.set_loss("cauchy", a)
    ks = (0, 1, 3)
    ref = _iterates(monkeypatch, ba, kw, lam, ks, "block_jacobi", name + " mask cauchy", loss=("cauchy", a), mask=(cm, pm))
    free = ~SC.unpack(cm)
    for k in ks:
        assert not ref["x"][k][~free].any() and not ref["dp"][k][pm].any()
        dc, dp, _ = ba.solve_step(lam, max_iters=k, rel_tol=0.0)
        SC.assert_zeros(_np(dc), _np(dp), cm, pm, (name, k))
    kept = _np(ba.solve_step(lam, max_iters=3, rel_tol=0.0)[0]).copy()
    ba.set_priors()
    assert not _bits(_np(ba.solve_step(lam, max_iters=3, rel_tol=0.0)[0]), kept)
    ba.close()


# ---- 7. bits --------------------------------------------------------------------------------------------------------------------
def _step_bits(ba, lam=1e-4, k=5):
    dc, dp, info = ba.solve_step(lam, max_iters=k, rel_tol=0.0)
    return _np(dc).copy(), _np(dp).copy(), info


def _ne_bits(ba):
    U, gc, V, gp, ss = ba.normal_equations()
    return [_np(t).copy() for t in (U, gc, V, gp)] + [ss]


def _same(a, b):
    return all(_bits(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["block_jacobi", "schur_jacobi"])
def test_no_priors_is_bit_for_bit_what_it_was_and_priors_are_deterministic(env, kind):
    from city2ba_amd.solve import levenberg_marquardt_device
    name = "small grid culled"
    fresh, _ = _make(name)
    fresh.set_preconditioner(kind)
    want_step, want_ne = _step_bits(fresh), _ne_bits(fresh)
    want_lm = levenberg_marquardt_device(fresh, 3)
    want_state = (fresh.cameras_bal(), fresh.points())
    fresh.close()
    nc, npt = None, None
    for how in ("none", "cleared", "zero weights"):
        ba, _ = _make(name)
        ba.set_preconditioner(kind)
        nc, npt = ba.num_cameras(), ba.num_points()
        if how == "cleared":
            ba.set_priors(**_priors(ba, name))
            assert any(ba.priors["active"])
            ba.set_priors()
        elif how == "zero weights":
            ba.set_priors(camera_centers=np.full((nc, 3), np.nan), camera_center_weights=0.0, intrinsics_weights=np.zeros(3),
                          points=np.zeros((npt, 3)), point_weights=np.zeros((npt, 3)))
        assert ba.priors["active"] == (0, 0, 0) and ba.prior_cost() == 0.0
        assert _same(_step_bits(ba), want_step) and _same(_ne_bits(ba), want_ne), how
        assert levenberg_marquardt_device(ba, 3) == want_lm, how
        assert _bits(ba.cameras_bal(), want_state[0]) and _bits(ba.points(), want_state[1]), how
        ba.close()
    ba, _, kw = _with_priors(name, kind)
    a, b = _step_bits(ba), _step_bits(ba)
    assert _same(a, b) and not _bits(a[0], want_step[0])
    assert _same(_ne_bits(ba), _ne_bits(ba)) and ba.prior_cost() == ba.prior_cost()
    ba.close()
    ba, _, _ = _with_priors(name, kind)                          # the same priors on a second handle
    assert _same(_step_bits(ba), a)
    ba.close()


# ---- 8. lifetime and arguments ------------------------------------------------------------------------------------------------------
def test_priors_round_trip_survive_uploads_and_leave_with_a_cull(env, monkeypatch):
    import city2ba_amd.solve as S
    from city2ba_amd import _lib as L
    name = "small grid"
    ba, _ = _make(name)
    nc, npt = ba.num_cameras(), ba.num_points()
    assert ba.priors["active"] == (0, 0, 0) and not ba.priors["point_weights"].any()
    kw = _priors(ba, name)
    names = ("camera_centers", "camera_center_weights", "intrinsics", "intrinsics_weights", "points", "point_weights")

    def in_force():
        got = ba.priors
        act = tuple(int((kw[k] > 0).any(axis=1).sum()) for k in names[1::2])
        return got["active"] == act and all(_bits(got[k], kw[k]) for k in names)

    ba.set_priors(**kw)
    assert in_force()
    # a scalar and a length-3 weight broadcast; a target left out is the current value, whose residual is 0
    ba.set_priors(camera_center_weights=2.0, point_weights=[1.0, 0.0, 3.0])
    got = ba.priors
    assert (got["camera_center_weights"] == 2.0).all() and (got["point_weights"] == np.array([1.0, 0.0, 3.0])).all()
    assert _bits(got["points"], ba.points()) and got["active"] == (nc, 0, npt)
    assert ba.prior_cost() <= 1e-20 and not ba.prior_residual_jacobian()[2].any()
    ba.set_priors(**kw)
    # refused arguments leave the priors in force
    for key, value in (("camera_center_weights", -1.0), ("point_weights", np.nan), ("intrinsics_weights", np.inf)):
        bad = dict(kw)
        bad[key] = kw[key].copy()
        bad[key][5, 1] = value
        with pytest.raises(L.City2baError) as e:
            ba.set_priors(**bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT == -1 and in_force()
    bad = dict(kw, points=kw["points"].copy())
    bad["points"][np.argwhere(kw["point_weights"] > 0)[0][0]] = np.nan            # a non-finite target under a positive weight
    with pytest.raises(L.City2baError):
        ba.set_priors(**bad)
    with pytest.raises(ValueError):
        ba.set_priors(points=kw["points"])                           # a target without weights
    with pytest.raises(ValueError):
        ba.set_priors(points=kw["points"][:-1], point_weights=1.0)
    assert in_force()
    # the handle's other settings, a step, noise-free uploads of the same counts, checkpoint / rollback and LM runs keep them
    ba.set_loss("huber", 1.0)
    ba.set_loss(None)
    ba.set_preconditioner("schur_jacobi")
    ba.set_preconditioner("block_jacobi")
    ba.set_constant(np.full(nc, 0x040, dtype=np.uint16), None)
    ba.set_constant(None, None)
    dc, dp, _ = ba.solve_step(1e-3)
    ba.checkpoint()
    ba.apply_step(dc, dp)
    assert in_force()
    ba.rollback()
    ba._upload(ba.cameras_bal(), True, ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
    assert in_force()
    orig = type(ba).solve_step

    def wrong_way(self, lam, max_iters=100, rel_tol=1e-6, out=None):
        dc, dp, info = orig(self, lam, max_iters, rel_tol, out)
        return -dc * 1e3, -dp * 1e3, info

    b0 = ba.cameras_bal()
    with monkeypatch.context() as m:                                 # a rejected LM step
        m.setattr(type(ba), "solve_step", wrong_way)
        hist = S.levenberg_marquardt(ba, 2, lam=1e-4)
    assert not any(h["accepted"] for h in hist) and _bits(ba.cameras_bal(), b0) and in_force()
    hist, _ = S.levenberg_marquardt_device(ba, 2, lam=1e-4)
    assert len(hist) == 2 and in_force()
    # one kind alone
    ba.set_priors(points=kw["points"], point_weights=kw["point_weights"])
    assert ba.priors["active"][:2] == (0, 0) and ba.priors["active"][2] > 0 and not ba.priors["camera_center_weights"].any()
    # priors and no observation at all: a documented limit
    ba.set_priors(**kw)
    # a cull renumbers the entities: the priors go
    ba.cull()
    assert ba.num_cameras() < nc or ba.num_points() < npt
    assert ba.priors["active"] == (0, 0, 0) and ba.prior_cost() == 0.0
    # an upload of another size drops them too
    ba.set_priors(camera_center_weights=1.0)
    assert ba.priors["active"][0] == ba.num_cameras()
    b9, pts, rp, pi, uv = ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations()
    ba._upload(b9, True, np.concatenate([pts, pts[:1]]), rp, pi, uv)
    assert ba.priors["active"] == (0, 0, 0)
    # no observation at all: the step is refused with priors in force and is the zero step without
    ba._upload(b9, True, pts, np.zeros(len(b9) + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)))
    assert ba.solve_step(1e-3)[2]["iterations"] == 0
    ba.set_priors(camera_center_weights=1.0)
    with pytest.raises(L.City2baError) as e:
        ba.solve_step(1e-3)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(L.City2baError):
        S.levenberg_marquardt_device(ba, 1)
    ba.close()


# ---- 9. the LM loops --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random bal", "mixed k2", "small grid culled"])
def test_device_loop_is_the_python_loop_with_priors(env, name):
    """test_gpu_lm_device.test_device_loop_is_the_python_loop's criterion with priors in force; the cost in the history is
    the observations' cost + prior_cost(); prior_cost() alone is the reference's sum within _normref's form of bound: each
    of the n rows' squares rounds once and n - 1 additions follow, (n + 4) 2^-53, and a row itself carries
    _priorref.DEVICE_OPS_R roundings, twice that in its square."""
    from city2ba_amd import solve
    kw = None
    runs = []
    for loop in (solve.levenberg_marquardt, lambda ba, n, **k: solve.levenberg_marquardt_device(ba, n, **k)[0]):
        ba, _ = _make(name)
        kw = kw or _priors(ba, name)
        if loop is solve.levenberg_marquardt:
            ba.set_priors(**kw)
            rows = _prior_rows(ba, kw)
            want = float(PRI.prior_cost(rows["r_cam"], rows["r_pt"]))
            n = rows["r_cam"].size + rows["r_pt"].size
            got = ba.prior_cost()
            assert abs(got - want) <= (n + 4 + 2 * PRI.DEVICE_OPS_R) * N.U53 * want, (got, want)
            ba.apply_step(None, None)
            first = ba.total_reprojection_error(2.0) ** 2 + ba.prior_cost()
            ba.close()
            ba, _ = _make(name)
        h = loop(ba, 6, lam=1e-3, priors=kw)
        assert any(ba.priors["active"])                              # priors= stays on ba
        runs.append((h, ba.cameras_bal(), ba.points(), ba.total_reprojection_error(2.0) ** 2 + ba.prior_cost()))
        ba.close()
    (hp, bp, pp, ep), (hd, bd, pd, ed) = runs
    print("PRIOR LM %s: accepted %s cost %.6g -> %.6g" % (name, "".join("A" if e["accepted"] else "R" for e in hd), hd[0]["error"], ed))
    assert len(hp) == len(hd) == 6
    for k, (a, b) in enumerate(zip(hp, hd)):
        for key in ("accepted", "pcg_iterations", "status", "error", "cost", "lam"):
            assert a[key] == b[key], (name, k, key, a[key], b[key])
    assert hp[-1]["error_after"] == hd[-1]["error_after"] == ep == ed and hd[0]["cost"] == first
    assert _bits(bp, bd) and _bits(pp, pd)
    assert any(e["accepted"] for e in hd) and hd[-1]["error_after"] < hd[0]["error"]


# ---- 10. drift ------------------------------------------------------------------------------------------------------------------------
def test_centre_priors_undo_a_drift(env):
    """noise.add_drift(**DRIFT) on "small grid culled", centre priors of sigma = DRIFT_SIGMA at the clean centres, up to
    DRIFT_ITERATIONS iterations with gradient_tol = DRIFT_GRADIENT_TOL.  Orderings only: the mean distance to the clean
    centres after the solve with priors is below the start's and below the unanchored solve's, and the solve with priors
    stops on the gradient tolerance of the stacked system.  Checked on the CPU before any device saw it, with a host loop
    over the stacked reference (tests/test_priorref.py::test_centre_priors_undo_a_drift_on_the_host, these very values:
    strength 0.01, angle 0.002, std 0.01, sigma 0.3, 40 iterations, tolerance 1e-3): start 0.838, unanchored 0.845 after
    24 iterations, with priors 7.8e-4 after 5."""
    from city2ba_amd import noise, solve

    def run(priors):
        ba, _ = _make("small grid culled")
        clean = ba._camera_centers()
        noise.add_drift(ba, DRIFT["strength"], DRIFT["angle_strength"], DRIFT["std"], DRIFT["dir"], seed=DRIFT["seed"])
        dist = lambda: float(np.mean(np.linalg.norm(ba._camera_centers() - clean, axis=1)))
        start = dist()
        kw = dict(camera_centers=clean, camera_center_weights=1.0 / DRIFT_SIGMA) if priors else None
        h, s = solve.levenberg_marquardt_device(ba, DRIFT_ITERATIONS, lam=1e-4, max_iters=200, rel_tol=1e-8,
                                                gradient_tol=DRIFT_GRADIENT_TOL, priors=kw)
        out = (start, dist(), s, len(h))
        ba.close()
        return out

    start, free, sf, nf = run(False)
    start2, tied, st, nt = run(True)
    print("PRIOR drift: start %.4g, unanchored %.4g after %d iterations (termination %d), with priors %.4g after %d (termination %d)" % (
        start, free, nf, sf["termination"], tied, nt, st["termination"]))
    assert start == start2
    assert tied < start and tied < free, (start, free, tied)
    assert st["termination"] == 2, st
