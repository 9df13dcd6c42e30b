"""Constant camera parameters and points in the device step (BAProblem.set_constant / constant,
levenberg_marquardt(constant=...)) against the longdouble references of tests/_schurref.py, _precondref.py and
_robustref.py built from J~: the device's own Jacobian (BAProblem.residual_jacobian) with the constant columns set to
zero in numpy.  Every bound is one the reference returns, used as test_gpu_schur_jacobi._check_iterates uses it; the
constant entries of a step are asserted == 0.0 on their own.

One mask serves every test (_mask): camera 0 wholly constant, the intrinsics of every even camera, five seeded single
bits, the pose of the last camera, a seeded 10 % of the points with the last point among them, and on "random bal" one
empty camera with constant parameters and one without."""
import numpy as np
import pytest

import _precondref as PR
import _robustref as B
import _schurref as R
import _solvecheck as SC
import test_gpu_schur_jacobi as SJ
from test_gpu_schur_pcg import KS
from test_gpu_schur_step import EPS, _bits, _cam_of, _kappa, _make, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
ROTATION, TRANSLATION, POSE, FOCAL, K1, K2, INTRINSICS, ALL = 0x007, 0x038, 0x03f, 0x040, 0x080, 0x100, 0x1c0, 0x1ff


_unpack = SC.unpack


def _mask(ba, name):
    """(uint16 [n_cam], bool [n_pts]) of the module's one mask on this problem"""
    nc, npt = ba.num_cameras(), ba.num_points()
    rng = np.random.default_rng(2024)
    cm = np.zeros(nc, dtype=np.uint16)
    cm[::2] |= INTRINSICS
    cm[0] = ALL
    for c, k in zip(rng.integers(1, nc - 1, size=5), rng.integers(0, 9, size=5)):
        cm[c] |= np.uint16(1 << int(k))
    cm[-1] = POSE
    pm = rng.random(npt) < 0.1
    pm[-1] = True
    if name == "random bal":
        empty = [c for c in np.flatnonzero(np.diff(ba.row_ptr.astype(np.int64)) == 0) if 0 < c < nc - 1]
        assert len(empty) >= 2, empty
        cm[empty[0]] = TRANSLATION | K1
        cm[empty[1]] = 0
    assert 0 < pm.sum() < npt and (cm == 0).any()
    return cm, pm


def _lin(ba, cm, pm):
    """the arguments of _schurref.Problem / _robustref.problem for J~"""
    r, Jc, Jp = ba.residual_jacobian()
    cam, pt = _cam_of(ba.row_ptr), ba.pt_idx.astype(np.int64)
    Jc, Jp = SC.masked_jacobian(Jc, Jp, cam, pt, cm, pm)
    return r, Jc, Jp, cam, pt, ba.num_cameras(), ba.num_points()


def _masked(name, kind="block_jacobi"):
    ba, bal = _make(name)
    cm, pm = _mask(ba, name)
    ba.set_preconditioner(kind)
    ba.set_constant(cm, pm)
    return ba, bal, cm, pm


_assert_zeros = SC.assert_zeros


def _iterates(monkeypatch, ba, cm, pm, lam, ks, kind, tag, runs=8, loss=None):
    """test_gpu_schur_jacobi._check_iterates, its bounds as they are, on the reference problem of J~; then the zeros"""
    if loss is None:
        make = lambda p, dtype=np.float64: R.Problem(*_lin(p, cm, pm), dtype=dtype)
    else:
        make = lambda p, dtype=np.float64: B.problem(loss[0], loss[1], *_lin(p, cm, pm), dtype=dtype)
    monkeypatch.setattr(SJ, "_ref", make)
    ref = SJ._check_iterates(ba, lam, ks, runs=runs, tag="constant " + tag, kind=kind)
    free = ~_unpack(cm)
    for k in ks:
        assert not ref["x"][k][~free].any() and not ref["dp"][k][pm].any()       # the reference's own are exact zeros
        dc, dp, _ = ba.solve_step(lam, max_iters=k, rel_tol=0.0)
        _assert_zeros(_np(dc), _np(dp), cm, pm, (tag, lam, k))
    return ref


# ---- 1. every iterate -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random bal", "random state", "small grid culled"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_block_jacobi_iterates_follow_the_masked_reference(env, monkeypatch, name, lam):
    ba, _, cm, pm = _masked(name)
    _iterates(monkeypatch, ba, cm, pm, lam, KS, "block_jacobi", name)
    ba.close()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_schur_jacobi_iterates_follow_the_masked_reference(env, monkeypatch, lam):
    ba, _, cm, pm = _masked("small grid culled", "schur_jacobi")
    _iterates(monkeypatch, ba, cm, pm, lam, KS, "schur_jacobi", "small grid culled")
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


@pytest.mark.parametrize("name", ["random bal", "random state"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_schur_jacobi_on_block_diagonal_problems_converges_in_one_iteration(env, monkeypatch, name, lam):
    """as test_gpu_schur_jacobi.test_block_diagonal_problems_converge_in_one_iteration: every point is seen once, so the
    M of J~ is the S of J~"""
    ba, _, cm, pm = _masked(name, "schur_jacobi")
    assert len(np.unique(ba.pt_idx)) == len(ba.pt_idx)
    ref = _iterates(monkeypatch, ba, cm, pm, lam, (0, 1), "schur_jacobi", name)
    tol = min(float(ref["rel"][1]) + ref["bound"]["rel"][1], float(np.sqrt(R.EPS)))
    dc, dp, info = ba.solve_step(lam, max_iters=50, rel_tol=tol)
    assert info["status"] == 0 and info["iterations"] == 1 and info["rel_residual"] <= tol, (name, lam, tol, info)
    _assert_zeros(_np(dc), _np(dp), cm, pm, name)
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


# ---- 2. the converged step against a dense solve ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small grid culled", "random bal"])
def test_converged_step_is_the_dense_solution_of_the_masked_problem(env, name):
    """test_gpu_schur_step.test_solve_accuracy's tolerances, on Problem(J~)"""
    lam = 1.0
    ba, _, cm, pm = _masked(name)
    ref = R.Problem(*_lin(ba, cm, pm))
    dc, dp, info = ba.solve_step(lam, max_iters=5000, rel_tol=1e-12)
    dc, dp = _np(dc), _np(dp)
    assert info["status"] == 0 and info["rel_residual"] <= 1e-12, info
    _assert_zeros(dc, dp, cm, pm, name)
    kappa = _kappa(ref, lam)
    tol_res = max(1e-9, 1e3 * EPS * kappa)
    res, g = ref.damped_residual(lam, dc, dp)
    assert np.linalg.norm(res) <= tol_res * np.linalg.norm(g), (name, kappa, np.linalg.norm(res) / np.linalg.norm(g))
    wc, wp = ref.direct(lam)
    assert not wc[_unpack(cm)].any() and not wp[pm].any()
    d, w = np.concatenate([dc.ravel(), dp.ravel()]), np.concatenate([wc.ravel(), wp.ravel()])
    print("CONST dense %s: |d - w| / |w| %.3g, kappa %.3g, iterations %d" % (name, np.linalg.norm(d - w) / np.linalg.norm(w), kappa,
                                                                              info["iterations"]))
    assert np.linalg.norm(d - w) <= max(1e-8, kappa * tol_res) * np.linalg.norm(w), (name, kappa)
    ba.close()


# ---- 3. the mask reaches the operator ------------------------------------------------------------------------------------
def test_masked_step_is_not_the_unmasked_step_with_entries_overwritten(env):
    name, lam, k = "small grid culled", 1.0, max(KS)
    ba, _, cm, pm = _masked(name)
    free = ~_unpack(cm)
    masked = PR.pcg(R.Problem(*_lin(ba, cm, pm), dtype=R.LD), lam, k, 0.0, kind="block_jacobi", runs=3)
    dcm = _np(ba.solve_step(lam, max_iters=k, rel_tol=0.0)[0]).copy()
    ba.set_constant(None, None)
    plain = PR.pcg(SJ._ref(ba, R.LD), lam, k, 0.0, kind="block_jacobi", runs=3)
    dcu = _np(ba.solve_step(lam, max_iters=k, rel_tol=0.0)[0]).copy()
    gap = float(np.linalg.norm(dcm[free] - dcu[free]))
    bound = masked["bound"]["x"][k] + plain["bound"]["x"][k]
    ref_gap = float(np.linalg.norm((masked["x"][k] - plain["x"][k])[free].astype(np.float64)))
    print("CONST operator: |dc masked - dc unmasked| on the free entries %.3g (reference %.3g), both bounds %.3g" % (gap, ref_gap, bound))
    assert gap > bound, (gap, bound)
    ba.close()


# ---- 4. normal_equations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random bal", "random state", "small grid culled"])
def test_normal_equations_under_the_mask(env, name):
    ba, _ = _make(name)
    cm, pm = _mask(ba, name)
    want = [_np(t).copy() for t in ba.normal_equations()[:4]] + [ba.normal_equations()[4]]
    ba.set_constant(cm, pm)
    U, gc, V, gp, ss = ba.normal_equations()
    U, gc, V, gp = _np(U), _np(gc), _np(V), _np(gp)
    m = _unpack(cm)
    block = m[:, :, None] | m[:, None, :]
    assert (U[block] == 0.0).all() and (gc[m] == 0.0).all() and (V[pm] == 0.0).all() and (gp[pm] == 0.0).all()
    assert _bits(U[~block], want[0][~block]) and _bits(gc[~m], want[1][~m])
    assert _bits(V[~pm], want[2][~pm]) and _bits(gp[~pm], want[3][~pm])
    assert want[0][block].any() and want[2][pm].any()                # the mask had something to remove
    assert ss == want[4]
    ba.close()


# ---- 5. bits ------------------------------------------------------------------------------------------------------------
def _step_bits(ba, lam=1e-4, k=5):
    dc, dp, info = ba.solve_step(lam, max_iters=k, rel_tol=0.0)
    return _np(dc).copy(), _np(dp).copy(), info


def _same(a, b):
    return _bits(a[0], b[0]) and _bits(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("kind", ["block_jacobi", "schur_jacobi"])
def test_no_mask_is_bit_for_bit_the_step_it_was_and_a_mask_is_deterministic(env, kind):
    name = "small grid culled"
    ba, _ = _make(name)
    ba.set_preconditioner(kind)
    nc, npt = ba.num_cameras(), ba.num_points()
    want = _step_bits(ba)
    ba.set_constant(None, None)
    assert _same(_step_bits(ba), want)
    ba.set_constant(np.zeros(nc, dtype=np.uint16), np.zeros(npt, dtype=bool))
    assert _same(_step_bits(ba), want)
    cm, pm = _mask(ba, name)
    ba.set_constant(cm, pm)
    a, b = _step_bits(ba), _step_bits(ba)
    assert _same(a, b) and not _bits(a[0], want[0])
    ba.set_constant(None, None)
    assert _same(_step_bits(ba), want)
    ba.close()


def test_apply_step_leaves_constant_entries_bit_for_bit(env):
    torch = env["torch"]
    ba, bal, cm, pm = _masked("random bal")
    assert bal
    m = _unpack(cm)
    b0, x0 = ba.cameras_bal(), ba.points()
    dc, dp, _ = ba.solve_step(1e-3)
    ba.apply_step(dc, dp)
    b1, x1 = ba.cameras_bal(), ba.points()
    assert _bits(b1[m], b0[m]) and _bits(x1[pm], x0[pm])
    assert _bits(b1[~m], (b0 + _np(dc))[~m]) and _bits(x1[~pm], (x0 + _np(dp))[~pm])      # the free entries took the step
    assert not _bits(b1[~m], b0[~m]) and not _bits(x1[~pm], x0[~pm])
    # whatever a caller's step holds there, -0.0 included: b + (-0.0) would keep b, -0.0 + 0.0 would not
    ba.apply_step(torch.ones_like(dc), torch.ones_like(dp))
    b2, x2 = ba.cameras_bal(), ba.points()
    assert _bits(b2[m], b0[m]) and _bits(x2[pm], x0[pm]) and _bits(b2[~m], b1[~m] + 1.0) and _bits(x2[~pm], x1[~pm] + 1.0)
    ba.close()
    # state mode: the constant entries are the bits to_vec(cam15) produced
    ba, bal, cm, pm = _masked("random state")
    assert not bal
    m = _unpack(cm)
    vec, x0 = ba.cameras_bal(), ba.points()
    dc, dp, _ = ba.solve_step(1e-3)
    ba.apply_step(dc, dp)
    b1, x1 = ba.cameras_bal(), ba.points()
    assert _bits(b1[m], vec[m]) and _bits(x1[pm], x0[pm]) and _bits(b1[~m], (vec + _np(dc))[~m])
    ba.close()


# ---- 6. limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["block_jacobi", "schur_jacobi"])
def test_every_camera_constant_is_triangulation(env, kind):
    name, lam = "small grid culled", 1e-2
    ba, _ = _make(name)
    ba.set_preconditioner(kind)
    nc, npt = ba.num_cameras(), ba.num_points()
    cm, pm = np.full(nc, ALL, dtype=np.uint16), np.zeros(npt, dtype=bool)
    ba.set_constant(cm, None)
    P = R.Problem(*_lin(ba, cm, pm), dtype=R.LD)
    ref = PR.pcg(P, lam, 0, 0.0, kind=kind, runs=8)
    dc, dp, info = ba.solve_step(lam, max_iters=50, rel_tol=1e-6)
    dc, dp = _np(dc), _np(dp)
    assert info["iterations"] == 0 and info["status"] == 0 and info["rel_residual"] == 0.0, info
    assert (dc == 0.0).all() and dp.any()
    # the reference's iterate 0 is x = 0 and its back-substitution: dp = -V_l^-1 gp
    assert not ref["x"][0].any()
    err = float(np.linalg.norm(dp - ref["dp"][0].astype(np.float64)))
    assert err <= ref["bound"]["dp"][0], (err, ref["bound"]["dp"][0])
    assert info["model_decrease"] > 0
    ba.close()


def test_every_point_constant_is_resection(env):
    name, lam = "small grid culled", 1e-2
    ba, _ = _make(name)
    cm, _ = _mask(ba, name)
    pm = np.ones(ba.num_points(), dtype=bool)
    ba.set_constant(cm, pm)
    dc, dp, info = ba.solve_step(lam, max_iters=50, rel_tol=1e-10)     # S = U_l is its own block-Jacobi preconditioner
    assert info["status"] == 0 and info["iterations"] == 1 and info["rel_residual"] <= 1e-10, info
    dc, dp = _np(dc), _np(dp)
    assert (dp == 0.0).all() and dc.any()
    _assert_zeros(dc, dp, cm, pm, name)
    ba.close()


# ---- 7. a robust loss with a mask ---------------------------------------------------------------------------------------
def test_iterates_under_cauchy_and_a_mask(env, monkeypatch):
    name, lam = "random bal", 1e-2
    ba, _, cm, pm = _masked(name)
    r = ba.residual_jacobian()[0]
    a = 3.0 * float(np.sqrt(np.mean(r * r)))
    ba.set_loss("cauchy", a)
    _iterates(monkeypatch, ba, cm, pm, lam, (0, 1, 3), "block_jacobi", name + " cauchy", loss=("cauchy", a))
    plain = _step_bits(ba, lam, 3)
    ba.set_loss(None)
    assert not _bits(_step_bits(ba, lam, 3)[0], plain[0])            # the weights did something
    ba.close()


# ---- 8. several workgroups, a partly empty last wave ------------------------------------------------------------------------
def test_mid_grid_iterates_follow_the_masked_reference(env, monkeypatch):
    ba, _, cm, pm = _masked("mid grid")
    assert ba.num_cameras() == 2879
    _iterates(monkeypatch, ba, cm, pm, 1e-4, (0, 1, 3), "block_jacobi", "mid grid", runs=3)
    ba.close()


# ---- 9. lifetime and arguments ----------------------------------------------------------------------------------------------
def test_masks_round_trip_survive_uploads_and_leave_with_a_cull(env):
    import ctypes as C
    from city2ba_amd import _lib as L
    from city2ba_amd.solve import levenberg_marquardt
    name = "small grid"
    ba, _ = _make(name)
    nc, npt = ba.num_cameras(), ba.num_points()
    assert not ba.constant()[0].any() and not ba.constant()[1].any()
    cm, pm = _mask(ba, name)

    def in_force():
        c, p = ba.constant()
        return c.shape == (nc, 9) and p.shape == (npt,) and np.array_equal(c, _unpack(cm)) and np.array_equal(p, pm)

    ba.set_constant(_unpack(cm), pm)                                 # the bool [n_cam, 9] form
    assert in_force()
    ba.set_constant(cm, pm.astype(np.uint8))
    assert in_force()
    n_par, n_pts = C.c_int64(), C.c_int64()
    L.check(L.lib().c2b_problem_get_constant(ba._h, None, None, C.byref(n_par), C.byref(n_pts)))
    assert n_par.value == int(_unpack(cm).sum()) and n_pts.value == int(pm.sum())
    # refused arguments leave the masks in force
    bad = cm.copy()
    bad[3] |= 0x200
    for args in ((bad, pm), (cm, np.where(np.arange(npt) == 5, 2, pm).astype(np.uint8))):
        with pytest.raises(L.City2baError) as e:
            ba.set_constant(*args)
        assert e.value.status == L.ERR_INVALID_ARGUMENT == -1
        assert in_force()
    with pytest.raises(ValueError):
        ba.set_constant(cm[:-1], pm)
    with pytest.raises(ValueError):
        ba.set_constant(cm, pm[:-1])
    assert in_force()
    # the handle's other settings, an upload of the same counts, noise, steps and an LM run keep them
    ba.set_loss("huber", 1.0)
    ba.set_loss(None)
    ba.set_preconditioner("schur_jacobi")
    ba.set_preconditioner("block_jacobi")
    ba._upload(ba.cameras_bal(), True, ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
    assert in_force()
    hist = levenberg_marquardt(ba, 2, lam=1e-4)
    assert len(hist) == 2 and in_force()
    # one kind alone; both None clears
    ba.set_constant(cm, None)
    assert np.array_equal(ba.constant()[0], _unpack(cm)) and not ba.constant()[1].any()
    ba.set_constant(None, pm)
    assert not ba.constant()[0].any() and np.array_equal(ba.constant()[1], pm)
    ba.set_constant(None, None)
    assert not ba.constant()[0].any() and not ba.constant()[1].any()
    # a cull renumbers the entities: the masks go
    ba.set_constant(cm, pm)
    ba.cull()
    assert ba.num_cameras() < nc or ba.num_points() < npt
    c, p = ba.constant()
    assert c.shape == (ba.num_cameras(), 9) and not c.any() and not p.any()
    # an upload of another size drops them too
    ba.set_constant(np.full(ba.num_cameras(), FOCAL, dtype=np.uint16), None)
    assert ba.constant()[0][:, 6].all()
    b9, pts, rp, pi, uv = ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations()
    ba._upload(b9, True, np.concatenate([pts, pts[:1]]), rp, pi, uv)
    assert not ba.constant()[0].any()
    ba.close()


def test_rejected_lm_step_keeps_the_masks_and_the_constant_bits(env, monkeypatch):
    import city2ba_amd.solve as S
    name = "small grid culled"
    ba, _, cm, pm = _masked(name)
    ba.apply_step(None, None)
    orig = type(ba).solve_step

    def wrong_way(self, lam, max_iters=100, rel_tol=1e-6, out=None):
        dc, dp, info = orig(self, lam, max_iters, rel_tol, out)
        return -dc * 1e3, -dp * 1e3, info

    b0, x0 = ba.cameras_bal(), ba.points()
    monkeypatch.setattr(type(ba), "solve_step", wrong_way)
    hist = S.levenberg_marquardt(ba, 2, lam=1e-4)
    assert not any(h["accepted"] for h in hist)
    assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), x0)
    c, p = ba.constant()
    assert np.array_equal(c, _unpack(cm)) and np.array_equal(p, pm)
    ba.close()


# ---- 10. the LM loop with the gauge fixed ----------------------------------------------------------------------------------
def test_lm_with_the_gauge_fixed(env):
    from city2ba_amd.solve import ALL as S_ALL, levenberg_marquardt
    ba, _ = _make("small grid culled")
    ba.apply_step(None, None)
    nc = ba.num_cameras()
    cm = np.zeros(nc, dtype=np.uint16)
    cm[0], cm[1] = S_ALL, 1 << 3                                     # camera 0 and t0 of camera 1
    b0 = ba.cameras_bal()
    hist = levenberg_marquardt(ba, 5, lam=1e-4, constant=(cm, None))
    assert len(hist) == 5 and all(h["status"] in (0, 1) for h in hist), hist
    assert hist[-1]["error_after"] < hist[0]["error"], hist
    b1 = ba.cameras_bal()
    assert _bits(b1[0], b0[0]) and _bits(b1[1, 3], b0[1, 3])
    assert not _bits(b1[2:], b0[2:]) and not _bits(b1[1, :3], b0[1, :3])
    assert np.array_equal(ba.constant()[0], _unpack(cm)) and not ba.constant()[1].any()
    ba.close()
