"""The damped Gauss-Newton step on the device: the Schur complement passes (c2b_schur_points_rows,
c2b_schur_cameras_rows), c2b_problem_solve_step / c2b_problem_apply_step (BAProblem.solve_step / apply_step) and
city2ba_amd.solve.levenberg_marquardt, against the host reference of tests/_schurref.py built from the device's own
Jacobian (BAProblem.residual_jacobian)."""
import ctypes as C

import numpy as np
import pytest

import _schurref as R
import oracle as O
from _problems import mixed_k2_cameras, random_problem

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0
    return dict(torch=torch, D=D, dev=torch.device("cuda", 0))


def _np(t):
    return t.cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _cam_of(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def _ref(ba, dtype=np.float64):
    r, Jc, Jp = ba.residual_jacobian()
    return R.Problem(r, Jc, Jp, _cam_of(ba.row_ptr), ba.pt_idx.astype(np.int64), ba.num_cameras(), ba.num_points(), dtype=dtype)


def _grid(cull):
    from city2ba_amd import synthetic as S
    g = S.synthetic_grid(3, 20, 3, 5.0, 1.0, 1.0, 1.0, 10.0, False, cull=False)
    if cull:
        g.cull()
    return g


def _problems():
    """(name, factory) of the problems the operator and solve tests run on; each factory returns (ba, bal_mode)"""
    import city2ba_amd as c2b
    from city2ba_amd import noise as N

    def rand_bal():
        P = random_problem(30, 300, 8, seed=11, noise=1e-3, empty_every=7)
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0), True

    def rand_state():
        ba, _ = rand_bal()
        N.add_drift(ba, 0.05, 0.01, 0.01, [1.0, 0.5, 0.0], seed=4)
        return ba, False

    def k2():
        P = random_problem(25, 250, 10, seed=23)
        cams = mixed_k2_cameras(P["cams15"], "signs", seed=5)
        uv = O.project_observations(cams, P["pts"], P["row_ptr"], P["pt_idx"])
        uv = uv + np.random.default_rng(8).normal(scale=1e-3, size=uv.shape)
        return c2b.BAProblem.from_visibility(cams, P["pts"], P["row_ptr"], P["pt_idx"], uv, device=0), False

    def grid(cull):
        def make():
            g = _grid(cull)
            uv = g.observations() + np.random.default_rng(3).normal(scale=1e-2, size=(g.num_observations(), 2))
            ba = c2b.BAProblem.from_bal(g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), uv)
            g.close()
            return ba, True
        return make

    def small_grid(cull):                                        # few enough unknowns for a dense solve on the host
        def make():
            from city2ba_amd import synthetic as S
            g = S.synthetic_grid(2, 5, 2, 5.0, 1.0, 1.0, 1.0, 10.0, False, cull=cull)
            uv = g.observations() + np.random.default_rng(4).normal(scale=1e-2, size=(g.num_observations(), 2))
            ba = c2b.BAProblem.from_bal(g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), uv)
            g.close()
            return ba, True
        return make

    def mid_grid():                                              # n_cam = 2879: several k_pcg_update workgroups, a
        from city2ba_amd import synthetic as S                   # partly empty last wave, > 256 p.q and model partials
        g = S.synthetic_grid(10, 10, 8, 20.0, 1.0, 1.0, 1.0, 10.0, False, cull=False)
        nc = g.num_cameras() - 1
        rp = g.row_ptr[:nc + 1].copy()
        no = int(rp[-1])
        uv = g.observations()[:no] + np.random.default_rng(6).normal(scale=1e-3, size=(no, 2))
        ba = c2b.BAProblem.from_bal(g.cameras_bal()[:nc], g.points(), rp, g.pt_idx[:no].copy(), uv)
        g.close()
        return ba, True

    return [("random bal", rand_bal), ("random state", rand_state), ("mixed k2", k2), ("grid culled", grid(True)),
            ("grid", grid(False)), ("small grid culled", small_grid(True)), ("small grid", small_grid(False)),
            ("mid grid", mid_grid)]


PROBLEMS = ["random bal", "random state", "mixed k2", "grid culled", "grid", "mid grid"]




def _make(name):
    return dict(_problems())[name]()


def _level0(env, ba, bal):
    """the problem's Level-0 inputs: camblk of its mode, pts4, rows, point rows, pt_idx, uv"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ex = ba.export_device()
    camblk = D.cameras_prepare_bal(torch.from_numpy(ba.cameras_bal()).to(dev)) if bal else D.cameras_prepare_state(ex["cam15"])
    rows = D.Rows(ex["row_ptr"], ex["n_obs"])
    prows = D.PointRows(rows, ex["pt_idx"], ba.num_points())
    return camblk, ex["pts4"], rows, prows, ex["pt_idx"], ex["uv"]


# ---- 1. operator exactness --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_operator_rhs_and_back_substitution(env, name):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ba, bal = _make(name)
    ref = _ref(ba, R.LD)
    nc, npt = ba.num_cameras(), ba.num_points()
    U, gc, V, gp, _ = ba.normal_equations()
    camblk, pts4, rows, prows, pi, uv = _level0(env, ba, bal)
    f64 = dict(dtype=torch.float64, device=dev)
    t, y = torch.empty((npt, 3), **f64), torch.empty((nc, 9), **f64)
    rng = np.random.default_rng(7)
    for lam in (1e-2, 1.0):
        x = rng.normal(size=(nc, 9))
        xt = torch.from_numpy(x).to(dev)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, xt, None, t)
        D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, lam, xt, t, y)
        want, scale = ref.S_times(lam, x)
        err = np.linalg.norm((_np(y).astype(R.LD) - want).astype(np.float64))
        assert err <= 1e-12 * np.linalg.norm(scale.astype(np.float64)), (name, lam, err)
        # b = -gc - cameras(NULL, points(NULL, gp))
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, None, gp, t)
        D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, lam, None, t, y)
        b = -_np(gc) - _np(y)
        want, scale = ref.rhs(lam)
        err = np.linalg.norm((b.astype(R.LD) - want).astype(np.float64))
        assert err <= 1e-12 * np.linalg.norm(scale.astype(np.float64)), (name, "b", lam, err)
        # dp = -points(dc, gp)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, xt, gp, t)
        want, scale = ref.back_substitute(lam, x)
        err = np.linalg.norm((-_np(t).astype(R.LD) - want).astype(np.float64))
        assert err <= 1e-12 * np.linalg.norm(scale.astype(np.float64)), (name, "dp", lam, err)
    ba.close()


# ---- 2. solve accuracy --------------------------------------------------------------------------------------------
def _kappa(ref, lam):
    """condition number of the Jacobi-scaled damped system: how far any f64 solve can be trusted"""
    _, H, _ = ref.dense_H()
    i = np.arange(len(H))
    H[i, i] = R.damp_diag(H[i, i], lam)
    s = 1.0 / np.sqrt(np.diag(H))
    return np.linalg.cond(H * s[:, None] * s[None, :])


@pytest.mark.parametrize("name", ["random bal", "random state", "mixed k2", "small grid culled", "small grid"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_solve_accuracy(env, name, lam):
    ba, _ = _make(name)
    ref = _ref(ba)
    dc, dp, info = ba.solve_step(lam, max_iters=5000, rel_tol=1e-12)
    dc, dp = _np(dc), _np(dp)
    assert info["status"] == 0 and info["rel_residual"] <= 1e-12, info
    kappa = _kappa(ref, lam)
    tol_res = max(1e-9, 1e3 * EPS * kappa)
    res, g = ref.damped_residual(lam, dc, dp)
    assert np.linalg.norm(res) <= tol_res * np.linalg.norm(g), (name, lam, kappa, np.linalg.norm(res) / np.linalg.norm(g))
    wc, wp = ref.direct(lam)
    d, w = np.concatenate([dc.ravel(), dp.ravel()]), np.concatenate([wc.ravel(), wp.ravel()])
    assert np.linalg.norm(d - w) <= max(1e-8, kappa * tol_res) * np.linalg.norm(w), (name, lam, kappa)
    md = float(R.Problem(ref.r, ref.Jc, ref.Jp, ref.cam, ref.pt, ref.n_cam, ref.n_pts, dtype=R.LD).model_decrease(dc, dp))
    assert md > 0 and abs(info["model_decrease"] - md) <= 1e-10 * md, (info["model_decrease"], md)
    e2 = ba.total_reprojection_error(2.0) ** 2
    assert abs(info["sum_sq"] - e2) <= 1e-12 * e2
    ba.close()


# ---- 3. a joint step ------------------------------------------------------------------------------------------------
def _perturbed_grid(seed):
    import city2ba_amd as c2b
    g = _grid(cull=True)
    bal9, pts, rp, pi = g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy()
    uv = g.project()                                                  # exact observations
    g.close()
    rng = np.random.default_rng(seed)
    b9 = bal9.copy()
    b9[:, :6] += rng.normal(scale=1e-4, size=(len(b9), 6))
    X = pts + rng.normal(scale=1e-3, size=pts.shape)
    return c2b.BAProblem.from_bal(b9, X, rp, pi, uv, device=0)


def test_joint_step_and_levenberg_marquardt(env):
    from city2ba_amd.solve import levenberg_marquardt
    ba = _perturbed_grid(12)
    e0 = ba.total_reprojection_error(2.0)
    dc, dp, info = ba.solve_step(1e-8, max_iters=1000, rel_tol=1e-10)
    ba.apply_step(dc, dp)
    e1 = ba.total_reprojection_error(2.0)
    assert e0 > 1e-6 and e1 <= e0 / 100.0, (e0, e1, info)
    ba.close()
    ba = _perturbed_grid(13)
    e0 = ba.total_reprojection_error(2.0)
    hist = levenberg_marquardt(ba, 10)
    e = ba.total_reprojection_error(2.0)
    assert len(hist) == 10 and hist[0]["accepted"]
    assert e <= 1e-6 * e0, (e0, e, hist)
    ba.close()


# ---- 4. determinism and edges ----------------------------------------------------------------------------------------
def test_determinism_zeros_max_iters_and_zero_gradient(env):
    import city2ba_amd as c2b
    torch = env["torch"]
    ba, _ = _make("grid")
    a = ba.solve_step(1e-3, max_iters=40, rel_tol=1e-9)
    out = (torch.full_like(a[0], float("nan")), torch.full_like(a[1], float("nan")))
    b = ba.solve_step(1e-3, max_iters=40, rel_tol=1e-9, out=out)
    assert b[0] is out[0] and b[1] is out[1]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    for name in ("grid", "random bal"):                            # empty cameras; unobserved points
        bz, _ = _make(name)
        dc, dp, _ = bz.solve_step(1e-3, max_iters=40, rel_tol=1e-9)
        dc, dp = _np(dc), _np(dp)
        kc = np.diff(bz.row_ptr.astype(np.int64))
        kp = np.bincount(bz.pt_idx.astype(np.int64), minlength=bz.num_points())
        assert (kc == 0).any() and (name == "grid" or (kp == 0).any())
        assert not dc[kc == 0].any() and not dp[kp == 0].any()
        assert dc[kc > 0].any(axis=1).all()
        bz.close()
    _, _, info = ba.solve_step(1e-3, max_iters=3, rel_tol=1e-14)
    assert info["status"] == 1 and info["iterations"] == 3 and 0 < info["rel_residual"] < np.inf
    _, _, info = ba.solve_step(1e-3, max_iters=0, rel_tol=1e-6)
    assert info["status"] == 1 and info["iterations"] == 0 and info["rel_residual"] == 1.0
    ba.close()
    # a zero gradient: observe exactly what the Jacobian pass projects (r = projected - 0 with zero observations), so r = 0
    P = random_problem(20, 200, 8, seed=3)
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], np.zeros_like(P["uv"]), device=0)
    proj = ba.residual_jacobian()[0].copy()
    ba._upload(P["bal9"], True, P["pts"], P["row_ptr"], P["pt_idx"], proj)
    assert not ba.residual_jacobian()[0].any()
    dc, dp, info = ba.solve_step(1e-3)
    assert info["iterations"] == 0 and info["status"] == 0 and info["rel_residual"] == 0.0 and info["model_decrease"] == 0.0
    assert not _np(dc).any() and not _np(dp).any()
    ba.close()


# ---- 5. apply_step ------------------------------------------------------------------------------------------------------
def test_apply_step_semantics(env):
    import city2ba_amd as c2b
    from city2ba_amd import noise as N
    torch, dev = env["torch"], env["dev"]
    P = random_problem(30, 300, 8, seed=19, noise=1e-3, empty_every=7)
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    dc, dp, _ = ba.solve_step(1e-3)
    b0, x0 = ba.cameras_bal(), ba.points()
    ba.apply_step(dc, dp)
    b1, x1 = ba.cameras_bal(), ba.points()
    assert _bits(b1, b0 + _np(dc)) and _bits(x1, x0 + _np(dp))
    fresh = c2b.BAProblem.from_bal(b1, x1, P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    assert all(_bits(a, b) for a, b in zip(ba.residual_jacobian(), fresh.residual_jacobian()))
    assert ba.total_reprojection_error(2.0) == fresh.total_reprojection_error(2.0)
    fresh.close()
    # state mode: the columns refer to to_vec(cam15)
    N.add_drift(ba, 0.05, 0.01, 0.01, [1.0, 0.5, 0.0], seed=4)
    vec = ba.cameras_bal()
    dc, dp, _ = ba.solve_step(1e-3)
    ba.apply_step(dc, None)
    assert _bits(ba.cameras_bal(), vec + _np(dc))
    want = O.camera_from_bal(vec + _np(dc)) if hasattr(O, "camera_from_bal") else None
    if want is not None:
        assert np.allclose(ba.cameras(), want, rtol=0, atol=1e-12)
    # apply_step(None, None) takes a state-mode problem to bal mode: its Jacobian is then that of from_bal(to_vec)
    N.add_drift(ba, 0.05, 0.01, 0.01, [0.0, 0.5, 1.0], seed=5)
    vec, pts = ba.cameras_bal(), ba.points()
    ba.apply_step(None, None)
    assert _bits(ba.cameras_bal(), vec) and _bits(ba.points(), pts)
    fresh = c2b.BAProblem.from_bal(vec, pts, P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    assert all(_bits(a, b) for a, b in zip(ba.residual_jacobian(), fresh.residual_jacobian()))
    fresh.close()
    ba.close()


def test_solver_buffers_follow_cull_and_upload(env):
    import city2ba_amd as c2b
    g = _grid(cull=False)
    uv = g.observations() + np.random.default_rng(5).normal(scale=1e-2, size=(g.num_observations(), 2))
    ba = c2b.BAProblem.from_bal(g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), uv)
    g.close()

    def fresh_equal(ba):
        got = ba.solve_step(1e-2, max_iters=30)
        f = c2b.BAProblem.from_bal(ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
        want = f.solve_step(1e-2, max_iters=30)
        f.close()
        assert _bits(_np(got[0]), _np(want[0])) and _bits(_np(got[1]), _np(want[1])) and got[2] == want[2]

    fresh_equal(ba)
    n0 = ba.num_observations()
    ba.cull()
    assert ba.num_observations() < n0
    fresh_equal(ba)
    P = random_problem(40, 500, 10, seed=3, noise=1e-3)
    ba._upload(P["bal9"], True, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    fresh_equal(ba)
    ba.close()


def test_rejected_lm_step_restores_the_problem_bit_for_bit(env, monkeypatch):
    ba = _perturbed_grid(21)
    ba.apply_step(None, None)
    # force a rejection: a model decrease the error cannot follow (sign-flipped step)
    import city2ba_amd.solve as S
    orig = type(ba).solve_step

    def wrong_way(self, lam, max_iters=100, rel_tol=1e-6, out=None):
        dc, dp, info = orig(self, lam, max_iters, rel_tol, out)
        return -dc * 1e3, -dp * 1e3, info

    b1, x1 = ba.cameras_bal(), ba.points()
    monkeypatch.setattr(type(ba), "solve_step", wrong_way)
    hist = S.levenberg_marquardt(ba, 2, lam=1e-4)
    assert not any(h["accepted"] for h in hist) and hist[1]["lam"] > hist[0]["lam"]
    assert _bits(ba.cameras_bal(), b1) and _bits(ba.points(), x1)
    ba.close()


# ---- 6. bad arguments ------------------------------------------------------------------------------------------------
def test_bad_arguments(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    torch, dev = env["torch"], env["dev"]
    lib = L.lib()
    P = random_problem(20, 300, 10, seed=1, noise=1e-3)
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    nc, npt = ba.num_cameras(), ba.num_points()
    dc = torch.full((nc, 9), float("nan"), dtype=torch.float64, device=dev)
    dp = torch.full((npt, 3), float("nan"), dtype=torch.float64, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    info = L.StepInfo()
    for lam, it, tol, a, b in ((0.0, 10, 1e-6, p(dc), p(dp)), (-1.0, 10, 1e-6, p(dc), p(dp)), (float("nan"), 10, 1e-6, p(dc), p(dp)),
                               (float("inf"), 10, 1e-6, p(dc), p(dp)), (1e-3, -1, 1e-6, p(dc), p(dp)),
                               (1e-3, 10, float("nan"), p(dc), p(dp)), (1e-3, 10, -1.0, p(dc), p(dp)),
                               (1e-3, 10, 1e-6, None, p(dp)), (1e-3, 10, 1e-6, p(dc), None), (1e-3, 10, 1e-6, p(dc, 4), p(dp))):
        assert lib.c2b_problem_solve_step(ba._h, lam, it, tol, a, b, C.byref(info)) == L.ERR_INVALID_ARGUMENT, (lam, it, tol)
    assert lib.c2b_problem_solve_step(None, 1e-3, 10, 1e-6, p(dc), p(dp), C.byref(info)) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_problem_apply_step(ba._h, p(dc, 4), None) == L.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool(torch.isnan(dc).all()) and bool(torch.isnan(dp).all())
    for lam in (0.0, float("nan")):
        with pytest.raises(L.City2baError):
            ba.solve_step(lam)
    with pytest.raises(L.City2baError):
        ba.solve_step(1e-3, max_iters=-1)
    for out in ((dc[:-1], dp), (dc.float(), dp), (dc, dp.cpu()), (dc.t().contiguous().t(), dp) if nc != 9 else (dc[:, :8], dp),
                (dc,)):
        with pytest.raises((ValueError, L.City2baError)):
            ba.solve_step(1e-3, out=out)
    with pytest.raises(ValueError):
        ba.apply_step(dc[:-1], None)
    assert bool(torch.isnan(dc).all()) and bool(torch.isnan(dp).all())
    # a shard is refused
    L.check(lib.c2b_problem_set_shard(ba._h, 0, nc, 0))
    assert lib.c2b_problem_solve_step(ba._h, 1e-3, 10, 1e-6, p(dc), p(dp), C.byref(info)) == L.ERR_INVALID_ARGUMENT
    assert b"shard" in lib.c2b_last_error()
    # Level 0: lambda and NULL outputs
    assert lib.c2b_schur_points_rows(None, None, 5, None, None, None, None, None, 1.0, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_schur_cameras_rows(None, None, None, 3, None, None, 0, None, 1.0, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_schur_points_rows(None, None, 0, None, None, None, None, None, 0.0, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_schur_cameras_rows(None, None, None, 0, None, None, 0, None, float("nan"), None, None, None, None) == L.ERR_INVALID_ARGUMENT
    ba.close()


# ---- 7. full size ---------------------------------------------------------------------------------------------------
def test_blocks_32_sample(env):
    from city2ba_amd import noise as N
    from city2ba_amd import synthetic as S
    torch = env["torch"]
    ba = S.synthetic_grid(10, 10, 32, 20.0, 1.0, 1.0, 1.0, 10.0, cull=False, mirror=False)     # bench.py's instance
    assert ba.num_observations() == 1_225_066
    N.add_noise(ba, 0.0, 0.0, 0.0, 1e-3, seed=20243)
    a5 = ba.solve_step(1e-4, max_iters=5, rel_tol=0.0)
    a = ba.solve_step(1e-4, max_iters=25, rel_tol=0.0)
    b = ba.solve_step(1e-4, max_iters=25, rel_tol=0.0)
    assert a[2]["iterations"] == 25 and a[2]["status"] == 1, a[2]
    assert a[2]["rel_residual"] < a5[2]["rel_residual"] < 1.0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[2]["model_decrease"] > 0 and torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    ba.close()
