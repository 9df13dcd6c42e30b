"""The direct solve of the reduced camera system in c2b_problem_solve_step (linear_solver = "cholesky") on the device:
the step against the longdouble direct solve of the reference system by the project's rule (16 x the largest deviation over seeded
perturbed reruns, floored at 1e-13 of the norm) and against test_gpu_coupled's criteria; against the PCG step converged to 1e-10 by
the gap-plus-both-bounds rule on the issue's grid, under Cauchy, under a mask, in a window child and under priors; exact zeros at
constant entries and empty cameras; a factor that fails; the cap, a shard; the default path bit for bit; the handle's state; memory;
the LM loop."""
import ctypes as C

import numpy as np
import pytest

import _denseref as DR
import _explicitref as X
import _schurref as R
import _solvecheck as SC
from test_gpu_coupled import _dome, _lin, _load
from test_gpu_schur_explicit import _issue_grid_on_the_device
from test_gpu_schur_step import EPS, _bits, _kappa, _make, _np, _ref, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
_cache = {}


def _norm(v):
    return float(np.linalg.norm(np.asarray(v).astype(np.float64)))


def _direct_reference(key, Q, lam, runs):
    if key not in _cache:
        _cache[key] = DR.direct_step_bound(Q, lam, runs=runs)
    return _cache[key]


def _true_rel_residual(ba, lam, dc):
    """|b - S dc| / |b| in longdouble from the device's own blocks and b, and what an f64 product and two folds may move it by:
    the product's bound (1e-13 of each row's absolute-value scale, tests/test_gpu_schur_explicit.py), relative to |b|"""
    nbr_ptr, nbr, Sd, So, b = ba.schur_complement(lam)
    y, scale = X.spmv(nbr_ptr, nbr, Sd.astype(R.LD), So.astype(R.LD), np.asarray(dc).astype(R.LD))
    bn = _norm(b)
    if bn == 0.0:
        return 0.0, 0.0
    r = b.astype(R.LD) - y
    return float(np.sqrt(np.sum(r * r))) / bn, 1e-13 * _norm(scale.astype(np.float64) + np.abs(b)) / bn


# ---- 1. the dome ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bal", "state"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_step_on_the_dome(env, lam, mode):
    ba = _load(_dome(mode))
    assert ba.linear_solver() == "pcg"
    ba.set_linear_solver("cholesky")
    assert ba.linear_solver() == "cholesky" and ba.schur() == "implicit"
    Q = _lin(ba)
    ref = _direct_reference(("dome", mode, lam), Q, lam, 8)
    dc, dp, info = ba.solve_step(lam)
    dc, dp = _np(dc), _np(dp)
    assert (info["iterations"], info["status"]) == (0, 0), info
    assert ba.schur() == "implicit" and ba.preconditioner_fallbacks() == 0           # `schur` is left alone
    ex, ed = _norm(dc - ref["x"].astype(np.float64)), _norm(dp - ref["dp"].astype(np.float64))
    print("DENSE step dome %s lam=%g: |dc - ref| / bound %.3g, |dp - ref| / bound %.3g (bounds %.3g, %.3g of the norms)"
          % (mode, lam, ex / ref["bound_x"], ed / ref["bound_dp"], ref["bound_x"] / _norm(ref["x"]), ref["bound_dp"] / _norm(ref["dp"])))
    assert ex <= ref["bound_x"] and ed <= ref["bound_dp"], (mode, lam, ex, ref["bound_x"], ed, ref["bound_dp"])
    # test_gpu_coupled's criteria against the dense solve
    ref64 = _lin(ba, np.float64)
    kappa = _kappa(ref64, lam)
    tol_res = max(1e-9, 1e3 * EPS * kappa)
    res, g = ref64.damped_residual(lam, dc, dp)
    wc, wp = ref64.schur_direct(lam)
    d, w = np.concatenate([dc.ravel(), dp.ravel()]), np.concatenate([wc.ravel(), wp.ravel()])
    print("DENSE step dome %s lam=%g: kappa %.3g, |res| / |g| %.3g, |d - w| / |w| %.3g, rel_residual %.3g"
          % (mode, lam, kappa, np.linalg.norm(res) / np.linalg.norm(g), np.linalg.norm(d - w) / np.linalg.norm(w), info["rel_residual"]))
    assert np.linalg.norm(res) <= tol_res * np.linalg.norm(g), (lam, kappa)
    assert np.linalg.norm(d - w) <= max(1e-8, kappa * tol_res) * np.linalg.norm(w), (lam, kappa)
    # rel_residual is the true one
    want, tol = _true_rel_residual(ba, lam, dc)
    assert abs(info["rel_residual"] - want) <= tol + 4 * EPS * want, (info["rel_residual"], want, tol)
    # sum_sq and the model decrease are the unchanged model pass's
    assert abs(info["sum_sq"] - float(SC.sum_sq(Q))) <= 1e-12 * float(SC.sum_sq(Q))
    assert abs(info["model_decrease"] - float(Q.model_decrease(dc, dp))) <= SC.model_tol(Q, dc, dp)
    # the dome's empty camera: S_cc = lam 1e-6 I, b = 0, an exact zero
    kc = np.diff(ba.row_ptr.astype(np.int64))
    assert (kc == 0).sum() == 1 and _bits(dc[kc == 0], np.zeros((1, 9)))
    # the same problem and arguments: the same bits
    dc2, dp2, info2 = ba.solve_step(lam, max_iters=3, rel_tol=0.5)                   # (validated, otherwise unused)
    assert _bits(_np(dc2), dc) and _bits(_np(dp2), dp) and info2 == info
    n, Np = 9 * ba.num_cameras(), DR.padded(9 * ba.num_cameras())
    assert ba.linear_solver_bytes() == ba.schur_bytes() + 8 * (Np * Np + 2 * Np) and Np == 768 and n == 729
    ba.close()


# ---- 2. the variants: the Cholesky step against the converged PCG step ----------------------------------------------------------
def _agrees_with_the_converged_pcg(ba, Q, lam, tag, kind="schur_jacobi", max_iters=3000, tol=1e-10, runs=3):
    """test_converged_step_agrees_with_the_implicit_path_and_the_dense_solve's rule between the two solvers: the device steps may
    differ by what the two references' solutions differ by plus each one's own bound.  The PCG runs on the stored blocks
    (schur = explicit), as its reference does.  Returns the Cholesky step."""
    rp = X.pcg(Q, lam, max_iters, tol, kind=kind, runs=runs)
    rd = DR.direct_step_bound(Q, lam, runs=runs)
    assert rp["status"] == 0, (tag, rp["iterations"])
    ba.set_schur("explicit")
    ba.set_preconditioner(kind)
    ba.set_linear_solver("pcg")
    dcp, dpp, ip = ba.solve_step(lam, max_iters=max_iters, rel_tol=tol)
    dcp, dpp = _np(dcp).copy(), _np(dpp).copy()
    ba.set_linear_solver("cholesky")
    dcc, dpc, ic = ba.solve_step(lam, max_iters=max_iters, rel_tol=tol)
    dcc, dpc = _np(dcc), _np(dpc)
    assert ip["status"] == 0 and ip["iterations"] > 0 and (ic["iterations"], ic["status"]) == (0, 0), (tag, ip, ic)
    assert ba.schur() == "explicit" and ba.preconditioner_fallbacks() == 0
    for key, rkey, bkey, gp, gc in (("x", "x", "bound_x", dcp, dcc), ("dp", "dp", "bound_dp", dpp, dpc)):
        gap = _norm(rp[key][-1] - rd[rkey])
        bound = gap + rp["bound"][key][-1] + rd[bkey]
        err = _norm(gp - gc)
        print("DENSE agreement %s %s: |pcg - cholesky| %.3g, bound %.3g (reference gap %.3g), %d PCG iterations, rel_residual %.3g vs %.3g"
              % (tag, key, err, bound, gap, ip["iterations"], ip["rel_residual"], ic["rel_residual"]))
        assert err <= bound, (tag, key, err, bound)
        assert _norm(gc - rd[rkey].astype(np.float64)) <= rd[bkey], (tag, key, "the direct reference")
    want, rtol = _true_rel_residual(ba, lam, dcc)
    assert abs(ic["rel_residual"] - want) <= rtol + 4 * EPS * want, (tag, ic["rel_residual"], want, rtol)
    return dcc, dpc, ic


def test_issue_grid(env):
    ba = _issue_grid_on_the_device()
    assert (ba.num_cameras(), ba.num_points()) == (240, 720)
    _agrees_with_the_converged_pcg(ba, _ref(ba, R.LD), 1e-2, "issue grid", runs=1)     # (240 cameras: a rerun's blocks take over a second)
    ba.close()


def test_dome_under_cauchy(env):
    P = _dome("bal")
    uv, _ = SC.dome_scaled_observations(P)
    ba = _load(P, uv)
    a = SC.cauchy_scale(ba.residual_jacobian()[0])
    ba.set_loss("cauchy", a)
    _agrees_with_the_converged_pcg(ba, _lin(ba, loss=("cauchy", a)), 1e-2, "dome cauchy")
    ba.close()


def test_dome_under_a_mask_gives_positive_zeros(env):
    P = _dome("bal")
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    ba.set_constant(cm, pm)
    dc, dp, _ = _agrees_with_the_converged_pcg(ba, _lin(ba, mask=(cm, pm)), 1e-2, "dome mask")
    m = SC.unpack(cm)
    assert m.sum() > 9 and _bits(dc[m], np.zeros(int(m.sum())))                      # +0.0 by bits, not merely == 0
    assert _bits(dp[np.asarray(pm, dtype=bool)], np.zeros((int(np.sum(pm)), 3)))
    ba.close()


def test_window_child_carries_the_setting(env):
    g, _ = _make("small grid culled")
    g.set_linear_solver("cholesky")
    w = g.window(np.arange(5), halo=True)
    assert w.linear_solver() == "cholesky"
    cmb, pm = w.constant()
    assert cmb.all(axis=1).any() and not cmb.all()                                   # the rim is held, the seeds are free
    cm = (cmb.astype(np.uint16) << np.arange(9, dtype=np.uint16)).sum(axis=1).astype(np.uint16)
    dc, dp, _ = _agrees_with_the_converged_pcg(w, _lin(w, mask=(cm, pm)), 1e-2, "window child")
    assert _bits(dc[cmb], np.zeros(int(cmb.sum())))
    for carry, want in ((False, "pcg"), (True, "cholesky")):                         # without carry: a new problem's
        child = g.subset(np.arange(4), np.arange(g.num_points()), carry=carry)
        assert child.linear_solver() == want
        child.close()
    w.close()
    g.close()


def test_priors_on_the_small_culled_grid(env):
    from test_gpu_priors import _stacked, _with_priors
    ba, bal, kw = _with_priors("small grid culled")
    _agrees_with_the_converged_pcg(ba, _stacked(ba, kw, dtype=R.LD), 1e-2, "priors", kind="block_jacobi", max_iters=400)
    ba.close()


# ---- 3. failure and refusals ------------------------------------------------------------------------------------------------------
def test_a_factor_that_fails_is_status_2_and_a_zero_step(env):
    """a camera with a non-finite intrinsic: its block of S is not finite, its first pivot fails, the step is the step without a factor"""
    import city2ba_amd as c2b
    from _problems import random_problem
    P = random_problem(12, 120, 8, seed=5, noise=1e-3)
    bal9 = P["bal9"].copy()
    bal9[3, 6] = np.nan
    ba = c2b.BAProblem.from_bal(bal9, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    ba.set_linear_solver("cholesky")
    dc, dp, info = ba.solve_step(1e-2)
    assert info["status"] == 2 and info["iterations"] == 0 and info["rel_residual"] == 1.0 and info["model_decrease"] == 0.0, info
    assert not _np(dc).any() and not _np(dp).any()
    ba.set_linear_solver("pcg")                                                      # the handle stays usable
    _, _, info = ba.solve_step(1e-2)
    assert info["status"] == 2
    ba.close()


def test_the_cap_and_a_shard_are_refused(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    lib = L.lib()
    n = C.c_int64(-7)
    nc = L.DENSE_MAX_CAMERAS + 1                                                     # one observation, 4097 cameras
    bal9 = np.zeros((nc, 9))
    bal9[:, 6] = 1.0
    row_ptr = np.concatenate([[0], np.ones(nc)]).astype(np.uint64)
    big = c2b.BAProblem.from_bal(bal9, np.array([[0.0, 0.0, -5.0]]), row_ptr, np.zeros(1, dtype=np.uint64), np.zeros((1, 2)), device=0)
    big.set_linear_solver("cholesky")
    assert lib.c2b_problem_linear_solver_bytes(big._h, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"C2B_DENSE_MAX_CAMERAS" in lib.c2b_last_error()
    with pytest.raises(L.City2baError, match="C2B_DENSE_MAX_CAMERAS"):
        big.solve_step(1e-2)
    big.set_linear_solver("pcg")                                                     # usable under pcg
    _, _, info = big.solve_step(1e-2)
    assert info["status"] == 0 and n.value == -7
    big.close()
    ba, _ = _make("random bal")
    with pytest.raises(ValueError):
        ba.set_linear_solver("dense")
    with pytest.raises(L.City2baError):
        ba.set_linear_solver(2)
    with pytest.raises(ValueError):
        ba.set_schur("dense")                                                        # still no third value of set_schur
    assert ba.linear_solver() == "pcg"
    ba.set_linear_solver("cholesky")
    L.check(lib.c2b_problem_set_shard(ba._h, 0, 2 * ba.num_cameras(), 0))
    assert lib.c2b_problem_linear_solver_bytes(ba._h, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"shard" in lib.c2b_last_error() and n.value == -7
    with pytest.raises(L.City2baError, match="shard"):
        ba.solve_step(1e-2)
    ba.close()
    empty = c2b.BAProblem(0)
    assert lib.c2b_problem_linear_solver_bytes(empty._h, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"nothing uploaded" in lib.c2b_last_error()
    empty.set_linear_solver("cholesky")                                              # the handle's, with or without an upload
    assert empty.linear_solver() == "cholesky"
    empty.close()


# ---- 4. the default path; the handle's state; memory -------------------------------------------------------------------------------
@pytest.mark.parametrize("schur", ["implicit", "explicit"])
def test_default_path_is_untouched(env, schur):
    lam = 1e-4
    plain, _ = _make("small grid culled")
    plain.set_schur(schur)
    want = plain.solve_step(lam, max_iters=7, rel_tol=0.0)
    want = [_np(want[0]).copy(), _np(want[1]).copy(), want[2]]
    assert plain.linear_solver() == "pcg"
    plain.close()
    ba, _ = _make("small grid culled")
    ba.set_schur(schur)
    ba.set_linear_solver("cholesky")
    a = ba.solve_step(lam, max_iters=7, rel_tol=0.0)
    assert a[2]["iterations"] == 0 and not _bits(_np(a[0]), want[0])
    ba.set_linear_solver("pcg")
    got = ba.solve_step(lam, max_iters=7, rel_tol=0.0)
    assert _bits(_np(got[0]), want[0]) and _bits(_np(got[1]), want[1]) and got[2] == want[2]       # a handle that never left pcg
    ba.close()


def test_setting_survives_upload_and_cull(env):
    from test_gpu_schur_step import _grid
    g = _grid(cull=False)
    g.set_linear_solver("cholesky")
    g.cull()
    assert g.linear_solver() == "cholesky"
    bal9, pts, rp, pi, uv = g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), g.observations()
    uv = uv + np.random.default_rng(3).normal(scale=1e-2, size=uv.shape)
    g._upload(bal9, True, pts, rp, pi, uv)
    assert g.linear_solver() == "cholesky"
    _, _, info = g.solve_step(1e-2, max_iters=3, rel_tol=0.0)
    assert (info["iterations"], info["status"]) == (0, 0)
    g.close()


def test_fifty_rounds_leave_the_free_memory_where_it_was(env):
    """in the manner of tests/test_gpu_schur_explicit.py: a warm-up round, then 50 rounds of set / solve / drop (the upload drops the
    rows, the pattern and the solve buffers with the dense image)"""
    torch = env["torch"]
    ba = _load(_dome("bal"))
    bal9, pts, rp, pi, uv = ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations()

    def round_():
        ba.set_linear_solver("cholesky")
        ba.solve_step(1e-2)
        ba.set_linear_solver("pcg")
        ba._upload(bal9, True, pts, rp, pi, uv)
    round_()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        round_()
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info(0)[0]
    print("free device memory dropped by %d bytes over 50 cholesky set / solve / drop rounds" % drop)
    assert drop <= 0
    ba.close()


# ---- 5. the LM loop ----------------------------------------------------------------------------------------------------------------
def test_lm_loop_reaches_the_pcg_loop_s_error(env):
    """test_gpu_schur_explicit.test_lm_loop_reaches_the_implicit_loop_s_error's allowance, between the two solvers: the PCG loop solves
    every step to rel_tol 1e-10; the converged PCG reference and the direct reference of the first linearisation differ by a relative
    eta in the step (their gap plus each one's bound, floored at 1e-13), and the final errors are held to 16 x iterations x 2 eta,
    relative.  The direct loop runs 0 PCG iterations in every row."""
    from city2ba_amd.solve import levenberg_marquardt_device
    its, lam, tol = 6, 1e-4, 1e-10
    out = {}
    for solver in ("pcg", "cholesky"):
        ba, _ = _make("small grid culled")
        if solver == "pcg":
            Q = _ref(ba, R.LD)
            rp = X.pcg(Q, lam, 3000, tol, kind="schur_jacobi", runs=1)
            rd = DR.direct_step_bound(Q, lam, runs=1)
            assert rp["status"] == 0
            gap = _norm(rp["x"][-1] - rd["x"]) + rp["bound"]["x"][-1] + rd["bound_x"]
            eta = max(gap / _norm(rd["x"]), 1e-13)
        hist, summary = levenberg_marquardt_device(ba, its, lam=lam, max_iters=3000, rel_tol=tol, preconditioner="schur_jacobi", schur="explicit",
                                                   linear_solver=solver)
        assert ba.linear_solver() == solver and all(h["status"] == 0 for h in hist), [(h["status"], h["pcg_iterations"]) for h in hist]
        out[solver] = (hist[-1]["error_after"], [h["accepted"] for h in hist], [h["pcg_iterations"] for h in hist])
        ba.close()
    (ep, ap, npcg), (ec, ac, nchol) = out["pcg"], out["cholesky"]
    bound = 16 * its * 2 * eta
    print("DENSE lm: final error %.15g (pcg, %d PCG iterations) %.15g (cholesky); |diff| / error %.3g, bound %.3g"
          % (ep, sum(npcg), ec, abs(ep - ec) / ep, bound))
    assert nchol == [0] * len(nchol) and min(npcg) > 0
    assert ap == ac and abs(ep - ec) <= bound * ep, (ep, ec, bound, ap, ac)
