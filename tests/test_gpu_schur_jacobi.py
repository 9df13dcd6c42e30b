"""The Schur-Jacobi preconditioner on the device (k_schur_jacobi, k_schur_factor_blocks; BAProblem.set_preconditioner,
device.schur_jacobi_blocks, levenberg_marquardt(preconditioner=...)) against the longdouble reference of
tests/_precondref.py built from the device's own Jacobian: the blocks M, every PCG iterate, the stopping iteration, the
converged step, the untouched default path, determinism, persistence, the fallback count and the LM loop.
Worst |err| / bound seen on the MI355X (printed as SJREF lines): see DESIGN 4.4."""
import numpy as np
import pytest

import _precondref as PR
import _robustref as B
import _schurref as R
import _solvecheck as SC
from test_gpu_schur_pcg import KS, _crossing_tols, _model_tol, _over, _sparse_problem, _sum_sq
from test_gpu_schur_step import _bits, _cam_of, _level0, _make, _np, _ref, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
FIVE = ["random bal", "random state", "mixed k2", "small grid culled", "mid grid"]
RANDOM = ["random bal", "random state", "mixed k2"]              # every point seen by one camera: S is block-diagonal


def _sj(name):
    ba, bal = _make(name)
    ba.set_preconditioner("schur_jacobi")
    return ba, bal


def _device_blocks(env, ba, bal, lam, loss=None):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    camblk, pts4, rows, prows, pi, uv = _level0(env, ba, bal)
    f64 = dict(dtype=torch.float64, device=dev)
    nc, npt = ba.num_cameras(), ba.num_points()
    U, gc = torch.empty((nc, 9, 9), **f64), torch.empty((nc, 9), **f64)
    V, gp = torch.empty((npt, 3, 3), **f64), torch.empty((npt, 3), **f64)
    D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U, gc, loss=loss)
    D.normal_points_rows(camblk, pts4, prows, uv, V, gp, loss=loss)
    M = torch.full((nc, 9, 9), float("nan"), **f64)
    D.schur_jacobi_blocks(camblk, pts4, rows, pi, uv, U, V, lam, M, loss=loss)
    torch.cuda.synchronize()
    return _np(M)


_check_blocks = SC.check_blocks


# ---- 1. the blocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIVE)
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_blocks_follow_the_longdouble_definition(env, name, lam):
    ba, bal = _make(name)
    _check_blocks(_device_blocks(env, ba, bal, lam), _ref(ba, R.LD), lam, name, runs=3 if name == "mid grid" else 8)
    ba.close()


@pytest.mark.parametrize("name", ["random bal", "small grid culled"])
def test_weighted_blocks_follow_the_reweighted_reference(env, name):
    ba, bal = _make(name)
    r, Jc, Jp = ba.residual_jacobian()
    a = 3.0 * float(np.sqrt(np.mean(r * r)))
    P = B.problem("cauchy", a, r, Jc, Jp, _cam_of(ba.row_ptr), ba.pt_idx.astype(np.int64), ba.num_cameras(), ba.num_points(), dtype=R.LD)
    lam = 1e-3
    M = _device_blocks(env, ba, bal, lam, loss=("cauchy", a))
    _check_blocks(M, P, lam, name + " cauchy", runs=8)
    assert not _bits(M, _device_blocks(env, ba, bal, lam))       # the weights did something
    ba.close()


# ---- 2. every iterate -------------------------------------------------------------------------------------------------
def _check_iterates(ba, lam, ks, runs=8, tag="", kind="schur_jacobi"):
    """test_gpu_schur_pcg._check_iterates with the reference's preconditioner as a parameter: solve_step(lam, k, 0)
    against _precondref.pcg for every k in ks (x, dp, recurrence residual, energy, model decrease, sum_sq)"""
    P = _ref(ba, R.LD)
    ref = PR.pcg(P, lam, max(ks), 0.0, kind=kind, runs=runs)
    return SC.check_iterates(ba, P, ref, lam, ks, tag=tag, label="SJREF iterates")


@pytest.mark.parametrize("name", RANDOM)
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_block_diagonal_problems_converge_in_one_iteration(env, name, lam):
    ba, _ = _sj(name)
    P = _ref(ba, R.LD)
    assert len(np.unique(P.pt)) == len(P.pt)                     # every point seen once: S is block-diagonal, M is S
    ref = _check_iterates(ba, lam, (0, 1), tag=name)
    # the largest |r_1| / |b| the reference's bound allows -- but never looser than sqrt(eps): M = S makes the iteration
    # a direct solve whose residual is rounding alone, and where the points are seen once at small lam the reference's
    # perturbed reruns allow more than 1, which would stop the solve before its first iteration
    tol = min(float(ref["rel"][1]) + ref["bound"]["rel"][1], float(np.sqrt(R.EPS)))
    _, _, info = ba.solve_step(lam, max_iters=50, rel_tol=tol)
    assert info["status"] == 0 and info["iterations"] == 1 and info["rel_residual"] <= tol, (name, lam, tol, info)
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_small_grid_iterates_follow_the_reference(env, lam):
    ba, _ = _sj("small grid culled")
    _check_iterates(ba, lam, KS, tag="small grid culled")
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


# ---- 3. stopping; mid size ----------------------------------------------------------------------------------------------
def test_stopping_iteration_is_exact_on_the_small_grid(env):
    ba, _ = _sj("small grid culled")
    lam = 1e-4
    ref = PR.pcg(_ref(ba, R.LD), lam, max(KS), 0.0)
    tols = _crossing_tols(ref, 4)
    assert len(tols) >= 2, ref["rel"]
    for K, tol in tols:
        _, _, info = ba.solve_step(lam, max_iters=200, rel_tol=tol)
        assert info["status"] == 0 and info["iterations"] == K and info["rel_residual"] <= tol, (K, tol, info)
    ba.close()


def test_mid_size_iterates_stopping_and_fallbacks(env):
    ba, _ = _sj("mid grid")
    for lam in (1e-4, 1.0):
        ba.solve_step(lam, max_iters=1)
        assert ba.preconditioner_fallbacks() == 0, lam
    lam = 1e-4
    ref = _check_iterates(ba, lam, (0, 1, 3), runs=3, tag="mid grid")
    tols = _crossing_tols(ref, 2)
    assert tols, ref["rel"]
    for K, tol in tols:
        _, _, info = ba.solve_step(lam, max_iters=50, rel_tol=tol)
        assert info["status"] == 0 and info["iterations"] == K, (K, tol, info)
    ba.close()


# ---- 4. the same step; the default path; determinism; persistence ----------------------------------------------------------
def test_converged_step_agrees_with_block_jacobi(env):
    """Both loops solve S dc = b; at rel_tol both reach, the device steps may differ by what the reference's two
    converged solutions differ by plus each one's own bound."""
    ba, _ = _make("small grid culled")
    P = _ref(ba, R.LD)
    lam, tol = 1e-2, 1e-10
    rb = PR.pcg(P, lam, 400, tol, kind="block_jacobi", runs=3)
    rs = PR.pcg(P, lam, 400, tol, kind="schur_jacobi", runs=3)
    assert rb["status"] == 0 and rs["status"] == 0
    dcb, dpb, ib = ba.solve_step(lam, max_iters=400, rel_tol=tol)
    dcb, dpb = _np(dcb).copy(), _np(dpb).copy()
    ba.set_preconditioner("schur_jacobi")
    dcs, dps, i_s = ba.solve_step(lam, max_iters=400, rel_tol=tol)
    dcs, dps = _np(dcs), _np(dps)
    assert ib["status"] == 0 and i_s["status"] == 0, (ib, i_s)
    for key, got_b, got_s in (("x", dcb, dcs), ("dp", dpb, dps)):
        gap = float(np.linalg.norm((rb[key][-1] - rs[key][-1]).astype(np.float64)))
        bound = gap + rb["bound"][key][-1] + rs["bound"][key][-1]
        err = float(np.linalg.norm(got_b - got_s))
        print("SJREF step agreement %s: |bj - sj| %.3g, bound %.3g (reference gap %.3g), iterations %d vs %d"
              % (key, err, bound, gap, ib["iterations"], i_s["iterations"]))
        assert err <= bound, (key, err, bound)
    ba.close()


def test_default_path_is_untouched_and_the_solve_is_deterministic(env):
    lam = 1e-4
    plain, _ = _make("small grid culled")
    want = [_np(t).copy() for t in plain.solve_step(lam, max_iters=7, rel_tol=0.0)[:2]]
    assert plain.preconditioner == "block_jacobi" and plain.preconditioner_fallbacks() == 0
    plain.close()
    ba, _ = _sj("small grid culled")
    assert ba.preconditioner == "schur_jacobi"
    a = [_np(t).copy() for t in ba.solve_step(lam, max_iters=7, rel_tol=0.0)[:2]]
    b = [_np(t).copy() for t in ba.solve_step(lam, max_iters=7, rel_tol=0.0)[:2]]
    assert _bits(a[0], b[0]) and _bits(a[1], b[1])               # the same problem and arguments: the same bits
    assert not _bits(a[0], want[0])
    ba.set_preconditioner("block_jacobi")
    got = [_np(t).copy() for t in ba.solve_step(lam, max_iters=7, rel_tol=0.0)[:2]]
    assert _bits(got[0], want[0]) and _bits(got[1], want[1])     # kind 0 after kind 1 == a handle that never had one set
    assert ba.preconditioner_fallbacks() == 0
    with pytest.raises(ValueError):
        ba.set_preconditioner("jacobi")
    from city2ba_amd import _lib as L
    with pytest.raises(L.City2baError):
        ba.set_preconditioner(2)
    assert ba.preconditioner == "block_jacobi"
    ba.close()


def test_setting_survives_upload_and_cull(env):
    from test_gpu_schur_step import _grid
    g = _grid(cull=False)
    g.set_preconditioner("schur_jacobi")
    g.cull()
    assert g.preconditioner == "schur_jacobi"
    bal9, pts, rp, pi, uv = g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), g.observations()
    uv = uv + np.random.default_rng(3).normal(scale=1e-2, size=uv.shape)     # exact observations would make b = 0
    g._upload(bal9, True, pts, rp, pi, uv)
    assert g.preconditioner == "schur_jacobi"
    _, _, info = g.solve_step(1e-2, max_iters=3, rel_tol=0.0)
    assert info["iterations"] == 3 and g.preconditioner_fallbacks() == 0
    g.close()


# ---- 5. fallback ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIVE)
def test_no_fallback_on_the_five_problems(env, name):
    ba, _ = _sj(name)
    for lam in (1e-4, 1.0):
        _, _, info = ba.solve_step(lam, max_iters=2, rel_tol=0.0)
        assert info["status"] == 1 and ba.preconditioner_fallbacks() == 0, (name, lam, info, ba.preconditioner_fallbacks())
    ba.close()


def test_damping_range_gives_finite_steps(env):
    from city2ba_amd.solve import LAMBDA_MAX, LAMBDA_MIN
    ba = _sparse_problem()
    ba.set_preconditioner("schur_jacobi")
    seen = []
    for lam in (LAMBDA_MIN, 1e-16, 1e-14, 1e-12, 1e2, LAMBDA_MAX):
        it, tol = (8, 0.0) if lam < 1.0 else (100, 1e-6)
        dc, dp, info = ba.solve_step(lam, max_iters=it, rel_tol=tol)
        dc, dp = _np(dc), _np(dp)
        seen.append((lam, info["status"], info["iterations"], ba.preconditioner_fallbacks()))
        assert np.isfinite(dc).all() and np.isfinite(dp).all(), (lam, info)
        assert all(np.isfinite(v) for v in info.values()), (lam, info)
        assert 0 <= ba.preconditioner_fallbacks() <= ba.num_cameras()
    print("SJREF damping range (lam, status, iterations, fallbacks):", seen)
    ba.close()


# ---- 6. the LM loop ---------------------------------------------------------------------------------------------------
def test_lm_loop_reaches_the_same_error_in_fewer_pcg_iterations(env):
    """Both loops solve every step to rel_tol 1e-10.  The reference's two converged solutions of the first linearisation
    differ by a relative eta in the step (their gap plus each one's bound, floored at 1e-13); the error after a step is
    at most quadratic in the step, so a step moved by eta moves it by about 2 eta of what the step gained, and the damping
    update and the later steps, which contract towards the same minimum, carry that on without amplifying it.  The final
    errors are therefore held to 16 x iterations x 2 eta, relative.  That Schur-Jacobi needs fewer PCG iterations on this
    input is first confirmed on the reference (the first linearisation's two counts), then asserted of the loops."""
    from city2ba_amd.solve import levenberg_marquardt
    its, lam, tol = 6, 1e-4, 1e-10
    out = {}
    for kind in ("block_jacobi", "schur_jacobi"):
        ba, _ = _make("grid culled")
        if kind == "block_jacobi":
            P = _ref(ba, R.LD)
            rb = PR.pcg(P, lam, 3000, tol, kind="block_jacobi", runs=1)
            rs = PR.pcg(P, lam, 3000, tol, kind="schur_jacobi", runs=1)
            print("SJREF lm reference first step: block-Jacobi %d iterations, Schur-Jacobi %d" % (rb["iterations"], rs["iterations"]))
            assert rb["status"] == 0 and rs["status"] == 0 and rs["iterations"] < rb["iterations"]
            gap = float(np.linalg.norm((rb["x"][-1] - rs["x"][-1]).astype(np.float64))) + rb["bound"]["x"][-1] + rs["bound"]["x"][-1]
            eta = max(gap / float(np.linalg.norm(rb["x"][-1].astype(np.float64))), 1e-13)
        hist = levenberg_marquardt(ba, its, lam=lam, max_iters=3000, rel_tol=tol, preconditioner=kind)
        assert ba.preconditioner == kind and all(h["status"] == 0 for h in hist), [(h["status"], h["pcg_iterations"]) for h in hist]
        out[kind] = (hist[-1]["error_after"], sum(h["pcg_iterations"] for h in hist), [h["accepted"] for h in hist])
        ba.close()
    (eb, nb, ab), (es, ns, as_) = out["block_jacobi"], out["schur_jacobi"]
    bound = 16 * its * 2 * eta
    print("SJREF lm: final error %.15g (block-Jacobi, %d PCG iterations) %.15g (Schur-Jacobi, %d); |diff| / error %.3g, bound %.3g"
          % (eb, nb, es, ns, abs(eb - es) / eb, bound))
    assert ab == as_ and abs(eb - es) <= bound * eb, (eb, es, bound, ab, as_)
    assert ns < nb, (ns, nb)
