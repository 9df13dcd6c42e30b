"""c2b_problem_solve_step's PCG held to the reference loop of tests/_schurref.py (pcg), iterate by iterate: with
rel_tol = 0 and max_iters = k the solve returns the k-th iterate, whose dc, dp, recurrence residual and energy must lie
within bounds that seeded f64-scale perturbations of the longdouble reference give; the stopping rule to the exact
iteration; a mid-size problem whose reductions span several workgroups; and the damping's whole accepted range."""
import numpy as np
import pytest

import _schurref as R
import _solvecheck as SC
from test_gpu_schur_step import _make, _np, _ref, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
EPS = R.EPS
KS = (0, 1, 2, 3, 5, 8, 13)


_over, _sum_sq, _model_tol = SC.over, SC.sum_sq, SC.model_tol


def _check_iterates(ba, lam, ks, runs=8, tag=""):
    """solve_step(lam, k, 0) against pcg for every k in ks (tests/_solvecheck.py's check_iterates: the worst |err| / bound
    per quantity is printed); returns the reference"""
    P = _ref(ba, R.LD)
    return SC.check_iterates(ba, P, R.pcg(P, lam, max(ks), 0.0, runs=runs), lam, ks, tag=tag, label="PCGREF")


# ---- 1. every iterate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random bal", "random state", "mixed k2", "small grid culled"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_iterates_follow_the_reference(env, name, lam):
    ba, _ = _make(name)
    _check_iterates(ba, lam, KS, tag=name)
    ba.close()


# ---- 2. stopping ------------------------------------------------------------------------------------------------------
_crossing_tols = SC.crossing_tols


@pytest.mark.parametrize("name", ["random bal", "mixed k2"])
def test_stopping_iteration_is_exact(env, name):
    ba, _ = _make(name)
    P = _ref(ba, R.LD)
    lam = 1e-4
    ref = R.pcg(P, lam, max(KS), 0.0)
    tols = _crossing_tols(ref, 4)
    assert len(tols) >= 3, ref["rel"]
    for K, tol in tols:
        _, _, info = ba.solve_step(lam, max_iters=200, rel_tol=tol)
        assert info["status"] == 0 and info["iterations"] == K, (name, K, tol, info)
        assert info["rel_residual"] <= tol
    ba.close()


# ---- 3. mid size: several workgroups in every reduction ------------------------------------------------------------------
def test_mid_size_iterates_and_stopping(env):
    ba, _ = _make("mid grid")
    nc, no = ba.num_cameras(), ba.num_observations()
    print("PCGREF mid grid: n_cam %d, n_obs %d, n_pts %d" % (nc, no, ba.num_points()))
    assert nc == 2879 and nc % 4 == 3 and nc > 1024 and no > 65536
    lam = 1e-4
    ref = _check_iterates(ba, lam, (0, 1, 3), runs=3, tag="mid grid")
    tols = _crossing_tols(ref, 2)
    assert tols, ref["rel"]
    for K, tol in tols:
        _, _, info = ba.solve_step(lam, max_iters=50, rel_tol=tol)
        assert info["status"] == 0 and info["iterations"] == K, (K, tol, info)
    ba.close()


# ---- 4. the damping's range --------------------------------------------------------------------------------------------
def _sparse_problem():
    """a grid whose rows are cut so that some cameras keep 1-4 observations and some points are seen once"""
    import city2ba_amd as c2b
    from test_gpu_schur_step import _grid
    g = _grid(cull=True)
    bal9, pts, rp, pi = g.cameras_bal(), g.points(), g.row_ptr.astype(np.int64), g.pt_idx.astype(np.int64)
    uv = g.observations() + np.random.default_rng(9).normal(scale=1e-2, size=(g.num_observations(), 2))
    g.close()
    keep, counts = [], []
    for c in range(len(bal9)):
        rows = np.arange(rp[c], rp[c + 1])
        k = c % 6
        if 1 <= k <= 4:
            rows = rows[:k]
        keep.append(rows)
        counts.append(len(rows))
    keep = np.concatenate(keep)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    ba = c2b.BAProblem.from_bal(bal9, pts, row_ptr, pi[keep].astype(np.uint32), uv[keep])
    kc = np.diff(row_ptr.astype(np.int64))
    kp = np.bincount(pi[keep], minlength=len(pts))
    assert ((kc >= 1) & (kc <= 4)).sum() >= 8 and (kp == 1).sum() >= 8, (np.bincount(kc)[:6], (kp == 1).sum())
    return ba


def test_damping_range_gives_finite_steps(env):
    from city2ba_amd.solve import LAMBDA_MAX, LAMBDA_MIN, levenberg_marquardt
    ba = _sparse_problem()
    P = _ref(ba, R.LD)
    seen = []
    for lam in (LAMBDA_MIN, 1e-16, 1e-14, 1e-12, 1e2, LAMBDA_MAX):
        small = lam < 1.0
        it, tol = (8, 0.0) if small else (100, 1e-6)
        dc, dp, info = ba.solve_step(lam, max_iters=it, rel_tol=tol)
        dc, dp = _np(dc), _np(dp)
        seen.append((lam, info["status"], info["iterations"], float(np.abs(dp).max())))
        assert np.isfinite(dc).all() and np.isfinite(dp).all(), (lam, info)
        assert all(np.isfinite(v) for v in info.values()), (lam, info)
        with np.errstate(all="ignore"):                          # the longdouble factors fail too at the low end
            ref = R.pcg(P, lam, it, tol, runs=0)
        if info["status"] == 2:
            zero = not dc.any() and not dp.any()
            if zero:
                assert info["model_decrease"] == 0.0, (lam, info)
            else:                                                    # the last good iterate, bit for bit
                dc2, _, info2 = ba.solve_step(lam, max_iters=info["iterations"], rel_tol=0.0)
                assert np.array_equal(_np(dc2), dc) and info2["iterations"] == info["iterations"], (lam, info, info2)
        else:
            assert info["status"] == ref["status"], (lam, info, ref["status"], ref["iterations"])
    print("PCGREF damping range (lam, status, iterations, max |dp|):", seen)
    e0 = ba.total_reprojection_error(2.0)
    hist = levenberg_marquardt(ba, 8, lam=1e-16)
    assert np.isfinite(ba.cameras_bal()).all() and np.isfinite(ba.points()).all()
    e1 = ba.total_reprojection_error(2.0)
    print("PCGREF lm from 1e-16: %g -> %g" % (e0, e1), [(h["lam"], h["accepted"], h["status"]) for h in hist])
    assert e1 <= e0 and all(LAMBDA_MIN <= h["lam"] <= LAMBDA_MAX for h in hist)
    ba.close()


def test_damping_range_ends(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    from city2ba_amd.solve import LAMBDA_MAX, LAMBDA_MIN, _clamp
    assert (LAMBDA_MIN, LAMBDA_MAX) == (1e-20, 1e32) and _clamp(1e-40) == LAMBDA_MIN and _clamp(1e40) == LAMBDA_MAX
    ba, _ = _make("random bal")
    for lam in (LAMBDA_MIN, LAMBDA_MAX):
        ba.solve_step(lam, max_iters=2)
    for lam in (LAMBDA_MIN * 0.99, LAMBDA_MAX * 1.01, 0.0, float("inf")):
        with pytest.raises(L.City2baError):
            ba.solve_step(lam)
    lib = L.lib()
    for lam in (LAMBDA_MIN * 0.99, LAMBDA_MAX * 1.01):
        assert lib.c2b_schur_points_rows(None, None, 0, None, None, None, None, None, lam, None, None, None, None) == L.ERR_INVALID_ARGUMENT
        assert lib.c2b_schur_cameras_rows(None, None, None, 0, None, None, 0, None, lam, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    for lam in (LAMBDA_MIN, LAMBDA_MAX):
        assert lib.c2b_schur_points_rows(None, None, 0, None, None, None, None, None, lam, None, None, None, None) == 0
        assert lib.c2b_schur_cameras_rows(None, None, None, 0, None, None, 0, None, lam, None, None, None, None) == 0
    ba.close()
