"""Robust losses (Huber, Cauchy, soft-L1) in the device step, by iteratively reweighted least squares
(BAProblem.set_loss / robust_cost, the *_rows_loss Level-0 passes, solve.levenberg_marquardt(loss=...)), against the
reweighted host reference of tests/_robustref.py built from the device's own residual and Jacobian.

The problems are those of test_gpu_schur_step._problems() with a seeded 2 % of the observations replaced by pixels
drawn uniformly over the image area the problem's observations span.  The scale a of every loss is twice the median
residual norm of the problem (for Gaussian noise of deviation sigma the median of |r| is 1.18 sigma: a = 2.35 sigma, which
5 % of the inliers exceed); the tests assert that between 1 % and 50 % of the observations lie past a -- the
observations whose Huber weight is < 1, and whose Cauchy / soft-L1 weight is below 1/2 and 1/sqrt(2)."""
import ctypes as C

import numpy as np
import pytest

import _normref as NR
import _robustref as B
import _schurref as R
import test_gpu_schur_pcg as PCG
from test_gpu_schur_step import _bits, _cam_of, _grid, _level0, _make, _np, _problems, env  # noqa: F401  (env: the module fixture)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
LOSSES = ("huber", "cauchy", "soft_l1")
PROBLEMS = [name for name, _ in _problems()]                  # the whole set: the six of test_gpu_schur_step and its two small grids


def _with_outliers(name, frac=0.02, seed=77):
    """the problem `name` with a seeded `frac` of its observations replaced by uniform pixels; returns (ba, bal, a)"""
    ba, bal = _make(name)
    uv = ba.observations().copy()
    rng = np.random.default_rng(seed)
    bad = rng.random(len(uv)) < frac
    lo, hi = uv.min(axis=0), uv.max(axis=0)
    uv[bad] = rng.uniform(lo, hi, size=(int(bad.sum()), 2))
    cams = ba.cameras_bal() if bal else ba.cameras()
    ba._upload(cams, bal, ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), uv)
    r, _, _ = ba.residual_jacobian()
    a = 2.0 * float(np.median(np.linalg.norm(np.asarray(r).reshape(-1, 2), axis=1)))
    w = B.weights("huber", a, r)
    past = float(np.mean(w < 1))
    assert 0.01 <= past <= 0.5, (name, a, past)               # a condition on the input: both sides of a^2 are populated
    assert np.array_equal(w < 1, B._s(r) > B.LD(a) * B.LD(a))
    return ba, bal, a


def _lin(ba):
    r, Jc, Jp = ba.residual_jacobian()
    return r, Jc, Jp, _cam_of(ba.row_ptr), ba.pt_idx.astype(np.int64), ba.num_cameras(), ba.num_points()


# ---- 4. the squared-loss path is what it was ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random state", "grid culled"])
def test_squared_loss_path_is_bit_equal_to_a_problem_without_a_loss(env, name):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ba0, bal = _make(name)
    want_ne = ba0.normal_equations()
    want_step = ba0.solve_step(1e-2, max_iters=7, rel_tol=0.0)
    ba, _ = _make(name)
    for setter in (lambda: ba.set_loss(None), lambda: ba.set_loss(None, 3.0), lambda: ba.set_loss("squared", 1e-3),
                   lambda: (ba.set_loss("cauchy", 0.01), ba.set_loss(None))):
        setter()
        assert ba.loss == (None, 1.0)
        got = ba.normal_equations()
        for x, y in zip(got[:4], want_ne[:4]):
            assert _bits(_np(x), _np(y))
        assert got[4] == want_ne[4]
        dc, dp, info = ba.solve_step(1e-2, max_iters=7, rel_tol=0.0)
        assert _bits(_np(dc), _np(want_step[0])) and _bits(_np(dp), _np(want_step[1])) and info == want_step[2]
        e = ba.total_reprojection_error(2.0) ** 2
        assert abs(ba.robust_cost() - e) <= 1e-12 * e
    # Level 0: loss = (None, scale) goes through the *_rows_loss entries with kind 0
    camblk, pts4, rows, prows, pi, uv = _level0(env, ba, bal)
    nc, npt = ba.num_cameras(), ba.num_points()
    f64 = dict(dtype=torch.float64, device=dev)
    outs = []
    for loss in (None, (None, 5.0)):
        U, gc = torch.empty((nc, 9, 9), **f64), torch.empty((nc, 9), **f64)
        V, gp = torch.empty((npt, 3, 3), **f64), torch.empty((npt, 3), **f64)
        t, y = torch.empty((npt, 3), **f64), torch.empty((nc, 9), **f64)
        D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U, gc, loss=loss)
        D.normal_points_rows(camblk, pts4, prows, uv, V, gp, loss=loss)
        x = torch.from_numpy(np.random.default_rng(5).normal(size=(nc, 9))).to(dev)
        D.schur_points_rows(camblk, pts4, prows, uv, V, 1e-2, x, gp, t, loss=loss)
        D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, 1e-2, x, t, y, loss=loss)
        outs.append([_np(a) for a in (U, gc, V, gp, t, y)])
    for x, y in zip(*outs):
        assert _bits(x, y)
    for x, y in zip(outs[0][:4], want_ne[:4]):
        assert _bits(x, _np(y))
    ba.close()
    ba0.close()


# ---- 5. the reweighted blocks ------------------------------------------------------------------------------------------
# Roundings the weighting adds to one product (sqrt(w) J_a)(sqrt(w) J_b) of the device, in units u = 2^-53 relative to
# the product: s = r0 r0 + r1 r1 carries 2 (two products, one sum of positive terms); a^2 = a * a on the host 1; w at
# most 3 more (s / a^2, 1 + ., 1 / . -- Cauchy, the longest chain; Huber and soft-L1 halve part of theirs in a sqrt): 6;
# sqrt(w) halves that and rounds: 4; the scaling of an entry 1 more: 5 per factor.  The reference's weighted entries are
# rounded to f64 once each (_normref.blocks takes f64): 1 per factor.  Two factors: 12.
_WEIGHT_OPS = 12


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", PROBLEMS)
def test_normal_equations_under_a_loss(env, name, loss):
    ba, bal, a = _with_outliers(name)
    r, Jc, Jp, cam_of, pt, nc, npt = _lin(ba)
    wr, wJc, wJp = B.reweighted(loss, a, r, Jc, Jp)
    ref = NR.blocks(wr.astype(np.float64), wJc.astype(np.float64), wJp.astype(np.float64), cam_of, pt, nc, npt)
    ba.set_loss(loss, a)
    U, gc, V, gp, s = ba.normal_equations()
    for dev_a, key, S, k in ((U, "U", "SU", "kc"), (gc, "gc", "Sgc", "kc"), (V, "V", "SV", "kp"), (gp, "gp", "Sgp", "kp")):
        x = NR.excess(_np(dev_a), ref[key], ref[S], ref[k] + _WEIGHT_OPS)
        print("ROBUST blocks %s %s %s: %.3g x the bound" % (name, loss, key, x))
        assert x <= 1.0, (name, loss, key, x)
    want = float(np.sum(B.weights(loss, a, r) * B._s(r)))
    assert abs(s - want) <= 1e-12 * want, (s, want)                       # the weighted sum of squares
    _, _, _, _, s2 = ba.normal_equations(out=(None, None, None, None))     # ... and without the blocks
    assert abs(s2 - want) <= 1e-12 * want, (s2, want)
    ba.close()


# ---- 6. operator, right-hand side, back-substitution ---------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", PROBLEMS)
def test_operator_rhs_and_back_substitution_under_a_loss(env, name, loss):
    """the criterion of test_gpu_schur_step.test_operator_rhs_and_back_substitution: 1e-12 of the absolute-value scale"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ba, bal, a = _with_outliers(name)
    ref = B.problem(loss, a, *_lin(ba), dtype=R.LD)
    nc, npt = ba.num_cameras(), ba.num_points()
    ba.set_loss(loss, a)
    U, gc, V, gp, _ = ba.normal_equations()
    camblk, pts4, rows, prows, pi, uv = _level0(env, ba, bal)
    f64 = dict(dtype=torch.float64, device=dev)
    t, y = torch.empty((npt, 3), **f64), torch.empty((nc, 9), **f64)
    rng = np.random.default_rng(7)
    la = (loss, a)
    for lam in (1e-2, 1.0):
        x = rng.normal(size=(nc, 9))
        xt = torch.from_numpy(x).to(dev)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, xt, None, t, loss=la)
        D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, lam, xt, t, y, loss=la)
        want, scale = ref.S_times(lam, x)
        err = np.linalg.norm((_np(y).astype(R.LD) - want).astype(np.float64))
        q = err / np.linalg.norm(scale.astype(np.float64))
        print("ROBUST operator %s %s lam=%g: S x %.3g" % (name, loss, lam, q))
        assert q <= 1e-12, (name, loss, lam, q)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, None, gp, t, loss=la)
        D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, lam, None, t, y, loss=la)
        b = -_np(gc) - _np(y)
        want, scale = ref.rhs(lam)
        q = np.linalg.norm((b.astype(R.LD) - want).astype(np.float64)) / np.linalg.norm(scale.astype(np.float64))
        print("ROBUST operator %s %s lam=%g: b %.3g" % (name, loss, lam, q))
        assert q <= 1e-12, (name, loss, "b", lam, q)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, xt, gp, t, loss=la)
        want, scale = ref.back_substitute(lam, x)
        q = np.linalg.norm((-_np(t).astype(R.LD) - want).astype(np.float64)) / np.linalg.norm(scale.astype(np.float64))
        print("ROBUST operator %s %s lam=%g: dp %.3g" % (name, loss, lam, q))
        assert q <= 1e-12, (name, loss, "dp", lam, q)
    ba.close()


# ---- 7. PCG iterates under Cauchy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random bal", "small grid culled"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_pcg_iterates_under_cauchy_follow_the_reweighted_reference(env, monkeypatch, name, lam):
    """test_gpu_schur_pcg._check_iterates with its bounds as they are; only the reference problem it builds is the
    reweighted one"""
    ba, bal, a = _with_outliers(name)
    ba.set_loss("cauchy", a)
    monkeypatch.setattr(PCG, "_ref", lambda p, dtype=np.float64: B.problem("cauchy", a, *_lin(p), dtype=dtype))
    PCG._check_iterates(ba, lam, PCG.KS, tag="cauchy " + name)
    ba.close()


# ---- 8. the robust cost ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES + (None,))
@pytest.mark.parametrize("name", PROBLEMS)
def test_robust_cost(env, name, loss):
    """sum rho(s) against the longdouble sum.  Every term is positive, so the bound is relative to the sum itself: a
    term's own rounding is at most 16 units of 2^-53 (s: 2; a^2: 1; then the longest chain, Cauchy's s / a^2, log1p at
    <= 2 ulp with condition <= 1, times a^2; Huber's 2 sqrt(a^2 s) - a^2 loses at most a factor 2 to its subtraction,
    as rho >= a^2 there) and it passes through at most `depth` additions: 6 + 3 in its workgroup (xor-free wave tree,
    four waves), ceil(n_blocks / 256) in a thread of k_normal_sum, 6 + 3 again.  Bound: sum x 2^-52 x (depth + 16),
    independent of how many observations there are."""
    ba, bal, a = _with_outliers(name)
    r, _, _ = ba.residual_jacobian()
    ba.set_loss(loss, a)
    want = np.sum(B.cost(loss, a, r))
    got = ba.robust_cost()
    n_blocks = -(-ba.num_observations() // 256)
    depth = 18 + -(-n_blocks // 256)
    err = abs(float(B.LD(got) - want))
    bound = float(want) * EPS * (depth + 16)
    print("ROBUST cost %s %s: %.17g err %.3g bound %.3g" % (name, loss, got, err, bound))
    assert err <= bound, (name, loss, got, float(want), err, bound)
    assert got == ba.robust_cost()
    if loss is not None:
        assert got < ba.total_reprojection_error(2.0) ** 2                 # rho(s) <= s, strictly past the scale
    ba.close()


# ---- 9. determinism, state, bad arguments ----------------------------------------------------------------------------------
def test_determinism_and_the_loss_survives_cull_and_upload(env):
    import city2ba_amd as c2b
    g = _grid(cull=False)
    uv = g.observations() + np.random.default_rng(3).normal(scale=1e-2, size=(g.num_observations(), 2))
    ba = c2b.BAProblem.from_bal(g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), uv)
    g.close()
    assert ba.loss == (None, 1.0)
    ba.set_loss("soft_l1", 0.02)
    a = ba.solve_step(1e-3, max_iters=20, rel_tol=1e-8)
    b = ba.solve_step(1e-3, max_iters=20, rel_tol=1e-8)
    assert _bits(_np(a[0]), _np(b[0])) and _bits(_np(a[1]), _np(b[1])) and a[2] == b[2]
    n0 = ba.num_observations()
    ba.cull()
    assert ba.num_observations() < n0 and ba.loss == ("soft_l1", 0.02)
    c1 = ba.robust_cost()
    ba._upload(ba.cameras_bal(), True, ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
    assert ba.loss == ("soft_l1", 0.02) and ba.robust_cost() == c1
    # a fresh problem with the same loss gives the same step
    fresh = c2b.BAProblem.from_bal(ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
    fresh.set_loss("soft_l1", 0.02)
    x, y = ba.solve_step(1e-3, max_iters=5, rel_tol=0.0), fresh.solve_step(1e-3, max_iters=5, rel_tol=0.0)
    assert _bits(_np(x[0]), _np(y[0])) and _bits(_np(x[1]), _np(y[1])) and x[2] == y[2]
    # and a different one than the squared loss
    fresh.set_loss(None)
    z = fresh.solve_step(1e-3, max_iters=5, rel_tol=0.0)
    assert not _bits(_np(x[0]), _np(z[0]))
    fresh.close()
    ba.close()


def test_bad_loss_arguments_are_refused(env):
    from city2ba_amd import _lib as L
    torch, D, dev = env["torch"], env["D"], env["dev"]
    lib = L.lib()
    ba, bal = _make("random bal")
    ba.set_loss("huber", 0.5)
    for kind, scale in ((-1, 1.0), (4, 1.0), (1, 0.0), (2, -1.0), (3, float("nan")), (1, float("inf"))):
        assert lib.c2b_problem_set_loss(ba._h, kind, scale) == L.ERR_INVALID_ARGUMENT, (kind, scale)
        assert b"loss" in lib.c2b_last_error()
    assert ba.loss == ("huber", 0.5)                                       # a refused call changes nothing
    assert lib.c2b_problem_set_loss(None, 0, 1.0) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_problem_set_loss(ba._h, 0, float("nan")) == 0           # kind 0 ignores the scale
    assert ba.loss == (None, 1.0)
    assert lib.c2b_problem_robust_cost(ba._h, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_problem_get_loss(None, None, None) == L.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        ba.set_loss("tukey", 1.0)
    camblk, pts4, rows, prows, pi, uv = _level0(env, ba, bal)
    nc, npt = ba.num_cameras(), ba.num_points()
    f64 = dict(dtype=torch.float64, device=dev)
    U, gc = torch.zeros((nc, 9, 9), **f64), torch.zeros((nc, 9), **f64)
    V, gp = torch.zeros((npt, 3, 3), **f64), torch.zeros((npt, 3), **f64)
    t, y = torch.zeros((npt, 3), **f64), torch.zeros((nc, 9), **f64)
    for loss in ("cauchy", ("cauchy",), 0.5, ("tukey", 1.0)):              # not a (name, scale) pair, or no such loss
        with pytest.raises(ValueError, match="loss must be"):
            D.normal_points_rows(camblk, pts4, prows, uv, V, gp, loss=loss)
    for loss in ((5, 1.0), ("cauchy", 0.0), ("huber", float("nan"))):
        for call in (lambda: D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U, gc, loss=loss),
                     lambda: D.normal_points_rows(camblk, pts4, prows, uv, V, gp, loss=loss),
                     lambda: D.schur_points_rows(camblk, pts4, prows, uv, V, 1e-2, y, None, t, loss=loss),
                     lambda: D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, 1e-2, y, t, y, loss=loss)):
            with pytest.raises(L.City2baError) as ei:
                call()
            assert ei.value.status == L.ERR_INVALID_ARGUMENT
    ba.close()


def test_lm_loop_uses_the_robust_cost_of_a_loss_set_on_the_problem(env):
    """levenberg_marquardt(ba) on a problem that already carries a loss is levenberg_marquardt(ba, loss=...): the cost it
    compares is robust_cost(), the one the reweighted step models, not the sum of squares"""
    from city2ba_amd.solve import levenberg_marquardt
    hists, ends = [], []
    for preset in (True, False):
        ba, bal, a = _with_outliers("grid culled")
        if preset:
            ba.set_loss("cauchy", a)
            hists.append(levenberg_marquardt(ba, 3, lam=1e-3))
        else:
            hists.append(levenberg_marquardt(ba, 3, lam=1e-3, loss="cauchy", loss_scale=a))
        assert ba.loss == ("cauchy", a)
        ends.append((ba.cameras_bal(), ba.points(), ba.robust_cost()))
        ba.close()
    assert hists[0] == hists[1] and any(h["accepted"] for h in hists[0])
    assert _bits(ends[0][0], ends[1][0]) and _bits(ends[0][1], ends[1][1])
    assert hists[0][-1]["error_after"] == ends[0][2]                       # the robust cost, not sum |r|^2


# ---- 10. what it is for ----------------------------------------------------------------------------------------------------
def test_cauchy_recovers_the_inliers_that_mismatched_correspondences_pull_away(env):
    """A culled grid with observation noise (sigma = 1e-3) and 2 % of the correspondences re-attached to wrong points
    (noise.add_incorrect_correspondences), from a perturbed start: eight LM iterations with the squared loss and eight
    with Cauchy (a = 3 sigma) from the same start.  The robust run must end with the lower RMS reprojection error over
    the inliers, and its cost must fall on every accepted step.  Both RMS values are printed (ROBUST LM ...).
    On the host the same loop -- the oracle's Jacobian, _robustref.problem(...).schur_direct(lam) for the step (the dense
    damped solve through the dense Schur complement, which test_robustref.py holds to direct()), the same update of the
    damping, these inputs -- ends at an inlier RMS of 4.7944e-02 with the squared loss (one step of eight accepted: the
    mismatches, whose residuals are of order one, own the sum of squares) and 1.2797e-03 with Cauchy (eight of eight;
    the noise alone is sqrt(2) sigma = 1.41e-3 before fitting): a factor 37 of room."""
    import city2ba_amd as c2b
    from city2ba_amd import noise as N
    from city2ba_amd.solve import levenberg_marquardt
    sigma = 1e-3
    g = _grid(cull=True)
    rng = np.random.default_rng(31)
    uv = g.project() + rng.normal(scale=sigma, size=(g.num_observations(), 2))
    clean = c2b.BAProblem.from_bal(g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), uv, device=0)
    g.close()
    truth_pt = clean.pt_idx.astype(np.int64).copy()
    dirty = N.add_incorrect_correspondences(clean, 0.02, seed=9)
    assert np.array_equal(dirty.row_ptr, clean.row_ptr)
    inlier = dirty.pt_idx.astype(np.int64) == truth_pt
    assert 0.005 < 1.0 - inlier.mean() < 0.05, inlier.mean()
    b9 = dirty.cameras_bal()
    b9[:, :6] += rng.normal(scale=1e-4, size=(len(b9), 6))
    X = dirty.points() + rng.normal(scale=1e-3, size=(dirty.num_points(), 3))
    rp, pi, ob = dirty.row_ptr.copy(), dirty.pt_idx.copy(), dirty.observations()

    def run(loss):
        ba = c2b.BAProblem.from_bal(b9, X, rp, pi, ob, device=0)
        hist = levenberg_marquardt(ba, 8, lam=1e-4, max_iters=200, rel_tol=1e-8, loss=loss, loss_scale=3.0 * sigma)
        r, _, _ = ba.residual_jacobian()
        r = np.asarray(r).reshape(-1, 2)[inlier]
        ba.close()
        return float(np.sqrt(np.mean(np.sum(r * r, axis=1)))), hist

    rms_sq, h_sq = run(None)
    rms_rb, h_rb = run("cauchy")
    print("ROBUST LM inlier RMS: squared loss %.6e, Cauchy %.6e (noise %.1e); accepted %d / %d" % (
        rms_sq, rms_rb, sigma, sum(h["accepted"] for h in h_sq), sum(h["accepted"] for h in h_rb)))
    assert any(h["accepted"] for h in h_rb)
    costs = [h["cost"] for h in h_rb] + [h_rb[-1]["error_after"]]
    for k, h in enumerate(h_rb):
        if h["accepted"]:
            assert costs[k + 1] < costs[k], (k, costs)
        else:
            assert costs[k + 1] == costs[k], (k, costs)
    assert all("cost" in h and h["cost"] == h["error"] for h in h_sq)
    assert rms_rb < rms_sq, (rms_rb, rms_sq)
    clean.close()
    dirty.close()
