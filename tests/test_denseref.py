"""tests/_denseref.py held to what is already trusted, without a GPU: its blocked Cholesky and substitutions are numpy.linalg's, its
bounds are met by a plain f64 factorisation and missed by a factor moved a little, its failed pivot is reported as the header says,
its dense image is _explicitref.dense's lower triangle and _schurref.Problem.dense_S, and its direct step is the dense solve."""
import numpy as np
import pytest

import _denseref as DR
import _explicitref as X
import _schurref as R
from test_explicitref import _problem

SIZES = [1, 9, 63, 64, 65, 129, 193]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_blocked_cholesky_and_substitution_are_numpys(n, scaled):
    A = DR.spd(n, seed=n, scaled=scaled)
    assert np.array_equal(A, A.T)
    img = DR.lower_image(A)
    Np = DR.padded(n)
    assert img.shape == (Np, Np) and not np.triu(img, 1).any() and np.array_equal(img[n:, :], np.eye(Np)[n:, :])
    L, info = DR.cholesky(img.astype(DR.LD))
    assert info == 0 and L.dtype == DR.LD and not np.triu(L, 1).any()
    assert np.array_equal(L[n:, :].astype(np.float64), np.eye(Np)[n:, :])          # the padding rows stay rows of the identity
    want = np.linalg.cholesky(A)
    scale = np.abs(want) @ np.abs(want).T                                        # |L| |L^T|: what an f64 factor may be off by, times n eps
    err = np.abs(L[:n, :n].astype(np.float64) @ L[:n, :n].astype(np.float64).T - A)
    assert (err <= 4 * (n + 1) * R.EPS * scale).all()
    d = np.sqrt(np.diag(A))
    assert np.abs((L[:n, :n].astype(np.float64) - want) / d[:, None]).max() <= 1e-9          # (row-scaled: D A D has entries over 12 decades)
    b = np.random.default_rng(n).normal(size=n)
    x = DR.solve(L, np.concatenate([b, np.zeros(Np - n)]))
    assert not x[n:].any()
    xw = np.linalg.solve(A, b)
    assert np.linalg.norm((x[:n].astype(np.float64) - xw) * d) <= 1e-9 * np.linalg.norm(xw * d)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_bounds_hold_for_a_plain_f64_factorisation_and_not_for_a_moved_one(n, scaled):
    A = DR.spd(n, seed=100 + n, scaled=scaled)
    img = DR.lower_image(A)
    L, info = DR.cholesky(img)                                                   # every operation rounded to f64
    assert info == 0 and L.dtype == np.float64
    fe = DR.factor_excess(img, L, n)
    b = np.random.default_rng(n).normal(size=DR.padded(n))
    b[n:] = 0.0
    x = DR.solve(L, b)
    se = DR.solve_excess(img, L, x, b, n)
    print("DENSEREF n=%d scaled=%d: f64 host factor |A - L L^T| / bound %.3g, |b - A x| / bound %.3g" % (n, scaled, fe, se))
    assert fe <= 1.0 and se <= 1.0
    # the bounds have teeth: one entry of the factor moved by 1e-10 of itself, one entry of the solution likewise
    M = L.copy()
    M[n - 1, 0 if n > 1 else n - 1] *= 1 + 1e-10
    if M[n - 1, 0]:
        assert DR.factor_excess(img, M, n) > 1.0
    y = x.copy()
    y[0] *= 1 + 1e-8
    assert DR.solve_excess(img, L, y, b, n) > 1.0
    assert DR.gamma(n + 1) < 2 * (n + 1) * DR.U and DR.gamma(3 * n + 1) > (3 * n + 1) * DR.U


@pytest.mark.parametrize("k", [0, 63, 64, 100])
@pytest.mark.parametrize("bad", [-1.0, float("nan"), 0.0, float("inf")])
def test_first_failed_pivot_is_reported_one_based_and_replaced_by_one(k, bad):
    A = np.eye(193)
    A[k, k] = bad
    A[150, 150] = -2.0                                                           # a later one: not the one reported
    L, info = DR.cholesky(DR.lower_image(A))
    assert info == k + 1
    assert np.array_equal(L, np.eye(256))                                        # both pivots replaced by 1, nothing else touched


@pytest.mark.parametrize("name", ["dome dup", "random"])
def test_dense_image_is_the_assembled_blocks_and_dense_S(name):
    P = _problem(name)
    lam = 1e-2
    ref = X.blocks(P, lam)
    D, E = ref["D"].astype(np.float64), ref["E"].astype(np.float64)
    img = DR.image_of_blocks(ref["nbr_ptr"], ref["nbr"], D, E)
    n, Np = 9 * P.n_cam, DR.padded(9 * P.n_cam)
    S = X.dense(ref, P.n_cam)
    assert img.shape == (Np, Np) and np.array_equal(img[:n, :n], np.tril(S)) and not np.triu(img, 1).any()
    assert np.array_equal(img[n:, :], np.eye(Np)[n:, :])
    want = P.dense_S(lam)
    assert np.abs(np.tril(want) - img[:n, :n]).max() <= 1e-12 * np.abs(want).max()
    SL = DR.assemble(ref["nbr_ptr"], ref["nbr"], ref["D"], ref["E"], dtype=DR.LD)
    assert SL.dtype == DR.LD and np.array_equal(SL.astype(np.float64), S)
    kc = np.bincount(P.cam, minlength=P.n_cam)
    for c in np.flatnonzero(kc == 0):                                            # an empty camera: lambda 1e-6 I and nothing beside it
        assert np.array_equal(S[9 * c:9 * c + 9, 9 * c:9 * c + 9], np.diag(np.full(9, lam * 1e-6)))
        assert not S[9 * c:9 * c + 9, :9 * c].any() and not S[9 * c + 9:, 9 * c:9 * c + 9].any()


@pytest.mark.parametrize("name", ["dome nodup", "random"])
def test_direct_step_is_the_dense_solve_both_ways(name):
    P = _problem(name)
    P64 = _problem(name, np.float64)
    for lam in ((1e-4, 1.0) if name == "random" else (1e-4,)):               # (the dome's blocks take a second per evaluation)
        # the two longdouble solves differ by a hundredth of what an f64 evaluation is allowed (both carry ~cond 2^-64, f64 ~cond 2^-53)
        ref = DR.direct_step_bound(P, lam, runs=2)
        dc, dp = ref["x"], ref["dp"]
        other = "refined" if 9 * P.n_cam <= DR.LD_DIRECT_MAX else "cholesky"      # (the bound's solves were the other kind)
        rc, rp = DR.direct_step(P, lam, how=other)
        nx, nd = np.linalg.norm(dc.astype(np.float64)), np.linalg.norm(dp.astype(np.float64))
        gx, gd = np.linalg.norm((dc - rc).astype(np.float64)), np.linalg.norm((dp - rp).astype(np.float64))
        print("DENSEREF %s lam=%g: |cholesky - refined| / bound: dc %.3g dp %.3g" % (name, lam, gx / ref["bound_x"], gd / ref["bound_dp"]))
        assert gx <= 1e-2 * ref["bound_x"] and gd <= 1e-2 * ref["bound_dp"]
        wc, wp = P64.schur_direct(lam)
        assert np.linalg.norm(dc.astype(np.float64) - wc) <= 1e-7 * nx and np.linalg.norm(dp.astype(np.float64) - wp) <= 1e-7 * nd
    assert 0 < ref["bound_x"] <= 1e-6 * np.linalg.norm(ref["x"].astype(np.float64))                # never a bound that holds nothing
    assert ref["bound_x"] >= 1e-13 * np.linalg.norm(ref["x"].astype(np.float64))
    kc = np.bincount(P.cam, minlength=P.n_cam)
    assert not ref["x"][kc == 0].any()                                           # an empty camera: b = 0 there, the step is exactly 0
