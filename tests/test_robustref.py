"""The host reference of the robust losses (tests/_robustref.py) checked against itself on the CPU: weights and costs
against closed forms and against each other (w = d rho / ds), the Schur route on the reweighted problem against the
dense damped solve of the reweighted system, and kind 0 against the unweighted reference bit for bit."""
import numpy as np
import pytest

import _robustref as B
import _schurref as R

LD = np.longdouble
EPS = float(np.finfo(LD).eps)
KINDS = (1, 2, 3)


def _r_of_s(s):
    """residuals [n,2] (f64) whose s is exactly the given f64 values where sqrt is exact, else near them"""
    s = np.asarray(s, dtype=np.float64)
    return np.stack([np.sqrt(s), np.zeros_like(s)], -1)


def test_weights_and_costs_at_zero_at_the_scale_and_far_out():
    a = 0.5                                               # a, a^2 and the s below are exact in binary
    a2 = a * a
    for kind in (0,) + KINDS:
        w0 = B.weights_of_s(kind, a, np.zeros(1, dtype=LD))
        assert w0[0] == 1 and B.cost_of_s(kind, a, np.zeros(1, dtype=LD))[0] == 0
    below, above = np.nextafter(LD(a2), LD(0)), np.nextafter(LD(a2), LD(1))
    s = np.array([below, LD(a2), above], dtype=LD)
    # Huber: 1 up to and at a^2, a / sqrt(s) past it: continuous, both sides 1 to first order
    w = B.weights_of_s(1, a, s)
    assert w[0] == 1 and w[1] == 1 and w[2] <= 1 and 1 - w[2] <= 4 * EPS       # 1 - eps / 2 may round to 1
    c = B.cost_of_s(1, a, s)
    assert c[0] == below and c[1] == a2 and abs(c[2] - above) <= 4 * EPS * a2
    # Cauchy and soft-L1 at s = a^2: w = 1/2 and 1/sqrt(2), rho = a^2 log 2 and 2 a^2 (sqrt 2 - 1)
    assert B.weights_of_s(2, a, s)[1] == LD(0.5)
    assert abs(B.weights_of_s(3, a, s)[1] - 1 / np.sqrt(LD(2))) <= 2 * EPS
    assert abs(B.cost_of_s(2, a, s)[1] - a2 * np.log(LD(2))) <= 4 * EPS * a2
    assert abs(B.cost_of_s(3, a, s)[1] - 2 * a2 * (np.sqrt(LD(2)) - 1)) <= 4 * EPS * a2
    for k in (2, 3):                                      # and both sides of a^2 agree there to rounding
        wk = B.weights_of_s(k, a, s)
        assert abs(wk[0] - wk[2]) <= 8 * EPS
    # huge s: the asymptotes
    big = np.array([LD(2) ** 80], dtype=LD)
    sq = np.sqrt(big[0])
    assert abs(B.weights_of_s(1, a, big)[0] - a / sq) <= 2 * EPS * a / sq
    assert abs(B.cost_of_s(1, a, big)[0] - (2 * a * sq - a2)) <= 2 * EPS * 2 * a * sq
    assert abs(B.weights_of_s(2, a, big)[0] * (big[0] / a2) - 1) <= 2.0 ** -70
    assert abs(B.cost_of_s(2, a, big)[0] - a2 * np.log(big[0] / a2)) <= 2.0 ** -60
    assert abs(B.weights_of_s(3, a, big)[0] * (sq / a) - 1) <= 2.0 ** -70
    assert abs(B.cost_of_s(3, a, big)[0] / (2 * a * sq) - 1) <= 2.0 ** -38       # 2 a sqrt(s) (1 - a / sqrt(s) + ...)
    for kind in KINDS:
        s = np.array([0, 1e-12, 1e-3, a2, 1.0, 1e6, 1e30], dtype=LD)
        w = B.weights_of_s(kind, a, s)
        assert np.all(w > 0) and np.all(w <= 1) and np.all(np.diff(w) <= 0)
        assert np.all(B.cost_of_s(kind, a, s) <= s)       # rho(s) <= s: w <= 1 and rho(0) = 0


@pytest.mark.parametrize("kind", KINDS)
def test_weight_is_the_derivative_of_the_cost(kind):
    """w = d rho / ds by a longdouble central difference.  With h = 2^-20 s the truncation error is |rho'''| h^2 / 6
    <= w h^2 / s^2 (every kind's third derivative is at most a small multiple of w / s^2) = 2^-40 w relative; the rounding
    of the difference is eps_LD rho / h <= 2^-63 2^20 (rho / (w s)) w, and rho / (w s) < 40 over the range below.  Bound
    2^-36 relative.  The points keep clear of Huber's kink (the difference would straddle it)."""
    a = 0.75
    a2 = a * a
    s = np.concatenate([np.geomspace(1e-6, 0.9, 40) * a2, np.geomspace(1.1, 1e6, 60) * a2]).astype(LD)
    h = s * LD(2.0 ** -20)
    d = (B.cost_of_s(kind, a, s + h) - B.cost_of_s(kind, a, s - h)) / (2 * h)
    w = B.weights_of_s(kind, a, s)
    assert np.max(np.abs(d - w) / w) <= 2.0 ** -36


def _random(seed, n_cam=12, n_pts=40, n_obs=160):
    """the layout of test_schurref._random with residuals on both sides of the scale a = 1"""
    rng = np.random.default_rng(seed)
    cams = np.setdiff1d(np.arange(n_cam), [0, 5])
    pts = np.setdiff1d(np.arange(n_pts), [3, 7, 11])
    cam_of = np.sort(rng.choice(cams, n_obs))
    pt_idx = rng.choice(pts, n_obs)
    pt_idx[rng.integers(n_obs)] = 11
    scale = np.array([1.0, 1.0, 1.0, 0.1, 0.1, 0.1, 1e-3, 10.0, 100.0])
    Jc = rng.normal(size=(n_obs, 2, 9)) * scale
    Jp = rng.normal(size=(n_obs, 2, 3))
    r = rng.normal(size=(n_obs, 2)) * np.where(rng.random(n_obs) < 0.1, 20.0, 0.5)[:, None]
    return r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("kind", KINDS)
def test_schur_route_on_the_reweighted_problem_equals_its_dense_damped_solve(kind, lam):
    args = _random(kind)
    w = B.weights(kind, 1.0, args[0])
    assert 0.05 < np.mean(w < 1) and np.any(w == 1) if kind == 1 else np.all(w < 1)
    P = B.problem(kind, 1.0, *args)
    # the blocks really are the weighted sums
    U = np.zeros((args[5], 9, 9), dtype=LD)
    np.add.at(U, args[3], w[:, None, None] * np.einsum("nia,nib->nab", args[1].astype(LD), args[1].astype(LD)))
    assert np.allclose(P.U, U.astype(np.float64), rtol=1e-13, atol=1e-13 * np.abs(P.U).max())
    dc, dp = P.direct(lam)
    sc, sp = P.schur_direct(lam)
    d = np.concatenate([dc.ravel(), dp.ravel()])
    s = np.concatenate([sc.ravel(), sp.ravel()])
    assert np.linalg.norm(s - d) <= 1e-9 * np.linalg.norm(d)
    res, g = P.damped_residual(lam, sc, sp)
    assert np.linalg.norm(res) <= 1e-10 * np.linalg.norm(g)
    # the model decrease of the reweighted problem is sum -w (2r + e).e
    e = np.einsum("nia,na->ni", args[1], sc[args[3]]) + np.einsum("nia,na->ni", args[2], sp[args[4]])
    want = float(np.sum(-w[:, None] * (2 * args[0].astype(LD) + e) * e))
    assert abs(float(P.model_decrease(sc, sp)) - want) <= 1e-11 * float(np.sum(w[:, None] * np.abs((2 * args[0] + e) * e)))


def test_kind_zero_is_the_unweighted_problem_bit_for_bit():
    args = _random(7)
    P0 = R.Problem(*args)
    for kind, a in ((0, 1.0), (None, 3.0), ("squared", 1e-3)):
        P = B.problem(kind, a, *args)
        for name in ("r", "Jc", "Jp", "U", "V", "gc", "gp", "W", "SU", "SV", "Sgc", "Sgp"):
            assert np.array_equal(getattr(P, name), getattr(P0, name)), name
        assert np.array_equal(np.asarray(B.cost(kind, a, args[0]), dtype=np.float64),
                              np.asarray(B._s(args[0]), dtype=np.float64))
        assert np.all(B.weights(kind, a, args[0]) == 1)
    for lam in (1e-4, 1.0):
        for x, y in zip(P0.schur_direct(lam), B.problem(0, 2.0, *args).schur_direct(lam)):
            assert np.array_equal(x, y)
