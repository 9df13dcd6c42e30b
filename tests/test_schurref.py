"""The host reference of the damped step (tests/_schurref.py) checked against itself by other routes, on the CPU: the
Schur elimination against a dense solve of the whole damped system, the implicit S x against the dense S, and the
damping's clamp rule on empty blocks."""
import numpy as np
import pytest

import _schurref as R


def _random(seed, n_cam=12, n_pts=40, n_obs=160):
    """random r / Jc / Jp on a random list; cameras 0 and 5 and points 3 and 7 never observed, point 11 seen once"""
    rng = np.random.default_rng(seed)
    cams = np.setdiff1d(np.arange(n_cam), [0, 5])
    pts = np.setdiff1d(np.arange(n_pts), [3, 7, 11])
    cam_of = np.sort(rng.choice(cams, n_obs))
    pt_idx = rng.choice(pts, n_obs)
    pt_idx[rng.integers(n_obs)] = 11
    scale = np.array([1.0, 1.0, 1.0, 0.1, 0.1, 0.1, 1e-3, 10.0, 100.0])     # uneven columns, like f, k1, k2
    Jc = rng.normal(size=(n_obs, 2, 9)) * scale
    Jp = rng.normal(size=(n_obs, 2, 3))
    r = rng.normal(size=(n_obs, 2))
    return R.Problem(r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts)


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_schur_elimination_equals_the_dense_damped_solve(seed, lam):
    P = _random(seed)
    dc, dp = P.direct(lam)
    sc, sp = P.schur_direct(lam)
    d = np.concatenate([dc.ravel(), dp.ravel()])
    s = np.concatenate([sc.ravel(), sp.ravel()])
    assert np.linalg.norm(s - d) <= 1e-9 * np.linalg.norm(d)
    res, g = P.damped_residual(lam, sc, sp)
    assert np.linalg.norm(res) <= 1e-10 * np.linalg.norm(g)


@pytest.mark.parametrize("seed", [4, 5])
def test_implicit_operator_equals_the_dense_schur_complement(seed):
    P = _random(seed)
    L = R.Problem(P.r, P.Jc, P.Jp, P.cam, P.pt, P.n_cam, P.n_pts, dtype=R.LD)
    lam = 1e-2
    S = P.dense_S(lam)
    assert np.allclose(S, S.T, rtol=0, atol=1e-12 * np.abs(S).max())
    x = np.random.default_rng(seed).normal(size=(P.n_cam, 9))
    y, scale = L.S_times(lam, x)
    want = (S @ x.reshape(-1)).reshape(-1, 9)
    assert np.linalg.norm(np.asarray(y, dtype=np.float64) - want) <= 1e-12 * np.linalg.norm(np.asarray(scale, dtype=np.float64))
    # b by hand: -gc + sum_o W_o V_l^-1 gp
    b, _ = L.rhs(lam)
    Vi = R.inv3(P.Vl(lam))
    hand = -P.gc.copy()
    for o in range(len(P.cam)):
        hand[P.cam[o]] += P.W[o] @ (Vi[P.pt[o]] @ P.gp[P.pt[o]])
    assert np.allclose(np.asarray(b, dtype=np.float64), hand, rtol=1e-12, atol=1e-12 * np.abs(hand).max())


def test_clamp_rule_and_empty_blocks():
    d = np.array([0.0, 1e-9, 1e-6, 3.0, 1e40])
    assert np.array_equal(R.damp_diag(d, 0.5), d + 0.5 * np.array([1e-6, 1e-6, 1e-6, 3.0, 1e32]))
    A = np.zeros((2, 3, 3))
    A[1] = np.diag([4.0, 0.0, 1e33])
    Al = R.damp(A, 2.0)
    assert np.array_equal(Al[0], np.diag([2e-6] * 3))
    assert np.array_equal(np.diag(Al[1]), [12.0, 2e-6, 1e33 + 2e32]) and np.count_nonzero(Al[1] - np.diag(np.diag(Al[1]))) == 0
    P = _random(9)
    for lam in (1e-4, 1.0):
        dc, dp = P.schur_direct(lam)
        assert not dc[[0, 5]].any() and not dp[[3, 7]].any()
        assert dp[11].any()
        ddc, ddp = P.direct(lam)
        assert np.abs(ddc[[0, 5]]).max() <= 1e-300 and np.abs(ddp[[3, 7]]).max() <= 1e-300
    # a zero gradient: a zero step
    Z = R.Problem(np.zeros_like(P.r), P.Jc, P.Jp, P.cam, P.pt, P.n_cam, P.n_pts)
    zc, zp = Z.schur_direct(1e-3)
    assert not zc.any() and not zp.any()


def test_model_decrease_of_the_exact_step():
    """for the exact damped step, |r|^2 - |r + J d|^2 = -d^T g + lam d^T D d (> 0): the LM model the gain ratio divides by"""
    P = _random(6)
    lam = 0.3
    dc, dp = P.schur_direct(lam)
    md = float(P.model_decrease(dc, dp))
    _, H, g = P.dense_H()
    d = np.concatenate([dc.ravel(), dp.ravel()])
    i = np.arange(len(g))
    D = np.minimum(np.maximum(H[i, i], 1e-6), 1e32)
    want = -d @ g + lam * d @ (D * d)
    assert md > 0 and abs(md - want) <= 1e-9 * abs(want)
