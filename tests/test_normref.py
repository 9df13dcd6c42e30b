"""tests/_normref.py -- the reference of BAProblem.normal_equations -- against the dense J^T J / J^T r of tiny random
problems built from the full sparse Jacobian (CPU only)."""
import numpy as np
import pytest

import _normref as R


def _tiny(seed, n_cam, n_pts, n_obs):
    rng = np.random.default_rng(seed)
    cam_of = np.sort(rng.integers(0, n_cam, n_obs))
    cam_of[cam_of == 1] = 2                                  # camera 1 has an empty list
    pt_idx = rng.integers(0, n_pts - 1, n_obs)               # the last point is never observed
    r = rng.normal(size=(n_obs, 2))
    Jc = rng.normal(size=(n_obs, 2, 9)) * 10.0 ** rng.integers(-3, 3, size=(1, 1, 9))
    Jp = rng.normal(size=(n_obs, 2, 3))
    return r, Jc, Jp, cam_of, pt_idx


def _dense(r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts):
    n = len(cam_of)
    J = np.zeros((2 * n, 9 * n_cam + 3 * n_pts))
    for i in range(n):
        c, p = cam_of[i], pt_idx[i]
        J[2 * i:2 * i + 2, 9 * c:9 * c + 9] = Jc[i]
        J[2 * i:2 * i + 2, 9 * n_cam + 3 * p:9 * n_cam + 3 * p + 3] = Jp[i]
    return J.T @ J, J.T @ r.reshape(-1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_blocks_equal_the_diagonal_of_the_dense_normal_matrix(seed):
    n_cam, n_pts, n_obs = 6, 11, 40
    r, Jc, Jp, cam_of, pt_idx = _tiny(seed, n_cam, n_pts, n_obs)
    ref = R.blocks(r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts)
    H, g = _dense(r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts)
    tol = 1e-12 * max(1.0, float(np.max(np.abs(H))))
    for c in range(n_cam):
        np.testing.assert_allclose(ref["U"][c].astype(np.float64), H[9 * c:9 * c + 9, 9 * c:9 * c + 9], rtol=0, atol=tol)
        np.testing.assert_allclose(ref["gc"][c].astype(np.float64), g[9 * c:9 * c + 9], rtol=0, atol=tol)
    o = 9 * n_cam
    for p in range(n_pts):
        np.testing.assert_allclose(ref["V"][p].astype(np.float64), H[o + 3 * p:o + 3 * p + 3, o + 3 * p:o + 3 * p + 3], rtol=0, atol=tol)
        np.testing.assert_allclose(ref["gp"][p].astype(np.float64), g[o + 3 * p:o + 3 * p + 3], rtol=0, atol=tol)
    assert float(ref["sum_sq"]) == pytest.approx(float(r.reshape(-1) @ r.reshape(-1)), rel=1e-14)
    # the empty camera and the unobserved point: exact zeros, counts zero
    assert not ref["U"][1].any() and not ref["gc"][1].any() and ref["kc"][1] == 0
    assert not ref["V"][-1].any() and not ref["gp"][-1].any() and ref["kp"][-1] == 0
    assert ref["kc"].sum() == n_obs and ref["kp"].sum() == n_obs


def test_bound_holds_for_f64_sums_in_any_order_and_catches_a_wrong_block():
    n_cam, n_pts, n_obs = 5, 9, 60
    r, Jc, Jp, cam_of, pt_idx = _tiny(7, n_cam, n_pts, n_obs)
    ref = R.blocks(r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts)
    rng = np.random.default_rng(3)
    for _ in range(3):                                         # f64 sums in a shuffled order stay inside the bound
        perm = rng.permutation(n_obs)
        U = np.zeros((n_cam, 9, 9)); gc = np.zeros((n_cam, 9)); V = np.zeros((n_pts, 3, 3)); gp = np.zeros((n_pts, 3))
        for i in perm:
            c, p = cam_of[i], pt_idx[i]
            U[c] += Jc[i].T @ Jc[i]; gc[c] += Jc[i].T @ r[i]
            V[p] += Jp[i].T @ Jp[i]; gp[p] += Jp[i].T @ r[i]
        R.check((U, gc, V, gp), ref, "shuffled")
    bad = U.copy()
    bad[2, 0, 3] *= 1.0 + 1e-9                                 # far above rounding: rejected
    with pytest.raises(AssertionError):
        R.check((bad, gc, V, gp), ref, "perturbed")
    with pytest.raises(AssertionError):
        R.check((U, gc, V, -gp), ref, "sign")
