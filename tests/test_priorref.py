"""tests/_priorref.py on the CPU: the centre's Jacobian against mpmath's derivative of -exp([w]x)^T t at 60 digits, the
stacking helper against blocks built directly, zero weights, and the host Levenberg-Marquardt loop over the stacked
reference on a drifted grid -- the orderings tests/test_gpu_priors.py asserts of the device."""
import numpy as np

import _jacref as J
import _priorref as PRI
import _schurref as R
import _solvecheck as SC
from _problems import random_problem

LD = np.longdouble


def _center_mp(mp, w, t):
    """C = -exp([w]x)^T t by Rodrigues' formula in mpmath"""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = mp.sqrt(th2)
    a = mp.sin(th) / th if th != 0 else mp.mpf(1)
    b = (1 - mp.cos(th)) / th2 if th != 0 else mp.mpf(1) / 2
    K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Rm = mp.eye(3) + a * K + b * K * K
    return -(Rm.T * mp.matrix(t))


def test_center_jacobian_is_the_derivative_of_the_center():
    """dC/d(w, t) of center_jacobian_bal against mpmath.mp.diff of -exp([w]x)^T t at 60 digits, |w| from 1e-8 to beyond 2.1;
    entry by entry within CENTER_OPS eps_longdouble (|R^T| |[t]x| |J_l|) (the count is _priorref's docstring), the
    translation block within 78 eps_longdouble x the sum of R's absolute terms (_priorref.rotation_scale)."""
    from mpmath import mp
    mp.dps = 60
    rng = np.random.default_rng(5)
    mags = (1e-8, 1e-6, 1e-4, 1e-2, 0.0999, 0.1001, 0.5, 1.0, 2.0, 2.1, 2.2, 3.0)
    worst = 0.0
    for mag in mags:
        for _ in range(2):
            d = rng.normal(size=3)
            w = mag * d / np.linalg.norm(d)
            t = rng.normal(size=3) * 10.0 ** rng.uniform(-1, 2)
            Dw, Dt, Sw = PRI.center_jacobian_bal(w[None], t[None])
            x = [mp.mpf(float(v)) for v in np.concatenate([w, t])]
            for k in range(3):
                f = lambda *a, k=k: _center_mp(mp, a[:3], a[3:])[k]
                for j in range(6):
                    order = tuple(1 if i == j else 0 for i in range(6))
                    want = mp.diff(f, tuple(x), order)
                    if j < 3:
                        got, bound = Dw[0, k, j], PRI.CENTER_OPS * PRI.ELD * float(Sw[0, k, j])
                    else:
                        got, bound = Dt[0, k, j - 3], 78.0 * PRI.ELD * float(PRI.rotation_scale(w[None])[0, j - 3, k])
                    err = abs(float(mp.mpf(float(got)) + mp.mpf(float(got - LD(float(got)))) - want))
                    assert err <= bound, (mag, k, j, err, bound)
                    worst = max(worst, err / bound if bound > 0 else 0.0)
    print("PRIORREF centre Jacobian: worst |err| / bound %.3g over |w| in %s" % (worst, mags))


def _problem(seed=11):
    import oracle as O
    P = random_problem(12, 60, 8, seed=seed, noise=1e-3, empty_every=5)
    r, Jc, Jp = O.residual_jacobian_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    return P, r, Jc, Jp, SC.cam_of(P["row_ptr"]), P["pt_idx"].astype(np.int64)


def _priors(P, seed=3):
    """targets a seeded perturbation of the current values; weights spanning 1e-3 ... 1e3 with zeros, whole entities
    without priors and a prior on an empty-row camera"""
    rng = np.random.default_rng(seed)
    nc, npt = len(P["bal9"]), len(P["pts"])
    b9 = P["bal9"]
    Rm, Jl = J.exp_so3(b9[:, :3]), J.left_jacobian_ld(b9[:, :3])
    C = PRI.center(Rm, b9[:, 3:6]).astype(np.float64)
    cw = 10.0 ** rng.uniform(-3, 3, size=(nc, 3))
    cw[rng.random((nc, 3)) < 0.2] = 0.0
    cw[1::4] = 0.0
    iw = 10.0 ** rng.uniform(-3, 3, size=(nc, 3))
    iw[::3] = 0.0
    empty = np.flatnonzero(np.diff(P["row_ptr"].astype(np.int64)) == 0)
    assert len(empty)
    cw[empty[0]] = (1e3, 1e-3, 2.0)
    xw = 10.0 ** rng.uniform(-3, 3, size=(npt, 3))
    xw[rng.random(npt) < 0.7] = 0.0
    c0 = C + rng.normal(scale=0.05, size=C.shape)
    i0 = b9[:, 6:9] * (1 + rng.normal(scale=0.01, size=(nc, 3)))
    x0 = P["pts"] + rng.normal(scale=0.05, size=P["pts"].shape)
    c0[cw == 0] = np.nan                                          # a target under a zero weight may be anything
    x0[xw == 0] = np.inf
    cams = PRI.camera_rows(Rm, b9[:, 3:6], Jl, b9[:, 6:9], C, c0, cw, i0, iw)
    ptsr = PRI.point_rows(P["pts"], x0, xw)
    return dict(r_cam=cams["r"], A_cam=cams["A"], iw=iw, r_pt=ptsr["r"], xw=xw), (cw, iw, xw)


def test_stacked_dense_system_is_the_observations_plus_the_prior_blocks():
    import __graft_entry__ as entry
    entry.build()                                                # the oracle's library
    P, r, Jc, Jp, cam, pt = _problem()
    nc, npt = len(P["bal9"]), len(P["pts"])
    prior, (cw, iw, xw) = _priors(P)
    assert np.isfinite(prior["r_cam"].astype(np.float64)).all() and np.isfinite(prior["r_pt"].astype(np.float64)).all()
    assert (cw > 0).any(axis=1).sum() < nc and (xw > 0).any(axis=1).sum() < npt       # whole entities without priors
    span = np.concatenate([cw[cw > 0], iw[iw > 0], xw[xw > 0]])
    assert span.min() <= 1e-2 and span.max() >= 1e2
    Q0 = R.Problem(r, Jc, Jp, cam, pt, nc, npt)
    Q = PRI.stacked_problem(r, Jc, Jp, cam, pt, nc, npt, prior)
    _, H0, g0 = Q0.dense_H()
    _, H, g = Q.dense_H()
    Hp, gp = PRI.prior_blocks_direct(nc, npt, **prior)
    assert np.abs(Hp).sum() > 0 and np.abs(gp).sum() > 0
    assert np.allclose(H, H0 + Hp, rtol=1e-13, atol=1e-13 * np.abs(H0 + Hp).max())
    assert np.allclose(g, g0 + gp, rtol=1e-12, atol=1e-13 * np.abs(g0 + gp).max())
    # the diagonal blocks and the cost of the stack, through the references the GPU tests use
    B = PRI.stacked_blocks(r, Jc, Jp, cam, pt, nc, npt, prior)
    for c in range(nc):
        assert np.allclose(B["U"][c].astype(np.float64), (H0 + Hp)[9 * c:9 * c + 9, 9 * c:9 * c + 9], rtol=1e-12, atol=1e-300)
    cost = float(np.sum(Q0.r * Q0.r) + PRI.prior_cost(prior["r_cam"], prior["r_pt"]))
    assert abs(float(B["sum_sq"]) - cost) <= 1e-13 * cost
    # the priors couple nothing: W of every pseudo-observation is 0
    assert not Q.W[len(cam):].any()


def test_loss_weights_the_real_rows_only_and_a_mask_zeroes_prior_columns():
    import __graft_entry__ as entry
    entry.build()
    P, r, Jc, Jp, cam, pt = _problem(seed=12)
    nc, npt = len(P["bal9"]), len(P["pts"])
    prior, _ = _priors(P)
    a = 2.0 * float(np.median(np.linalg.norm(r.reshape(-1, 2), axis=1)))
    plain = PRI.stacked_problem(r, Jc, Jp, cam, pt, nc, npt, prior)
    robust = PRI.stacked_problem(r, Jc, Jp, cam, pt, nc, npt, prior, loss=("cauchy", a))
    n = len(cam)
    assert np.array_equal(plain.r[n:], robust.r[n:]) and np.array_equal(plain.Jc[n:], robust.Jc[n:])
    assert (np.abs(robust.r[:n]) <= np.abs(plain.r[:n])).all() and (np.abs(robust.r[:n]) < np.abs(plain.r[:n])).any()
    cm = np.zeros(nc, dtype=np.uint16)
    cm[2] = 0x1ff
    cm[3] = 0x038
    pm = np.zeros(npt, dtype=bool)
    pm[np.flatnonzero(prior["xw"].sum(axis=1) > 0)[0]] = True
    masked = PRI.stacked_problem(r, Jc, Jp, cam, pt, nc, npt, prior, mask=(cm, pm))
    assert not masked.U[2].any() and not masked.U[3][3:6].any() and not masked.U[3][:, 3:6].any() and not masked.V[pm].any()
    assert plain.U[3][3:6].any() and plain.V[pm].any()
    assert np.array_equal(masked.r, plain.r)                     # the cost keeps a constant parameter's prior


# ---- the drifted grid: what tests/test_gpu_priors.py::test_centre_priors_undo_a_drift asserts of the device ---------------
DRIFT = dict(strength=0.01, angle_strength=0.002, std=0.01, dir=[1.0, 0.5, 0.0], seed=4)
DRIFT_SIGMA, DRIFT_ITERATIONS, DRIFT_GRADIENT_TOL = 0.3, 40, 1e-3


def small_grid_culled_host():
    """test_gpu_schur_step's "small grid culled" without a device: the numpy layout, the oracle's visibility predicate, the
    host cull, the same observation noise.  Returns (cams15, pts, row_ptr, pt_idx, uv)."""
    import oracle as O
    from _problems import np_candidate_pairs, np_grid_layout
    from city2ba_amd.baproblem import cull_arrays
    cams, pts = np_grid_layout(2, cpb=5, ppb=2, block_length=5.0, block_inset=1.0, camera_height=1.0, point_height=1.0)
    ci, pi = np_candidate_pairs(O.centers(cams), pts, 10.0)
    uv, keep = O.visibility_pairs(cams, pts, ci, pi, 10.0)
    ci, pi, uv = ci[keep == 1], pi[keep == 1], uv[keep == 1]
    row_ptr = np.zeros(len(cams) + 1, dtype=np.int64)
    np.add.at(row_ptr, ci.astype(np.int64) + 1, 1)
    cams, pts, row_ptr, pt_idx, uv = cull_arrays(cams, pts, np.cumsum(row_ptr).astype(np.uint64), pi.astype(np.uint64), uv)
    return cams, pts, row_ptr, pt_idx, uv + np.random.default_rng(4).normal(scale=1e-2, size=uv.shape)


def test_centre_priors_undo_a_drift_on_the_host():
    """DRIFT on the small culled grid (100 cameras, 141 points), centre priors of sigma = DRIFT_SIGMA at the clean centres:
    the host loop over the stacked reference ends nearer the clean centres than it started and than the unanchored loop
    ends, and stops on the gradient tolerance of the stacked system.  Seen here: mean centre distance 0.838 at the start,
    0.845 after the unanchored loop (24 iterations), 7.8e-4 with the priors (5 iterations)."""
    import __graft_entry__ as entry
    entry.build()
    import oracle as O
    cams, pts, row_ptr, pt_idx, uv = small_grid_culled_host()
    assert len(cams) == 100 and len(pts) == 141
    clean = O.centers(cams)
    dcams, dpts = O.add_drift(cams, pts, DRIFT["strength"], DRIFT["angle_strength"], DRIFT["std"], DRIFT["dir"], DRIFT["seed"])
    b9 = O.camera_to_bal(dcams)

    def dist(b):
        C = PRI.center(J.exp_so3(b[:, :3]), b[:, 3:6]).astype(np.float64)
        return float(np.mean(np.linalg.norm(C - clean, axis=1)))

    start = dist(b9)
    free = PRI.host_lm(b9, dpts, row_ptr, pt_idx, uv, DRIFT_ITERATIONS, gradient_tol=DRIFT_GRADIENT_TOL)
    tied = PRI.host_lm(b9, dpts, row_ptr, pt_idx, uv, DRIFT_ITERATIONS, c0=clean, cw=1.0 / DRIFT_SIGMA, gradient_tol=DRIFT_GRADIENT_TOL)
    print("PRIORREF drift: start %.4g, unanchored %.4g after %d iterations, with priors %.4g after %d" % (
        start, dist(free["bal9"]), len(free["costs"]) - 1, dist(tied["bal9"]), len(tied["costs"]) - 1))
    assert dist(tied["bal9"]) < start and dist(tied["bal9"]) < dist(free["bal9"])
    assert tied["termination"] == 2 and tied["gradient_max"][-1] <= DRIFT_GRADIENT_TOL
    assert tied["costs"][-1] < tied["costs"][0]
