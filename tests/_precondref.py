"""Host reference of the Schur-Jacobi preconditioner on a tests/_schurref.py Problem: the blocks
  M_c = lam diag(d_c) + sum_o Jc_o^T (I2 - Jp_o V_l,p(o)^-1 Jp_o^T) Jc_o        (d_c the clamp rule on U_c's diagonal)
restated from that definition in the Problem's dtype (longdouble works), the diagonal blocks of S by S's own definition
to hold them against, and _schurref's PCG (pcg_loop, _LDOps and pcg's bounds) with the preconditioner as a parameter.
With rng every intermediate is moved by +-(its first-order absolute scale) * 2^-52: one plausible f64 evaluation, as
_schurref._LDOps does it.  _schurref.py itself is untouched.  numpy only."""
import numpy as np

import _schurref as R

LD, EPS = R.LD, R.EPS


def _jig(v, scale, rng):
    if rng is None:
        return v
    s = rng.choice(np.array([-1.0, 1.0]), size=np.shape(v)).astype(v.dtype)
    return v + s * np.asarray(scale, dtype=v.dtype) * v.dtype.type(EPS)


def _cam_sum(P, per_obs):
    out = np.zeros((P.n_cam,) + per_obs.shape[1:], dtype=per_obs.dtype)
    np.add.at(out, P.cam, per_obs)
    return out


def _damped_inverse(P, lam, rng=None):
    """V_l^-1 per point and the first-order bound of an explicit inverse's error, |V_l^-1| (SV + lam d) |V_l^-1|
    (delta(V^-1) = -V^-1 dV V^-1, with |dV| a few eps of the absolute-value sums that make V)"""
    V = _jig(P.V, P.SV, rng)
    Vl = R.damp(V, lam)
    SVl = P.SV + (Vl - V)
    if rng is not None:
        # a Cholesky solve is backward stable: what it applies is the exact inverse of V_l + dV, |dV| a few eps of
        # |L| |L^T| <= SVl, dV symmetric.  (Moving V_l^-1 itself entry by entry by |V_l^-1| SVl |V_l^-1| would be a bound
        # and not a plausible evaluation: Jp V_l^-1 Jp^T does not see V_l^-1's large component along Jp's null direction)
        dV = _jig(np.zeros_like(Vl), SVl, rng)
        Vl = Vl + (dV + dV.transpose(0, 2, 1)) / 2
    Vi = R.inv3(Vl)
    aVi = np.abs(Vi)
    return Vi, np.einsum("pab,pbc,pcd->pad", aVi, SVl, aVi)


def blocks(P, lam, rng=None):
    """(M [n_cam, 9, 9], SM): the definition, term by term in its positive semi-definite form, and the absolute-value
    scale of the sum (|Jc|^T (I2 + |Jp| |V_l^-1| |Jp|^T) |Jc| summed, plus the damping's own diagonal)"""
    Vi, SVi = _damped_inverse(P, lam, rng)
    Vo, aVo = Vi[P.pt], np.abs(Vi[P.pt])
    G = np.einsum("nia,nab,njb->nij", P.Jp, Vo, P.Jp)                      # Jp V_l^-1 Jp^T, 2x2 per observation
    SG = np.einsum("nia,nab,njb->nij", P.aJp, aVo, P.aJp)
    G = _jig(G, SG, rng)                                                   # (the solve's own error came with Vi)
    I2 = np.eye(2, dtype=P.dtype)
    F = I2 - G
    if rng is not None:                                                    # 1 - g rounds at the scale of 1 + |g|; F stays symmetric
        F = _jig(F, I2 + np.abs(G), rng)
        F = (F + F.transpose(0, 2, 1)) / 2
    # Jc^T F Jc and its sum round at the scale of their own products, |Jc|^T |F| |Jc| (F's error went in above, where
    # it is one 2x2 per observation and not 81 independent entries); the floor's scale SM is the coarser I2 + SG
    T = np.einsum("nia,nij,njb->nab", P.Jc, F, P.Jc)
    SR = np.einsum("nia,nij,njb->nab", P.aJc, np.abs(F), P.aJc)
    T = _jig(T, SR, rng)
    SM = _cam_sum(P, np.einsum("nia,nij,njb->nab", P.aJc, I2 + SG, P.aJc))
    M = _jig(_cam_sum(P, T), _cam_sum(P, SR), rng)
    i = np.arange(9)
    Ud = _jig(P.U[:, i, i], P.SU[:, i, i], rng)
    dl = lam * np.minimum(np.maximum(Ud, 1e-6), 1e32)
    M[:, i, i] += dl
    SM[:, i, i] += dl
    return M, SM


def blocks_bound(P, lam, runs=8, seed=0, mult=16.0, floor=1e-13):
    """The longdouble blocks and, per camera, the bound an f64 evaluation is held to in the Frobenius norm: `mult` x the
    largest deviation over `runs` seeded perturbed reruns, floored at `floor` x the norm of the absolute-value scale of
    the sum -- _schurref.pcg's rule.  Returns (M, bound [n_cam], SM)."""
    assert P.dtype == LD
    M, SM = blocks(P, lam)
    rng = np.random.default_rng(seed)
    dev = np.zeros(P.n_cam)
    for _ in range(runs):
        Mp, _ = blocks(P, lam, rng)
        dev = np.maximum(dev, np.linalg.norm((Mp - M).astype(np.float64), axis=(1, 2)))
    return M, np.maximum(mult * dev, floor * np.linalg.norm(SM.astype(np.float64), axis=(1, 2))), SM


def schur_diag_blocks(P, lam):
    """(D [n_cam, 9, 9], SD): the diagonal blocks of S = U_l - W V_l^-1 W^T by S's definition (Problem.dense_S's double
    loop restricted to c1 == c2, so a duplicated (camera, point) pair brings its cross terms) in P's dtype, and the
    absolute-value scale of that difference"""
    Vi, SVi = _damped_inverse(P, lam)
    Ul = P.Ul(lam)
    D, SD = Ul.copy(), P.SU + (Ul - P.U)
    aW = np.abs(P.W)
    key = P.cam * P.n_pts + P.pt
    order = np.argsort(key, kind="stable")
    start = np.flatnonzero(np.concatenate([[True], key[order][1:] != key[order][:-1]]))
    for a, b in zip(start, np.concatenate([start[1:], [len(order)]])):
        obs = order[a:b]
        c, p = P.cam[obs[0]], P.pt[obs[0]]
        Ws, aWs = P.W[obs].sum(axis=0), aW[obs].sum(axis=0)               # sum over o1, o2 = (sum W) Vi (sum W)^T
        D[c] -= Ws @ Vi[p] @ Ws.T
        SD[c] += aWs @ (np.abs(Vi[p]) + SVi[p]) @ aWs.T
    return D, SD


def has_duplicate_pairs(P):
    key = P.cam * P.n_pts + P.pt
    return len(np.unique(key)) != len(key)


def pivots(M):
    """the Cholesky pivots d_j of a stack of blocks (before the square root), NaN once one was not > 0"""
    with np.errstate(all="ignore"):
        L = R.chol_blocks(M)
    i = np.arange(M.shape[1])
    return L[:, i, i] ** 2


def _ops(P, lam, kind, rng=None):
    """_schurref's _LDOps with Minv / MScale of the chosen blocks; under rng the Schur-Jacobi blocks are themselves one
    perturbed evaluation"""
    if kind == "block_jacobi":
        return R._pcg_ops(P, lam, rng)
    assert kind == "schur_jacobi", kind
    M, _ = blocks(P, lam, rng)
    L = R.chol_blocks(M.astype(LD))
    Minv = R.chol_inverse(L)
    MScale = np.einsum("cij,cjk->cik", np.abs(Minv), np.einsum("cij,ckj->cik", np.abs(L), np.abs(L)))
    return R._LDOps(P, lam, Minv, MScale, rng)


def pcg_plain(P, lam, max_iters, rel_tol, kind="schur_jacobi"):
    """pcg_loop alone (no reruns): dict(xs, rs, rel, status, iterations, rel_residual)"""
    return R.pcg_loop(_ops(P, lam, kind), max_iters, rel_tol)


def pcg(P, lam, max_iters, rel_tol, kind="schur_jacobi", runs=8, seed=0, mult=16.0, floor=1e-13):
    """_schurref.pcg with the preconditioner as a parameter: the same iterates' quantities, the same seeded reruns, the
    same rule for the bounds (its text, with _ops in place of _pcg_ops)."""
    assert P.dtype == LD
    b, bscale = P.rhs(lam)
    base = R.pcg_loop(_ops(P, lam, kind), max_iters, rel_tol)

    def derived(res, rng=None):
        xs = res["xs"]
        dps = [P.back_substitute(lam, x) for x in xs]
        dps = [d if rng is None else R._LDOps(P, lam, None, None, rng)._jig(d, s) for d, s in dps]
        en = [-LD(0.5) * np.sum(x * (b + r)) for x, r in zip(xs, res["rs"])]
        return xs, dps, [LD(v) for v in res["rel"]], en

    xs, dps, rel, en = derived(base)
    n = len(xs)
    dev = dict(x=np.zeros(n), dp=np.zeros(n), rel=np.zeros(n), energy=np.zeros(n))
    rng = np.random.default_rng(seed)
    for _ in range(runs):
        res = R.pcg_loop(_ops(P, lam, kind, rng), max_iters, rel_tol)
        pxs, pdps, prel, pen = derived(res, rng)
        m = min(n, len(pxs))
        for k in range(m):
            dev["x"][k] = max(dev["x"][k], float(np.linalg.norm((pxs[k] - xs[k]).astype(np.float64))))
            dev["dp"][k] = max(dev["dp"][k], float(np.linalg.norm((pdps[k] - dps[k]).astype(np.float64))))
            dev["rel"][k] = max(dev["rel"][k], abs(float(prel[k] - rel[k])))
            dev["energy"][k] = max(dev["energy"][k], abs(float(pen[k] - en[k])))
    nx = np.array([float(np.linalg.norm(x.astype(np.float64))) for x in xs])
    ndp = np.array([float(np.linalg.norm(d.astype(np.float64))) for d in dps])
    escale = np.array([float(abs(e)) for e in en])
    bound = dict(x=np.maximum(mult * dev["x"], floor * nx), dp=np.maximum(mult * dev["dp"], floor * ndp),
                 rel=np.maximum(mult * dev["rel"], 4 * EPS), energy=np.maximum(mult * dev["energy"], floor * escale))
    return dict(x=xs, dp=dps, rel=rel, energy=en, bound=bound, deviation=dev, status=base["status"],
                iterations=base["iterations"], rel_residual=base["rel_residual"])


def issue_grid(num_blocks=2, max_dist=10.0, front=0.5, obs_noise=1e-3, state_noise=1e-2, seed=0, dtype=np.float64):
    """The grid the preconditioners were compared on: tests/_problems.py's layout, every pair within max_dist whose point
    lies at least `front` in front of its camera, observations of the true state + obs_noise, then the cameras' poses
    (w, t of the bal 9-vectors) and the points moved by state_noise; the oracle's bal-mode Jacobian.  2 blocks: 240 cameras, 720 points."""
    import oracle as O
    from _problems import grid_candidate_pairs, grid_cameras_points
    cams15, pts = grid_cameras_points(num_blocks)
    cam_idx, pt_idx = grid_candidate_pairs(cams15, pts, max_dist)
    Rm = cams15[cam_idx, :9].reshape(-1, 3, 3).transpose(0, 2, 1)        # column-major R: q = R X + t, looking down -z
    qz = np.einsum("nj,nj->n", Rm[:, 2, :], pts[pt_idx]) + cams15[cam_idx, 11]
    keep = qz <= -front
    cam_idx, pt_idx = cam_idx[keep].astype(np.int64), pt_idx[keep].astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_idx, minlength=len(cams15)))]).astype(np.uint64)
    rng = np.random.default_rng(seed)
    uv = O.project_observations(cams15, pts, row_ptr, pt_idx) + rng.normal(scale=obs_noise, size=(len(pt_idx), 2))
    bal9 = O.camera_to_bal(cams15)
    bal9[:, :6] += rng.normal(scale=state_noise, size=(len(cams15), 6))   # the pose; f, k1, k2 stay (|uv| reaches 18 here)
    pts = pts + rng.normal(scale=state_noise, size=pts.shape)
    r, Jc, Jp = O.residual_jacobian_bal(bal9, pts, row_ptr, pt_idx, uv)
    return R.Problem(r, Jc, Jp, cam_idx, pt_idx, len(cams15), len(pts), dtype=dtype)
