"""Extended-precision reference of the priors on camera centres, intrinsics and points (BAProblem.set_priors),
numpy only: the prior residuals r_C = w_C o (C - C0), r_I = w_I o ((f, k1, k2) - I0), r_X = w_X o (X - X0), the centre's
Jacobian dC/dw = -R^T [t]x J_l(w), dC/dt = -R^T (C = -R^T t, left-Jacobian convention dR = [J_l dw]x R), and a stacking
helper that turns priors into pseudo-observations, so that tests/_normref.py, _schurref.py, _precondref.py, _robustref.py
and _solvecheck.py give blocks, S, M, iterates, sum_sq and model_decrease of the stacked system with the bounds they have.

center_jacobian evaluates, in np.longdouble, M = [t]x J_l entry by entry as a difference of two products and then -R^T M
as three products and two additions.  From R, t and J_l as given that is 2 + 3 = 5 roundings on an entry's longest path
(the negation is exact): |error| <= 5 eps_ld (|R^T| |[t]x| |J_l|) entry by entry, to first order.  When R = exp([w]x) and
J_l(w) come from _jacref.exp_so3 / left_jacobian_ld, each of their entries carries the roundings of that evaluation as
well: w.w (3 products, 2 additions: 5), a 32-term Horner series (32 products, 32 additions: 64), the entry of K^2 (3
products, 2 additions: 5), its product with the coefficient (1), the linear term's product (1) and the two additions
(2): 78 each.  Relative errors add to first order, so the whole evaluation from (w, t) is held to
    CENTER_OPS = 78 + 78 + 5 = 161,   |error| <= 161 eps_ld (|R^T| |[t]x| |J_l|)   entry by entry,
stated the way _normref states its (k + 4).  The translation block -R^T carries R's 78 alone, against the sum of R's
absolute terms (rotation_scale): an entry of R can be small where I + A K + B K^2 cancels, its rounding is not."""
import numpy as np

import _jacref as J
import _normref as N

LD = np.longdouble
ELD = float(np.finfo(LD).eps)
CENTER_OPS = 161.0
U53 = 2.0 ** -53
# the device's evaluation (city2ba_amd/csrc/prior_kernels.hpp states the count next to the kernel): six roundings on the
# longest path of an entry of diag(w_C) dC/dw from the record's R, t, J_l, one for an entry of diag(w_C) (-R^T), two for a
# residual; + 1 for the reference's own rounding to f64 where it is compared
DEVICE_OPS_DW, DEVICE_OPS_DT, DEVICE_OPS_R = 6.0 + 1.0, 1.0 + 1.0, 2.0 + 1.0


def _skew(t):
    t = np.asarray(t)
    K = np.zeros(t.shape[:1] + (3, 3), dtype=t.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -t[:, 2], t[:, 1], -t[:, 0]
    K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = t[:, 2], -t[:, 1], t[:, 0]
    return K


def center_jacobian(R, t, Jl):
    """R [n,3,3], t [n,3], J_l [n,3,3] (any float dtype; evaluated in longdouble) -> (Dw, Dt, Sw): dC/dw = -R^T [t]x J_l
    [n,3,3], dC/dt = -R^T [n,3,3] and the scale |R^T| |[t]x| |J_l| of Dw's rounding [n,3,3]"""
    R, t, Jl = np.asarray(R).astype(LD), np.asarray(t).astype(LD), np.asarray(Jl).astype(LD)
    K = _skew(t)
    M = np.einsum("nil,nlj->nij", K, Jl)
    Rt = np.transpose(R, (0, 2, 1))
    Dw = -np.einsum("nki,nij->nkj", Rt, M)
    Sw = np.einsum("nki,nij->nkj", np.abs(Rt), np.einsum("nil,nlj->nij", np.abs(K), np.abs(Jl)))
    return Dw, -Rt, Sw


def center(R, t):
    """C = -R^T t [n,3] (longdouble)"""
    return -np.einsum("nik,ni->nk", np.asarray(R).astype(LD), np.asarray(t).astype(LD))


def rotation_scale(w):
    """|I| + |A| |K| + |B| |K| |K| [n,3,3]: the sum of the absolute terms of exp([w]x) = I + A K + B K^2, the scale an entry
    of _jacref.exp_so3 rounds against (an entry of R itself can be small where its terms cancel)"""
    w = np.asarray(w, dtype=LD)
    A, B = J.rodrigues_coeffs((w * w).sum(axis=-1))[:2]
    K = np.abs(_skew(w))
    return np.eye(3, dtype=LD) + np.abs(A)[:, None, None] * K + np.abs(B)[:, None, None] * np.einsum("nij,njk->nik", K, K)


def center_jacobian_bal(w, t):
    """the same from the Rodrigues vector w [n,3] and t [n,3]: R = exp([w]x), J_l(w) of _jacref"""
    return center_jacobian(J.exp_so3(w), t, J.left_jacobian_ld(w))


def _w(a, n):
    return np.zeros((n, 3)) if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, 3)))


def camera_rows(R, t, Jl, intr, C, c0=None, cw=None, i0=None, iw=None):
    """The cameras' prior rows in longdouble from R, t, J_l, the intrinsics [n,3] and the centre C [n,3] (all as the device
    read them: device.camblk_records): dict(r [n,6], A [n,3,6] = diag(w_C) [dC/dw | -R^T], E_r [n,6], E_A [n,3,6]) --
    E the first-order bounds of the DEVICE's f64 evaluation (DEVICE_OPS_* x 2^-53 x the absolute-value scales).  A row of
    weight 0 is 0 whatever its target holds."""
    n = len(np.asarray(t))
    cw, iw = _w(cw, n), _w(iw, n)
    c0 = np.where(cw > 0, np.zeros((n, 3)) if c0 is None else np.asarray(c0, dtype=np.float64), 0.0)
    i0 = np.where(iw > 0, np.zeros((n, 3)) if i0 is None else np.asarray(i0, dtype=np.float64), 0.0)
    Dw, Dt, Sw = center_jacobian(R, t, Jl)
    wl = cw.astype(LD)
    A = np.concatenate([wl[:, :, None] * Dw, wl[:, :, None] * Dt], axis=2)
    dC, dI = np.asarray(C).astype(LD) - c0.astype(LD), np.asarray(intr).astype(LD) - i0.astype(LD)
    r = np.concatenate([wl * dC, iw.astype(LD) * dI], axis=1)
    E_A = np.concatenate([DEVICE_OPS_DW * U53 * cw[:, :, None] * Sw.astype(np.float64),
                          DEVICE_OPS_DT * U53 * np.abs((wl[:, :, None] * Dt).astype(np.float64))], axis=2)
    E_r = DEVICE_OPS_R * U53 * np.abs(r.astype(np.float64))
    return dict(r=r, A=A, E_r=E_r, E_A=E_A)


def camera_rows_from_records(rec, c0=None, cw=None, i0=None, iw=None):
    """camera_rows from camblk records [n, 32]: R row-major 0..8, t 9..11, intrinsics 12..14, J_l row-major 15..23, centre 24..26"""
    rec = np.asarray(rec, dtype=np.float64)
    return camera_rows(rec[:, 0:9].reshape(-1, 3, 3), rec[:, 9:12], rec[:, 15:24].reshape(-1, 3, 3), rec[:, 12:15], rec[:, 24:27],
                       c0, cw, i0, iw)


def point_rows(X, x0=None, xw=None):
    """dict(r [n,3] longdouble, E_r) of the points' prior rows"""
    X = np.asarray(X, dtype=np.float64)
    xw = _w(xw, len(X))
    x0 = np.where(xw > 0, np.zeros_like(X) if x0 is None else np.asarray(x0, dtype=np.float64), 0.0)
    r = xw.astype(LD) * (X.astype(LD) - x0.astype(LD))
    return dict(r=r, E_r=DEVICE_OPS_R * U53 * np.abs(r.astype(np.float64)))


def full_camera_jacobian(A, iw):
    """the 6x9 stack [n,6,9] of diag(w_C) [dC/dw | -R^T | 0] and [0 | 0 | diag(w_I)] from A [n,3,6] and w_I [n,3]"""
    A = np.asarray(A)
    n = len(A)
    out = np.zeros((n, 6, 9), dtype=A.dtype)
    out[:, :3, :6] = A
    iw = _w(iw, n)
    for m in range(3):
        out[:, 3 + m, 6 + m] = iw[:, m]
    return out


def _first_partner(idx, other, n):
    """per entity, the `other` index of its first observation, or 0"""
    out = np.zeros(n, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    seen = np.zeros(n, dtype=bool)
    for o in range(len(idx)):
        if not seen[idx[o]]:
            seen[idx[o]] = True
            out[idx[o]] = other[o]
    return out


def stack(r, Jc, Jp, cam, pt, n_cam, n_pts, r_cam=None, A_cam=None, iw=None, r_pt=None, xw=None):
    """The observations (r [n,2], Jc [n,2,9], Jp [n,2,3], cam, pt) with the priors appended as pseudo-observations of two
    rows: a camera's six rows (r_cam [n_cam,6], the 6x9 stack of A_cam [n_cam,3,6] and iw [n_cam,3]) as (0,1), (2, zeros),
    (3,4), (5, zeros) with Jp = 0; a point's three (r_pt [n_pts,3], Jp rows diag(xw)) as (0,1), (2, zeros) with Jc = 0.
    The other index is the entity's first observation's partner, or 0.  Only entities with a non-zero prior row are
    appended.  Returns (r, Jc, Jp, cam, pt) in float64 (the priors' values rounded to f64, as a device's would be)."""
    n = len(cam)
    r = np.asarray(r, dtype=np.float64).reshape(n, 2)
    Jc = np.asarray(Jc, dtype=np.float64).reshape(n, 2, 9)
    Jp = np.asarray(Jp, dtype=np.float64).reshape(n, 2, 3)
    cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
    rs, Jcs, Jps, cams, pts = [r], [Jc], [Jp], [cam], [pt]
    if r_cam is not None:
        rc = np.asarray(r_cam).astype(np.float64).reshape(n_cam, 6)
        A6 = full_camera_jacobian(np.zeros((n_cam, 3, 6)) if A_cam is None else np.asarray(A_cam).astype(np.float64), iw)
        on = np.flatnonzero(np.abs(A6).reshape(n_cam, -1).sum(axis=1) > 0)
        partner = _first_partner(cam, pt, n_cam)
        for a, b in ((0, 1), (2, None), (3, 4), (5, None)):
            rr, jj = np.zeros((len(on), 2)), np.zeros((len(on), 2, 9))
            rr[:, 0], jj[:, 0] = rc[on, a], A6[on, a]
            if b is not None:
                rr[:, 1], jj[:, 1] = rc[on, b], A6[on, b]
            rs.append(rr); Jcs.append(jj); Jps.append(np.zeros((len(on), 2, 3))); cams.append(on); pts.append(partner[on])
    if r_pt is not None:
        rp, w = np.asarray(r_pt).astype(np.float64).reshape(n_pts, 3), _w(xw, n_pts)
        on = np.flatnonzero(w.sum(axis=1) > 0)
        partner = _first_partner(pt, cam, n_pts)
        for a, b in ((0, 1), (2, None)):
            rr, jj = np.zeros((len(on), 2)), np.zeros((len(on), 2, 3))
            rr[:, 0], jj[:, 0, a] = rp[on, a], w[on, a]
            if b is not None:
                rr[:, 1], jj[:, 1, b] = rp[on, b], w[on, b]
            rs.append(rr); Jcs.append(np.zeros((len(on), 2, 9))); Jps.append(jj); cams.append(partner[on]); pts.append(on)
    return np.concatenate(rs), np.concatenate(Jcs), np.concatenate(Jps), np.concatenate(cams), np.concatenate(pts)


def stacked_problem(r, Jc, Jp, cam, pt, n_cam, n_pts, prior, loss=None, mask=None, dtype=np.float64):
    """_schurref.Problem of the stacked system.  prior = dict(r_cam, A_cam, iw, r_pt, xw) as stack takes them.  mask = (cm,
    pm): the constant columns zeroed in the observations' AND the priors' rows (_solvecheck.masked_jacobian on the stack).
    loss = (name, scale): the real rows weighted first, the unweighted prior rows stacked after (as _robustref.problem
    builds its Problem: the weighted entries round to f64 once)."""
    import _robustref as B
    import _schurref as R
    import _solvecheck as SC
    n = len(cam)
    if loss is not None:
        wr, wJc, wJp = B.reweighted(loss[0], loss[1], r, Jc, Jp)
        r, Jc, Jp = wr.astype(np.float64), wJc.astype(np.float64), wJp.astype(np.float64)
    sr, sJc, sJp, scam, spt = stack(r, Jc, Jp, cam, pt, n_cam, n_pts, **prior)
    if mask is not None:
        sJc, sJp = SC.masked_jacobian(sJc, sJp, scam, spt, *mask)
    assert len(scam) >= n
    return R.Problem(sr, sJc, sJp, scam, spt, n_cam, n_pts, dtype=dtype)


def stacked_blocks(r, Jc, Jp, cam, pt, n_cam, n_pts, prior):
    """_normref.blocks of the stacked system"""
    return N.blocks(*stack(r, Jc, Jp, cam, pt, n_cam, n_pts, **prior), n_cam, n_pts)


def prior_blocks_direct(n_cam, n_pts, r_cam=None, A_cam=None, iw=None, r_pt=None, xw=None):
    """(H_prior, g_prior) dense, cameras first then points, built directly: A6^T A6 and A6^T r per camera, diag(w_X^2) and
    w_X o r_X per point"""
    m = 9 * n_cam + 3 * n_pts
    H, g = np.zeros((m, m)), np.zeros(m)
    if r_cam is not None:
        A6 = full_camera_jacobian(np.asarray(A_cam).astype(np.float64), iw)
        rc = np.asarray(r_cam).astype(np.float64)
        for c in range(n_cam):
            H[9 * c:9 * c + 9, 9 * c:9 * c + 9] += A6[c].T @ A6[c]
            g[9 * c:9 * c + 9] += A6[c].T @ rc[c]
    if r_pt is not None:
        w, rp = _w(xw, n_pts), np.asarray(r_pt).astype(np.float64)
        for p in range(n_pts):
            o = 9 * n_cam + 3 * p
            H[o:o + 3, o:o + 3] += np.diag(w[p] ** 2)
            g[o:o + 3] += w[p] * rp[p]
    return H, g


def prior_cost(r_cam=None, r_pt=None):
    """sum |r_prior|^2 (longdouble) and its absolute-value sum (the same here: every term is a square)"""
    s = LD(0)
    for a in (r_cam, r_pt):
        if a is not None:
            a = np.asarray(a).astype(LD)
            s = s + np.sum(a * a)
    return s


def host_lm(bal9, pts, row_ptr, pt_idx, uv, iterations, lam=1e-4, c0=None, cw=None, gradient_tol=0.0):
    """city2ba_amd.solve.levenberg_marquardt's loop on the host in bal mode over the STACKED reference (_solvecheck.host_lm
    is the model): the oracle's Jacobian, centre priors (c0, cw) evaluated by this module from exp([w]x) and J_l(w), the
    step by a dense direct solve of the damped stacked system, the same acceptance and damping update, and the device
    loop's gradient test (max |g| <= gradient_tol at the state a step is solved at).  Returns dict(costs, bal9, pts,
    termination, gradient_max)."""
    import oracle as O
    import _schurref as R
    import _solvecheck as SC
    bal9, pts = np.array(bal9, dtype=np.float64), np.array(pts, dtype=np.float64)
    n_cam, n_pts = len(bal9), len(pts)
    cam, pt = SC.cam_of(row_ptr), np.asarray(pt_idx).astype(np.int64)

    def lin(b9, X):
        r, Jc, Jp = O.residual_jacobian_bal(b9, X, row_ptr, pt_idx, uv)
        prior = {}
        if cw is not None:
            Rm, Jl = J.exp_so3(b9[:, :3]), J.left_jacobian_ld(b9[:, :3])
            rows = camera_rows(Rm, b9[:, 3:6], Jl, b9[:, 6:9], center(Rm, b9[:, 3:6]), c0, cw)
            prior = dict(r_cam=rows["r"], A_cam=rows["A"])
        return stacked_problem(r, Jc, Jp, cam, pt, n_cam, n_pts, prior)

    Q = lin(bal9, pts)
    e0, nu = float(np.sum(Q.r * Q.r)), 2.0
    costs, termination, gmax = [e0], 0, []
    for _ in range(iterations):
        _, _, g = Q.dense_H()
        gmax.append(float(np.max(np.abs(g))))
        if gradient_tol > 0.0 and gmax[-1] <= gradient_tol:
            termination = 2
            break
        dc, dp = Q.direct(lam)
        Q1 = lin(bal9 + dc, pts + dp)
        e1 = float(np.sum(Q1.r * Q1.r))
        md = float(Q.model_decrease(dc, dp))
        rho = (e0 - e1) / md if md > 0.0 else -1.0
        if rho > 0.0 and e1 < e0:
            lam = min(max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e-20), 1e32)
            nu = 2.0
            bal9, pts, Q, e0 = bal9 + dc, pts + dp, Q1, e1
        else:
            lam = min(max(lam * nu, 1e-20), 1e32)
            nu *= 2.0
        costs.append(e0)
    return dict(costs=costs, bal9=bal9, pts=pts, termination=termination, gradient_max=gmax)
