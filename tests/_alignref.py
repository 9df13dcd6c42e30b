"""The rules of the similarity alignment (include/city2ba_hip_experimental.h) restated in numpy long double -- test
helper, shared by tests/test_alignref.py (CPU) and tests/test_gpu_align.py.

Correspondences x_i (estimate) -> y_i (reference), a boolean mask `on`.  Means, centred moments and every error are taken in
np.longdouble from the f64 inputs; only the 3x3 singular value decomposition is numpy's, on the f64-rounded covariance.  R is
row-major [3, 3], y = s R x + t.  Camera records are cam15: R_c column-major in [0:9], t_c in [9:12], c = -R_c^T t_c."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
OK, TOO_FEW, DEGENERATE = 0, 1, 2
RANK_TOL = 1e-12

# the similarity every test moves a cloud by: s = 2.5, 2.1 rad about a general axis, t = (100, -40, 7)
S0, T0 = 2.5, np.array([100.0, -40.0, 7.0])


def rotation(axis, angle):
    """Rodrigues' formula in long double, rounded once"""
    a = np.asarray(axis, dtype=LD)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=LD)
    return (np.eye(3, dtype=LD) + np.sin(LD(angle)) * K + (1 - np.cos(LD(angle))) * (K @ K)).astype(np.float64)


R0 = rotation([0.3, -1.2, 0.8], 2.1)


def move(x, s=S0, R=R0, t=T0):
    """s R x + t in long double, rounded once"""
    return (LD(s) * (np.asarray(x, dtype=LD) @ np.asarray(R, dtype=LD).T) + np.asarray(t, dtype=LD)).astype(np.float64)


def centers(cams15):
    c = np.asarray(cams15, dtype=LD)
    Rm = c[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)          # row-major R_c
    return -np.einsum("nji,nj->ni", Rm, c[:, 9:12])             # -R_c^T t_c


def moments(x, y, on=None):
    """dict(n, mean_x, mean_y, sxx, syy, sxy [3, 3] (rows y, columns x): the CENTRED SUMS (not divided by n), and abs_*: the sums of the
    absolute values of the same terms (what a summation bound is relative to); abs_mean_*: sum |x| per coordinate"""
    x, y = np.asarray(x, dtype=LD).reshape(-1, 3), np.asarray(y, dtype=LD).reshape(-1, 3)
    if on is not None:
        x, y = x[np.asarray(on, dtype=bool)], y[np.asarray(on, dtype=bool)]
    n = len(x)
    if n == 0:
        z = np.zeros(3, dtype=LD)
        return dict(n=0, mean_x=z, mean_y=z, sxx=LD(0), syy=LD(0), sxy=np.zeros((3, 3), dtype=LD), abs_sxx=LD(0), abs_syy=LD(0),
                    abs_sxy=np.zeros((3, 3), dtype=LD), abs_mean_x=z, abs_mean_y=z)
    mx, my = x.sum(0) / n, y.sum(0) / n
    dx, dy = x - mx, y - my
    return dict(n=n, mean_x=mx, mean_y=my, sxx=(dx * dx).sum(), syy=(dy * dy).sum(), sxy=np.einsum("ni,nj->ij", dy, dx),
                abs_sxx=(dx * dx).sum(), abs_syy=(dy * dy).sum(), abs_sxy=np.einsum("ni,nj->ij", np.abs(dy), np.abs(dx)),
                abs_mean_x=np.abs(x).sum(0), abs_mean_y=np.abs(y).sum(0))


def fit_from_moments(n, mean_x, mean_y, var_x, cov, scale=True):
    """Umeyama's closed form: (status, s, R, t, sig, eps) with sig the singular values of cov and eps = det(U V^T)"""
    eye = (OK, 1.0, np.eye(3), np.zeros(3), np.zeros(3), 1.0)
    if n < 3:
        return (TOO_FEW,) + eye[1:]
    if not var_x > 0:
        return (DEGENERATE,) + eye[1:]
    Um, sig, Vt = np.linalg.svd(np.asarray(cov, dtype=np.float64))
    if not sig[1] > RANK_TOL * sig[0]:
        return (DEGENERATE,) + eye[1:]
    eps = 1.0 if np.linalg.det(Um) * np.linalg.det(Vt) > 0 else -1.0
    D = np.diag([1.0, 1.0, eps])
    R = (Um.astype(LD) @ D.astype(LD) @ Vt.astype(LD))
    s = LD((sig.astype(LD) * np.diag(D)).sum() / LD(var_x)) if scale else LD(1)
    t = np.asarray(mean_y, dtype=LD) - s * (R @ np.asarray(mean_x, dtype=LD))
    return OK, float(s), R.astype(np.float64), t.astype(np.float64), sig, eps


def fit(x, y, on=None, scale=True):
    m = moments(x, y, on)
    n = m["n"]
    if n == 0:
        return fit_from_moments(0, m["mean_x"], m["mean_y"], 0.0, np.zeros((3, 3)), scale)
    return fit_from_moments(n, m["mean_x"], m["mean_y"], m["sxx"] / n, (m["sxy"] / n).astype(np.float64), scale)


def fit_brute(x, y, scale=True):
    """the same minimiser restated without the closed form's means trick: Horn's quaternion method on the centred clouds (the largest
    eigenvector of the 4x4 matrix N of the cross-covariance), s = sum (y - my) . R (x - mx) / sum |x - mx|^2"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = x.mean(0), y.mean(0)
    dx, dy = x - mx, y - my
    M = dx.T @ dy                                               # sum x y^T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [M[1, 2] - M[2, 1], M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [M[2, 0] - M[0, 2], M[0, 1] + M[1, 0], -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [M[0, 1] - M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]]])
    w, v = np.linalg.eigh(N)
    q0, q1, q2, q3 = v[:, -1]
    R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                  [2 * (q2 * q1 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                  [2 * (q3 * q1 - q0 * q2), 2 * (q3 * q2 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
    s = float((dy * (dx @ R.T)).sum() / (dx * dx).sum()) if scale else 1.0
    return s, R, my - s * R @ mx


def rotation_bound(sig, eps, d_sigma_f):
    """|dR|_F <= 2 |dSigma|_F / (sig_2 + eps sig_3): the perturbation bound of the orthogonal polar factor"""
    return 2.0 * d_sigma_f / (sig[1] + eps * sig[2])


def fit_bounds(m, sig, eps, s, d_sigma_f, d_var_rel=0.0):
    """first-order bounds (dR_F, ds, |dt|) of a fit whose covariance cov = sxy / n is off by d_sigma_f (Frobenius) and whose var_x is off
    by d_var_rel (relative), with 8u of the closed form's own rounding on s and t: every singular value moves by at most |dSigma|_2,
    so tr(D S) by at most 3 |dSigma|_F; t = mu_y - s R mu_x"""
    n = m["n"]
    var_x = float(m["sxx"] / n)
    nmx, nmy = float(np.sqrt((m["mean_x"] ** 2).sum())), float(np.sqrt((m["mean_y"] ** 2).sum()))
    dR = rotation_bound(sig, eps, d_sigma_f)
    ds = 3.0 * d_sigma_f / var_x + abs(s) * (d_var_rel + 8 * U)
    dt = ds * nmx + abs(s) * dR * nmx + 8 * U * (nmy + abs(s) * nmx)
    return dR, ds, dt


def errors(x, y, s, R, t):
    """|s R x + t - y| per row, long double"""
    x, y = np.asarray(x, dtype=LD).reshape(-1, 3), np.asarray(y, dtype=LD).reshape(-1, 3)
    d = LD(s) * (x @ np.asarray(R, dtype=LD).T) + np.asarray(t, dtype=LD) - y
    return np.sqrt((d * d).sum(1))


def error_bound(x, y, s, t):
    """8u (s |x| + |t| + |y|): the rounding of s R x + t - y and of the norm, per row"""
    nx, ny = np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(1)), np.sqrt((np.asarray(y, dtype=np.float64) ** 2).sum(1))
    return 8 * U * (abs(s) * nx + float(np.sqrt((np.asarray(t) ** 2).sum())) + ny)


def rotation_errors(cams_x, cams_y, R):
    """theta_c = 2 asin(min(1, q)), q = |R_c R^T - R_c_ref|_F / (2 sqrt 2); returns (theta, q) in long double"""
    a = np.asarray(cams_x, dtype=LD)[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    b = np.asarray(cams_y, dtype=LD)[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    D = a @ np.asarray(R, dtype=LD).T - b
    q = np.sqrt((D * D).sum((1, 2))) / (2 * np.sqrt(LD(2)))
    return 2 * np.arcsin(np.minimum(LD(1), q)), q


def rotation_error_bound(q):
    """theta = 2 asin(min(1, q)) from entries of size <= 1 rounded in f64.  Each entry of R_c R^T - R_c_ref carries an absolute error of
    at most 4u (three products, two sums, one difference of numbers <= 1 in size), so |D|_F is off by at most 12u and q by
    dq = 12u / (2 sqrt 2) + 3u q (the norm, the scaling).  d theta = 2 dq / sqrt(1 - q^2) to first order; where 1 - q^2 < 4 dq (the
    derivative's pole at theta = pi) the exact form takes over: asin is monotone, so theta moves by at most
    2 (asin(min(1, q + dq)) - asin(max(0, q - dq))); the larger of the two is used, plus 4u theta for asin itself."""
    q = np.minimum(1.0, np.asarray(q, dtype=np.float64))
    dq = 12 * U / (2 * np.sqrt(2.0)) + 3 * U * q
    first = 2 * dq / np.sqrt(np.maximum(1 - q * q, 1e-300))
    exact = 2 * (np.arcsin(np.minimum(1.0, q + dq)) - np.arcsin(np.maximum(0.0, q - dq)))
    return np.where(1 - q * q < 4 * dq, exact, np.maximum(first, exact)) + 4 * U * 2 * np.arcsin(q)


def summary(e, on=None):
    """dict(n, sum_sq, sum, max, argmax) over the rows that are on (argmax: the lowest index attaining the maximum, -1 with nothing on)"""
    e = np.asarray(e, dtype=LD)
    on = np.ones(len(e), dtype=bool) if on is None else np.asarray(on, dtype=bool)
    if not on.any():
        return dict(n=0, sum_sq=LD(0), sum=LD(0), max=0.0, argmax=-1)
    idx = np.flatnonzero(on)
    k = idx[np.argmax(e[idx])]                                  # argmax returns the first maximum
    return dict(n=len(idx), sum_sq=(e[idx] ** 2).sum(), sum=e[idx].sum(), max=e[k], argmax=int(k))


def trim(x, y, max_dist, rounds, on=None, scale=True):
    """rule 5.  Returns dict(status, s, R, t, refits, sets): sets = the inlier set derived after every fit, in order; `final` = the set
    the summaries run over (the set the returned transform was fitted on; the set that failed on TOO_FEW / DEGENERATE)"""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1, 3), np.asarray(y, dtype=np.float64).reshape(-1, 3)
    base = np.ones(len(x), dtype=bool) if on is None else np.asarray(on, dtype=bool)
    st, s, R, t, _, _ = fit(x, y, base, scale)
    out = dict(status=st, s=s, R=R, t=t, refits=0, sets=[], final=base)
    if st != OK:
        return out
    cur = base
    for _ in range(rounds):
        nxt = base & (errors(x, y, out["s"], out["R"], out["t"]) <= max_dist)
        out["sets"].append(nxt)
        if np.array_equal(nxt, cur):
            break
        st, s, R, t, _, _ = fit(x, y, nxt, scale) if nxt.sum() >= 3 else (TOO_FEW, None, None, None, None, None)
        if st != OK:
            out.update(status=st, final=nxt)
            break
        cur = nxt
        out.update(s=s, R=R, t=t, refits=out["refits"] + 1, final=nxt)
    return out


def apply(cams15, pts, s, R, t):
    """rule 6 in long double, rounded once: (cams15', pts')"""
    c = np.asarray(cams15, dtype=LD)
    Rl, tl = np.asarray(R, dtype=LD), np.asarray(t, dtype=LD)
    Rc = c[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    ctr = LD(s) * (centers(cams15) @ Rl.T) + tl
    Rn = Rc @ Rl.T
    out = np.array(cams15, dtype=np.float64)
    out[:, :9] = Rn.transpose(0, 2, 1).reshape(-1, 9).astype(np.float64)
    out[:, 9:12] = (-np.einsum("nij,nj->ni", Rn, ctr)).astype(np.float64)
    return out, move(pts, s, R, t)


DOME_DISPLACED = (3, 17, 29, 44, 71)


def dome_trim_case(displace, seed=7):
    """the trimming case of the dome: x = the 81 true centres of dome_problem(seed=0) + N(0, 1e-3), the cameras DOME_DISPLACED moved by
    `displace` units along random directions; y = the similarity (S0, R0, T0) of the true centres.  Returns (x, y)."""
    from _problems import dome_problem
    import oracle as O
    c = centers(O.camera_from_bal(dome_problem(seed=0)["true_bal9"])).astype(np.float64)
    rng = np.random.default_rng(seed)
    x = c + rng.normal(scale=1e-3, size=c.shape)
    d = rng.normal(size=(len(DOME_DISPLACED), 3))
    x[list(DOME_DISPLACED)] += displace * d / np.linalg.norm(d, axis=1, keepdims=True)
    return x, move(c)
