"""Host reference of linear midpoint triangulation (BAProblem.triangulate_points) in numpy.longdouble, and the
problems its CPU and GPU tests share.  numpy only: nothing here touches a device.

Per observation of camera c (cams15 row: R column-major 0..8, t 9..11, f, k1, k2; centre C given), observed (u, v):
m = (u, v) / f, rd = |m|, rho >= 0 with rho (1 + k1 rho^2 + k2 rho^4) = rd by Newton from rho = rd run to convergence
(k1 == k2 == 0: rho = rd), unusable when f is 0 or not finite, when the derivative 1 + 3 k1 rho^2 + 5 k2 rho^4 is <= 0 at
an iterate, or when rho is not finite; pn = m rho / rd (0 at rd == 0), d = R^T (pn.x, pn.y, -1) normalised;
A += I - d d^T, b += (I - d d^T) C.  Status (STATUS order): constant under the mask; n_used < 2; lambda_min(A) (eigvalsh)
< 1 - cos(min_angle), or a Cholesky pivot <= 0, or X = A^-1 b not finite; a usable observation's camera sees X at
q.z >= 0; else triangulated.

The bound on X is made as the bounds of tests/_schurref.py are (pcg): RUNS seeded reruns with uv, the camera records and
the centres moved by +-|value| 2^-52 and, as _schurref's reruns move every operator output by its first-order scale, the
two sums too: every entry of A and of b by +-(the sum of the magnitudes it is made of: |I| + |d||d|^T per ray for A,
|C| + |d| (|d| . |C|) for b) 2^-52, which is what six + three f64 accumulators round at.  (The inputs alone do not bound an f64 evaluation: a rounding of A of relative size 2^-52 moves X by
|X| 2^-52 / lambda_min(A), for rays half a degree apart 5e4 times the effect of the same rounding of an input.)  The bound
is MULT x the largest deviation of a point from the unperturbed run, floored at FLOOR x |X|; the constants are that
function's defaults."""
import numpy as np

import _schurref as R

LD = np.longdouble
EPS = R.EPS
RUNS, MULT, FLOOR = 8, 16.0, 1e-13                           # _schurref.pcg's runs, mult and floor
OK, TOO_FEW, DEGENERATE, BEHIND, CONSTANT = range(5)
STATUS = ("triangulated", "too_few", "degenerate", "behind", "constant")
CAP = 1e-6                                                   # no lambda_min within CAP (relative) of the threshold


def threshold(min_angle):
    """1 - cos(min_angle) in longdouble, min_angle in radians"""
    return LD(1) - np.cos(LD(min_angle))


def undistorted_pixels(f, k1, k2, uv):
    """(ray [n_obs, 3] longdouble, usable [n_obs] bool): every observed pixel's ray in its camera's frame, (m s, m s, -1)
    with m = uv / f and s = rho / |m| the undistortion (rho (1 + k1 rho^2 + k2 rho^4) = |m| by Newton), not normalised"""
    f, k1, k2 = (np.asarray(v).astype(LD) for v in (f, k1, k2))
    uv = np.asarray(uv).astype(LD).reshape(-1, 2)
    usable = (f != 0) & np.isfinite(f)
    with np.errstate(all="ignore"):
        m = uv / np.where(usable, f, LD(1))[:, None]
        rd = np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1])
        rho = rd.copy()
        active = usable & ((k1 != 0) | (k2 != 0))
        for _ in range(200):
            if not active.any():
                break
            r2 = rho * rho
            dg = 1 + 3 * k1 * r2 + 5 * k2 * r2 * r2
            bad = active & ~(dg > 0)
            usable &= ~bad
            active &= ~bad
            nxt = rho - (rho * (1 + k1 * r2 + k2 * r2 * r2) - rd) / np.where(dg > 0, dg, LD(1))
            done = active & ((np.abs(nxt - rho) <= 4 * np.finfo(LD).eps * np.abs(rho)) | ~np.isfinite(nxt))     # (a last-bit 2-cycle is convergence)
            rho = np.where(active, nxt, rho)
            active &= ~done
        assert not active.any(), "Newton did not converge"
        usable &= np.isfinite(rho)
        s = np.where(rd == 0, LD(0), rho / np.where(rd == 0, LD(1), rd))
        ray = np.stack([m[:, 0] * s, m[:, 1] * s, -np.ones(len(uv), dtype=LD)], axis=1)
    return ray, usable


def rays(cams15, uv, cam_of):
    """(d [n_obs, 3] longdouble, usable [n_obs] bool): the unit ray of every observation in the world frame"""
    cam = np.asarray(cams15).astype(LD)[cam_of]
    ray, usable = undistorted_pixels(cam[:, 12], cam[:, 13], cam[:, 14], uv)
    with np.errstate(all="ignore"):
        # cams15's R is column-major, Rm[i][j] = cam[3 j + i]; (R^T ray)_j = sum_i cam[3 j + i] ray_i
        d = np.stack([cam[:, 3 * j] * ray[:, 0] + cam[:, 3 * j + 1] * ray[:, 1] + cam[:, 3 * j + 2] * ray[:, 2] for j in range(3)], axis=1)
        d = d / np.sqrt(np.sum(d * d, axis=1))[:, None]
    return d, usable


def _solve(cams15, centers, row_ptr, pt_idx, uv, n_pts, thr, pt_mask, rng=None):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    cam_of = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    pt = np.asarray(pt_idx).astype(np.int64)
    d, usable = rays(cams15, uv, cam_of)
    C = np.asarray(centers).astype(LD)[cam_of]
    if pt_mask is not None:
        usable = usable & ~np.asarray(pt_mask, dtype=bool)[pt]               # a constant point reads nothing
    u = np.flatnonzero(usable)
    P = np.eye(3, dtype=LD)[None] - d[u, :, None] * d[u, None, :]
    A = np.zeros((n_pts, 3, 3), dtype=LD)
    b = np.zeros((n_pts, 3), dtype=LD)
    np.add.at(A, pt[u], P)
    np.add.at(b, pt[u], np.einsum("nij,nj->ni", P, C[u]))
    if rng is not None:                                          # one plausible f64 evaluation of the two sums
        SA = np.zeros_like(A)
        Sb = np.zeros_like(b)
        ad, aC = np.abs(d[u]), np.abs(C[u])                      # I - d d^T rounds at |I| + |d||d|^T, C - d (d . C) at |C| + |d| (|d| . |C|)
        np.add.at(SA, pt[u], np.eye(3, dtype=LD)[None] + ad[:, :, None] * ad[:, None, :])
        np.add.at(Sb, pt[u], aC + ad * np.sum(ad * aC, axis=1)[:, None])
        sa = np.triu(rng.choice(np.array([-1.0, 1.0]), size=A.shape))
        sa = sa + np.triu(sa, 1).transpose(0, 2, 1)               # A stays symmetric
        A = A + sa.astype(LD) * SA * LD(EPS)
        b = b + rng.choice(np.array([-1.0, 1.0]), size=b.shape).astype(LD) * Sb * LD(EPS)
    n_used = np.bincount(pt[u], minlength=n_pts)
    lam_min = np.linalg.eigvalsh(A.astype(np.float64))[:, 0]
    status = np.full(n_pts, TOO_FEW, dtype=np.uint8)
    X = np.full((n_pts, 3), np.nan, dtype=LD)
    cand = np.flatnonzero(n_used >= 2)
    status[cand] = DEGENERATE
    with np.errstate(all="ignore"):
        L = R.chol_blocks(A[cand])
        pivots = np.stack([L[:, k, k] for k in range(3)], axis=1)
        Xc = np.einsum("pij,pj->pi", R.inv3(A[cand]), b[cand])
    good = (lam_min[cand].astype(LD) >= thr) & np.all(pivots > 0, axis=1) & np.all(np.isfinite(Xc), axis=1)
    X[cand[good]] = Xc[good]
    status[cand[good]] = OK
    # cheirality: q.z = row 2 of R . X + t.z, for the usable observations of the points still in the running
    cam = np.asarray(cams15).astype(LD)[cam_of]
    sel = u[status[pt[u]] == OK]
    qz = cam[sel, 2] * X[pt[sel], 0] + cam[sel, 5] * X[pt[sel], 1] + cam[sel, 8] * X[pt[sel], 2] + cam[sel, 11]
    status[np.unique(pt[sel[qz >= 0]])] = BEHIND
    if pt_mask is not None:
        status[np.asarray(pt_mask, dtype=bool)] = CONSTANT
    return X, status, lam_min, n_used


def reference(cams15, centers, row_ptr, pt_idx, uv, n_pts, min_angle, pt_mask=None, bound=True, seed=0):
    """dict(X [n_pts, 3] longdouble (NaN where status != 0), status, lam_min, n_used, bound [n_pts], threshold);
    min_angle in radians"""
    thr = threshold(min_angle)
    cams15, centers, uv = (np.asarray(v, dtype=np.float64) for v in (cams15, centers, uv))
    X, status, lam_min, n_used = _solve(cams15, centers, row_ptr, pt_idx, uv, n_pts, thr, pt_mask)
    out = dict(X=X, status=status, lam_min=lam_min, n_used=n_used, threshold=thr, bound=None)
    if bound:
        rng = np.random.default_rng(seed)

        def jig(v):
            v = v.astype(LD)
            return v + rng.choice(np.array([-1.0, 1.0]), size=v.shape).astype(LD) * np.abs(v) * LD(EPS)
        dev = np.zeros(n_pts)
        ok = status == OK
        for _ in range(RUNS):
            Xp, sp, _, _ = _solve(jig(cams15), jig(centers), row_ptr, pt_idx, jig(uv), n_pts, thr, pt_mask, rng)
            both = ok & (sp == OK)
            dev[both] = np.maximum(dev[both], np.linalg.norm((Xp[both] - X[both]).astype(np.float64), axis=1))
            dev[ok & ~both] = np.inf                           # a status that rounding alone changes has no bound
        out["bound"] = np.where(ok, np.maximum(MULT * dev, FLOOR * np.linalg.norm(np.where(ok[:, None], X, 0).astype(np.float64), axis=1)), 0.0)
    return out


def cap_violations(ref):
    """points with at least two usable observations whose lambda_min lies within CAP (relative) of the threshold"""
    thr = float(ref["threshold"])
    return np.flatnonzero((ref["n_used"] >= 2) & (np.abs(ref["lam_min"] - thr) <= CAP * thr))


def centers_of(cams15):
    """the cameras' centres as the device's records hold them (the oracle's center() has the device's order)"""
    import oracle as O
    return O.centers(np.ascontiguousarray(cams15))


# ---- the problems -------------------------------------------------------------------------------------------------------
DOME_CASES = [(state, noise) for state in (False, True) for noise in (0.0, 1e-3)]
START = 0.5                                                  # every point starts this far from the truth


def dome_case(state, obs_noise):
    """tests/_problems.py's dome_problem with its true cameras, observations with obs_noise, and every point moved by
    exactly START in a seeded direction"""
    from _problems import dome_problem
    P = dict(dome_problem(seed=0, dup=True, state=state, obs_noise=obs_noise, start_noise=0.0))
    g = np.random.default_rng(17).normal(size=P["true_pts"].shape)
    P["pts"] = P["true_pts"] + START * g / np.linalg.norm(g, axis=1)[:, None]
    return P


def _cam(center, f=1.0, k1=0.0, k2=0.0):
    """a camera at `center` looking down -z with R = I: q = X - center"""
    c = np.asarray(center, dtype=np.float64)
    return np.concatenate([[1, 0, 0, 0, 1, 0, 0, 0, 1.0], -c, [f, k1, k2]])


def _project(cam, X):
    q = np.asarray(X, dtype=np.float64) + cam[9:12]
    p = -q[:2] / q[2]
    n = p @ p
    return cam[12] * (1 + cam[13] * n + cam[14] * n * n) * p


EDGE = dict(same_centre=6, half_degree=7, diverging=8, f_zero=9, k1_negative=10)     # point indices of the edge set


def edge_problem():
    """A small problem (four cameras over six points, every point seen by all four: status 0) with hand-placed cameras
    appended, each pair seeing one point of its own (EDGE):
      same_centre  two cameras with the same centre: the rays coincide, status 2;
      half_degree  two cameras whose rays to the point are 0.5 degrees apart: status 2 at 1 degree, 0 at 0.1;
      diverging    two cameras side by side looking down -z, the left one observing to its left, the right one to its
                   right: the lines meet behind both, status 3;
      f_zero       a good camera and one with f = 0, whose observation is skipped: status 1;
      k1_negative  a good camera and one with k1 = -50 observing at radius 0.2 (1 + 3 k1 rho^2 = -5 <= 0): status 1.
    Loaded in state mode (from_visibility).  Returns dict(cams15, pts, row_ptr, pt_idx, uv, bal=False)."""
    rng = np.random.default_rng(3)
    cams = [_cam([-3, -2, 10.0], 1.1, 1e-2, -2e-3), _cam([3, -2, 11.0], 0.9, -2e-2, 0.0), _cam([3, 2, 9.0]), _cam([-3, 2, 12.0], 1.0, 0.0, 1e-2)]
    pts = [list(v) for v in rng.uniform(-1.5, 1.5, size=(6, 3))]
    obs = [[(j, _project(c, pts[j])) for j in range(6)] for c in cams]

    def add(cam, p, uv=None):
        cams.append(cam)
        obs.append([(p, _project(cam, pts[p]) if uv is None else np.asarray(uv, dtype=np.float64))])
    pts.append([0.3, 0.2, 0.0])                                             # same_centre
    add(_cam([0, 0, 10.0]), 6)
    add(_cam([0, 0, 10.0], 1.2), 6)
    pts.append([1.0, 1.0, 0.0])                                             # half_degree
    add(_cam([1.0, 1.0, 10.0]), 7)
    add(_cam([1.0 + 10.0 * np.tan(np.deg2rad(0.5)), 1.0, 10.0]), 7)
    pts.append([0.0, 0.0, 0.0])                                             # diverging: the lines meet at (0, 0, 15)
    add(_cam([-1.0, 0, 10.0]), 8, uv=[-0.2, 0.0])
    add(_cam([1.0, 0, 10.0]), 8, uv=[0.2, 0.0])
    pts.append([-1.0, 0.5, 0.0])                                            # f_zero
    add(_cam([-2.0, 0, 10.0]), 9)
    add(_cam([2.0, 0, 10.0], 0.0), 9, uv=[0.1, 0.1])
    pts.append([0.5, -1.0, 0.0])                                            # k1_negative
    add(_cam([-2.0, 1.0, 10.0]), 10)
    add(_cam([2.0, 1.0, 10.0], 1.0, -50.0), 10, uv=[0.2, 0.0])
    pts = np.asarray(pts, dtype=np.float64)
    start = pts + np.random.default_rng(4).normal(scale=0.3, size=pts.shape)
    row_ptr = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.uint64)
    pt_idx = np.array([p for o in obs for p, _ in o], dtype=np.uint64)
    uv = np.array([v for o in obs for _, v in o], dtype=np.float64)
    return dict(cams15=np.ascontiguousarray(np.asarray(cams)), pts=start, true_pts=pts, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv, bal=False)


def edge_expected(min_angle_deg):
    """status per point of edge_problem at the default 1 degree and at 0.1"""
    s = np.zeros(11, dtype=np.uint8)
    s[EDGE["same_centre"]] = DEGENERATE
    s[EDGE["half_degree"]] = DEGENERATE if min_angle_deg > 0.5 else OK
    s[EDGE["diverging"]] = BEHIND
    s[EDGE["f_zero"]] = s[EDGE["k1_negative"]] = TOO_FEW
    return s


def counts_of(status):
    return dict(zip(STATUS, (int(v) for v in np.bincount(status, minlength=5))))


# ---- the end-to-end run: constant cameras, the points from a noisy start and from a triangulated one -------------------
# chosen with host_points_lm below on the same grid built with numpy and the oracle (DESIGN 4.9 has the figures); the GPU
# test asserts the ordering for the reference alone, on the problem itself, before it asks the device
E2E_POINT_STD = 3.0


def host_points_lm(P, iterations, lam=1e-4):
    """_solvecheck.host_lm's loop with every camera constant: the damped system is then block diagonal over the points,
    (V + lam D) dp = -gp, solved exactly point by point (inv3).  The same acceptance and damping update.  Returns the
    sums of squared residuals [iterations + 1] and the final points."""
    import oracle as O
    import _solvecheck as SC
    bal9, pts = P["bal9"], P["pts"].copy()
    n_cam, n_pts = len(bal9), len(pts)

    def lin(X):
        r, Jc, Jp = O.residual_jacobian_bal(bal9, X, P["row_ptr"], P["pt_idx"], P["uv"])
        return R.Problem(r, Jc, Jp, SC.cam_of(P["row_ptr"]), P["pt_idx"].astype(np.int64), n_cam, n_pts)

    Q = lin(pts)
    e0, nu, out = float(np.sum(Q.r * Q.r)), 2.0, []
    out.append(e0)
    dc = np.zeros((n_cam, 9))
    for _ in range(iterations):
        with np.errstate(all="ignore"):
            dp = -np.einsum("pab,pb->pa", R.inv3(Q.Vl(lam)), Q.gp)
        dp = np.where(np.isfinite(dp), dp, 0.0)
        Q1 = lin(pts + dp)
        e1 = float(np.sum(Q1.r * Q1.r))
        md = float(Q.model_decrease(dc, dp))
        rho = (e0 - e1) / md if md > 0.0 else -1.0
        if rho > 0.0 and e1 < e0:
            lam = min(max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e-20), 1e32)
            nu = 2.0
            pts, Q, e0 = pts + dp, Q1, e1
        else:
            lam = min(max(lam * nu, 1e-20), 1e32)
            nu *= 2.0
        out.append(e0)
    return out, pts
