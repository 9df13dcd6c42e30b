"""Host reference of camera resection (BAProblem.resect_cameras) in numpy.longdouble, and the problems its
CPU and GPU tests share.  numpy only: nothing here touches a device.

Per camera, f, k1, k2 as they are (cams15 entries 12..14).  Per observation of point X, observed (u, v): m = (u, v) / f,
rd = |m|, rho >= 0 with rho (1 + k1 rho^2 + k2 rho^4) = rd by Newton from rho = rd run to convergence (k1 == k2 == 0:
rho = rd), unusable when f is 0 or not finite, when the derivative 1 + 3 k1 rho^2 + 5 k2 rho^4 is <= 0 at an iterate, when
rho is not finite, or when X is not finite; pn = m rho / rd (0 at rd == 0), b = (pn.x, pn.y, -1) normalised, P = I - b b^T.
Xbar = the mean of the usable points, Y = X - Xbar; the sixty sums S[m][e] of the ten monomials 1, Y_a, Y_a Y_c times the
six entries of P; S0, S1[a], S2[ac] from them; M[(a,i),(c,j)] = S2[ac][ij] - (S1[a] S0^-1 S1[c])_ij; its eigenpairs by a
cyclic Jacobi of this module (numpy.linalg takes no longdouble); G from the eigenvector of lambda_1, negated if det G < 0;
R0 = G (G^T G)^-1/2 with the inverse square root from the same Jacobi; Gauss-Newton on r^T M r over R <- exp([d]x) R until
|d| <= 1e-30 or 50 iterations; t = -S0^-1 sum_a S1[a] R[:, a] - R Xbar.  Status (STATUS order): constant under the mask's
pose bits; n_used < min_points; a Cholesky pivot of S0 not > 0, an eigenvalue not finite, lambda_2 < min_gap lambda_9,
lambda_1 >= lambda_2 / 4, H not positive definite or a step, R or t not finite; a usable observation with (R X + t).z >= 0;
else resected.

The bounds on R and t are made as the bounds of tests/_triangref.py and tests/_schurref.py (pcg) are: RUNS seeded reruns
with uv, the intrinsics and the points moved by +-|value| 2^-52, every one of the sixty sums moved by +-(the sum of the
magnitudes it is made of) 2^-52, and every entry of M moved by +-2^-52 times the magnitudes of its two terms (the
subtraction cancels: the inputs and the sums alone do not bound an f64 evaluation of it).  The sensitivity of the
eigenvector and of the minimiser to those roundings then enters by construction.  The bound is MULT x the largest
deviation from the unperturbed run (R entry by entry, t in norm), floored at FLOOR (R) and FLOOR |t| (t)."""
import numpy as np

import _schurref as R_
import _triangref as T_

LD = np.longdouble
EPS = R_.EPS
RUNS, MULT, FLOOR = 8, 16.0, 1e-13                           # _schurref.pcg's runs, mult and floor
OK, TOO_FEW, DEGENERATE, BEHIND, CONSTANT = range(5)
STATUS = ("resected", "too_few", "degenerate", "behind", "constant")
CAP = 1e-6                                                   # no decision within CAP (relative) of its threshold
POSE_BITS = 0x03f
MIN_POINTS, MIN_GAP = 6, 1e-4                                # the defaults of BAProblem.resect_cameras
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # the order of a symmetric 3x3's six entries


def jacobi_eigh(A, sweeps=40):
    """eigenvalues [n, k] (unsorted) and eigenvectors (columns) [n, k, k] of a stack of symmetric matrices, by cyclic
    Jacobi in A's dtype"""
    A = np.array(A, copy=True)
    n, k, _ = A.shape
    V = np.broadcast_to(np.eye(k, dtype=A.dtype), A.shape).copy()
    tiny = np.finfo(A.dtype).eps ** 2
    off = ~np.eye(k, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            rest = np.sqrt(np.sum(np.where(off, A * A, 0), axis=(1, 2)))
            if np.all(~(rest > tiny * np.sqrt(np.sum(A * A, axis=(1, 2))))):
                break
            for p in range(k - 1):
                for q in range(p + 1, k):
                    apq = A[:, p, q]
                    nz = apq != 0
                    theta = (A[:, q, q] - A[:, p, p]) / (2 * np.where(nz, apq, 1))
                    t = np.where(theta < 0, -1, 1) / (np.abs(theta) + np.sqrt(theta * theta + 1))
                    t = np.where(nz, t, 0).astype(A.dtype)
                    c = (1 / np.sqrt(t * t + 1))[:, None]
                    s = t[:, None] * c
                    for Z, cols in ((A, True), (A, False), (V, True)):
                        if cols:
                            zp, zq = Z[:, :, p].copy(), Z[:, :, q].copy()
                            Z[:, :, p], Z[:, :, q] = c * zp - s * zq, s * zp + c * zq
                        else:
                            zp, zq = Z[:, p, :].copy(), Z[:, q, :].copy()
                            Z[:, p, :], Z[:, q, :] = c * zp - s * zq, s * zp + c * zq
    return np.stack([A[:, i, i] for i in range(k)], axis=1), V


def pixel_rays(intr, uv, cam_of):
    """(b [n_obs, 3] longdouble, usable [n_obs] bool): the unit ray of every observed pixel in its camera's frame"""
    intr = np.asarray(intr).astype(LD)[cam_of]
    b, usable = T_.undistorted_pixels(intr[:, 0], intr[:, 1], intr[:, 2], uv)
    with np.errstate(all="ignore"):
        b = b / np.sqrt(np.sum(b * b, axis=1))[:, None]
    return b, usable


def _sym_signs(rng, shape):
    """+-1 of a stack of square matrices, symmetric"""
    s = np.triu(rng.choice(np.array([-1.0, 1.0]), size=shape))
    return (s + np.triu(s, 1).swapaxes(-1, -2)).astype(LD)


def _expand(S):
    """S [n, 10, 6] -> S0 [n, 3, 3], S1 [n, 3(a), 3, 3], S2 [n, 3(a), 3(c), 3, 3]"""
    n = len(S)
    full = np.zeros((n, 10, 3, 3), dtype=S.dtype)
    for e, (i, j) in enumerate(SYM):
        full[:, :, i, j] = S[:, :, e]
        full[:, :, j, i] = S[:, :, e]
    S2 = np.zeros((n, 3, 3, 3, 3), dtype=S.dtype)
    for m, (a, c) in enumerate(SYM):
        S2[:, a, c] = full[:, 4 + m]
        S2[:, c, a] = full[:, 4 + m]
    return full[:, 0], full[:, 1:4], S2


def _exp_so3(d):
    """exp([d]x) of a stack of 3-vectors, in their dtype"""
    th2 = np.sum(d * d, axis=1)
    th = np.sqrt(th2)
    small = th < 1e-8
    ths = np.where(small, 1, th)
    a = np.where(small, 1 - th2 / 6, np.sin(ths) / ths)
    h = np.sin(ths / 2) / ths
    b = np.where(small, 0.5 - th2 / 24, 2 * h * h)
    K = np.zeros((len(d), 3, 3), dtype=d.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    return np.eye(3, dtype=d.dtype)[None] + a[:, None, None] * K + b[:, None, None] * np.einsum("nij,njk->nik", K, K)


CROSS = np.zeros((3, 3, 3))                                    # CROSS[k] = [e_k]x
CROSS[0, 1, 2], CROSS[0, 2, 1], CROSS[1, 0, 2], CROSS[1, 2, 0], CROSS[2, 0, 1], CROSS[2, 1, 0] = -1, 1, 1, -1, -1, 1


def _vec(Rm):
    """r[3 a + i] = R[i][a]"""
    return Rm.swapaxes(-1, -2).reshape(Rm.shape[:-2] + (9,))


def _jac(Rm):
    """J [n, 9, 3]: column k = vec([e_k]x R)"""
    return np.stack([_vec(np.einsum("ij,njk->nik", CROSS[k].astype(Rm.dtype), Rm)) for k in range(3)], axis=2)


def _form(M, Rm):
    r = _vec(Rm)
    return np.einsum("ni,nij,nj->n", r, M, r)


def _solve(intr, pts, row_ptr, pt_idx, uv, min_points, min_gap, cam_mask, rng=None, gn_iters=50, gn_tol=1e-30):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_cam = len(row_ptr) - 1
    cam_of = np.repeat(np.arange(n_cam), np.diff(row_ptr))
    pt = np.asarray(pt_idx).astype(np.int64)
    b, usable = pixel_rays(intr, uv, cam_of)
    X = np.asarray(pts).astype(LD)[pt]
    usable = usable & np.all(np.isfinite(X), axis=1)
    constant = np.zeros(n_cam, dtype=bool) if cam_mask is None else (np.asarray(cam_mask).astype(np.int64) & POSE_BITS) != 0
    usable = usable & ~constant[cam_of]                          # a constant camera reads nothing
    u = np.flatnonzero(usable)
    cu = cam_of[u]
    n_used = np.bincount(cu, minlength=n_cam)
    status = np.full(n_cam, TOO_FEW, dtype=np.uint8)
    cand = n_used >= min_points
    status[cand] = DEGENERATE
    nn = np.maximum(n_used, 1).astype(LD)
    Xbar = np.zeros((n_cam, 3), dtype=LD)
    np.add.at(Xbar, cu, X[u])
    Xbar = Xbar / nn[:, None]
    Y = X[u] - Xbar[cu]
    bu = b[u]
    mono = np.stack([np.ones(len(u), dtype=LD), Y[:, 0], Y[:, 1], Y[:, 2]] + [Y[:, a] * Y[:, c] for a, c in SYM], axis=1)
    ent = np.stack([(1 if i == j else 0) - bu[:, i] * bu[:, j] for i, j in SYM], axis=1)
    S = np.zeros((n_cam, 10, 6), dtype=LD)
    np.add.at(S, cu, mono[:, :, None] * ent[:, None, :])
    if rng is not None:                                          # one plausible f64 evaluation of the sixty sums
        mag = np.zeros_like(S)
        aent = np.stack([(1 if i == j else 0) + np.abs(bu[:, i] * bu[:, j]) for i, j in SYM], axis=1)
        np.add.at(mag, cu, np.abs(mono)[:, :, None] * aent[:, None, :])
        S = S + rng.choice(np.array([-1.0, 1.0]), size=S.shape).astype(LD) * mag * LD(EPS)
    S0, S1, S2 = _expand(S)
    out = dict(R=np.full((n_cam, 3, 3), np.nan, dtype=LD), t=np.full((n_cam, 3), np.nan, dtype=LD), n_used=n_used,
               lam1=np.full(n_cam, np.nan), lam2=np.full(n_cam, np.nan), lam9=np.full(n_cam, np.nan),
               form_start=np.full(n_cam, np.nan), form_end=np.full(n_cam, np.nan))
    with np.errstate(all="ignore"):
        L = R_.chol_blocks(np.where(cand[:, None, None], S0, np.eye(3, dtype=LD)[None]))
        cand = cand & np.all(np.stack([L[:, k, k] for k in range(3)], axis=1) > 0, axis=1)
    k = np.flatnonzero(cand)
    if len(k):
        S0, S1, S2, Xb = S0[k], S1[k], S2[k], Xbar[k]
        Si = R_.inv3(S0)
        T2 = np.einsum("naik,nkl,nclj->naicj", S1, Si, S1)
        first = S2.transpose(0, 1, 3, 2, 4)                      # [n, a, i, c, j]
        M = (first - T2).reshape(len(k), 9, 9)
        if rng is not None:                                      # and of the subtraction, which cancels
            aT2 = np.einsum("naik,nkl,nclj->naicj", np.abs(S1), np.abs(Si), np.abs(S1))
            M = M + _sym_signs(rng, M.shape) * (np.abs(first) + aT2).reshape(len(k), 9, 9) * LD(EPS)
        M = (M + M.swapaxes(1, 2)) / 2
        lam, V = jacobi_eigh(M)
        order = np.argsort(lam.astype(np.float64), axis=1)
        ar = np.arange(len(k))
        l1, l2, l9 = lam[ar, order[:, 0]], lam[ar, order[:, 1]], lam[ar, order[:, -1]]
        out["lam1"][k], out["lam2"][k], out["lam9"][k] = l1.astype(np.float64), l2.astype(np.float64), l9.astype(np.float64)
        with np.errstate(all="ignore"):
            good = np.all(np.isfinite(lam), axis=1) & ~(l2 < LD(min_gap) * l9) & ~(l1 >= l2 / 4)
            g = V[ar, :, order[:, 0]]
            G = g.reshape(len(k), 3, 3).swapaxes(1, 2)           # G[i][a] = g[3 a + i]
            G = np.where((np.linalg.det(G.astype(np.float64)) < 0)[:, None, None], -G, G)
            w, Wv = jacobi_eigh(np.einsum("nki,nkj->nij", G, G))
            Rm = np.einsum("nij,njk,nk,nlk->nil", G, Wv, 1 / np.sqrt(w), Wv)
            start = _form(M, Rm)
            live = good.copy()
            for _ in range(gn_iters):
                if not live.any():
                    break
                J = _jac(Rm)
                H = np.einsum("nia,nij,njb->nab", J, M, J)
                gr = np.einsum("nia,nij,nj->na", J, M, _vec(Rm))
                Lh = R_.chol_blocks(H)
                pd = np.all(np.stack([Lh[:, q, q] for q in range(3)], axis=1) > 0, axis=1)
                d = -np.einsum("nab,nb->na", R_.inv3(H), gr)
                fin = np.all(np.isfinite(d), axis=1)
                good &= ~(live & ~(pd & fin))
                live &= pd & fin
                d = np.where(live[:, None], d, 0)
                Rm = np.einsum("nij,njk->nik", _exp_so3(d), Rm)
                live &= np.sqrt(np.sum(d * d, axis=1)) > gn_tol
            v = np.einsum("naik,nka->ni", S1, Rm)                 # sum_a S1[a] R[:, a]
            t = -np.einsum("nij,nj->ni", Si, v) - np.einsum("nij,nj->ni", Rm, Xb)
            good &= np.all(np.isfinite(Rm), axis=(1, 2)) & np.all(np.isfinite(t), axis=1)
        kk = k[good]
        out["R"][kk], out["t"][kk] = Rm[good], t[good]
        out["form_start"][kk], out["form_end"][kk] = start[good].astype(np.float64), _form(M, Rm)[good].astype(np.float64)
        status[kk] = OK
        # cheirality: (R X + t).z of the usable observations of the cameras still in the running
        sel = np.flatnonzero(status[cu] == OK)
        cs = cu[sel]
        qz = np.einsum("nj,nj->n", out["R"][cs, 2, :], X[u][sel]) + out["t"][cs, 2]
        status[np.unique(cs[qz >= 0])] = BEHIND
    status[constant] = CONSTANT
    out["status"] = status
    return out


def reference(cams15, pts, row_ptr, pt_idx, uv, min_points=MIN_POINTS, min_gap=MIN_GAP, cam_mask=None, bound=True, seed=0):
    """dict(R [n_cam, 3, 3] and t [n_cam, 3] longdouble (q = R X + t; NaN where status != 0), status, lam1, lam2, lam9,
    n_used, form_start, form_end (r^T M r at R0 and at the end), bound_R, bound_t [n_cam], min_gap, min_points)"""
    intr = np.asarray(cams15, dtype=np.float64)[:, 12:15]
    pts, uv = np.asarray(pts, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    out = _solve(intr, pts, row_ptr, pt_idx, uv, min_points, min_gap, cam_mask)
    out.update(min_gap=min_gap, min_points=min_points, bound_R=None, bound_t=None)
    if bound:
        rng = np.random.default_rng(seed)

        def jig(v):
            v = v.astype(LD)
            with np.errstate(invalid="ignore"):
                return v + rng.choice(np.array([-1.0, 1.0]), size=v.shape).astype(LD) * np.abs(v) * LD(EPS)
        n_cam = len(intr)
        dR, dt = np.zeros(n_cam), np.zeros(n_cam)
        ok = out["status"] == OK
        for _ in range(RUNS):
            q = _solve(jig(intr), jig(pts), row_ptr, pt_idx, jig(uv), min_points, min_gap, cam_mask, rng)
            both = ok & (q["status"] == OK)
            dR[both] = np.maximum(dR[both], np.abs((q["R"][both] - out["R"][both]).astype(np.float64)).max(axis=(1, 2)))
            dt[both] = np.maximum(dt[both], np.linalg.norm((q["t"][both] - out["t"][both]).astype(np.float64), axis=1))
            dR[ok & ~both] = dt[ok & ~both] = np.inf             # a status that rounding alone changes has no bound
        tn = np.linalg.norm(np.where(ok[:, None], out["t"], 0).astype(np.float64), axis=1)
        out["bound_R"] = np.where(ok, np.maximum(MULT * dR, FLOOR), 0.0)
        out["bound_t"] = np.where(ok, np.maximum(MULT * dt, FLOOR * tn), 0.0)
    return out


def cap_violations(ref):
    """cameras one of whose decisions lies within CAP (relative) of its threshold: lambda_2 / lambda_9 against min_gap, and,
    for those that pass it, lambda_1 / lambda_2 against 1 / 4.  (n_used against min_points is an integer comparison.)"""
    l1, l2, l9, g = ref["lam1"], ref["lam2"], ref["lam9"], ref["min_gap"]
    with np.errstate(all="ignore"):
        seen = np.isfinite(l9)
        gap = seen & (np.abs(l2 - g * l9) <= CAP * g * np.abs(l9)) & (g > 0)
        quarter = seen & ~(l2 < g * l9) & (np.abs(l1 - l2 / 4) <= CAP * np.abs(l2) / 4)
    return np.flatnonzero(gap | quarter)


def counts_of(status):
    return dict(zip(STATUS, (int(v) for v in np.bincount(status, minlength=5))))


def rotation_angle_deg(Ra, Rb):
    """the angle of Ra Rb^T, per camera"""
    tr = np.einsum("nij,nij->n", np.asarray(Ra, dtype=np.float64), np.asarray(Rb, dtype=np.float64))
    return np.rad2deg(np.arccos(np.clip((tr - 1) / 2, -1, 1)))


def pose_of(cams15):
    """(R [n, 3, 3] with q = R X + t, t [n, 3]) of cams15 rows (R column-major 0..8, t 9..11)"""
    cams15 = np.asarray(cams15)
    return cams15[:, :9].reshape(-1, 3, 3).swapaxes(1, 2), cams15[:, 9:12]


# ---- the problems -------------------------------------------------------------------------------------------------------
DOME_CASES = [(state, noise) for state in (False, True) for noise in (0.0, 1e-3)]
START_ROTATION, START_TRANSLATION = 0.3, 1.0                 # every pose starts this far from the truth


def dome_case(state, obs_noise, start_seed=17):
    """tests/_problems.py's dome_problem with its true points, observations with obs_noise, and every camera's rotation
    vector moved by exactly START_ROTATION and its translation by exactly START_TRANSLATION in seeded directions"""
    import oracle as O
    from _problems import dome_problem
    P = dict(dome_problem(seed=0, dup=True, state=state, obs_noise=obs_noise, start_noise=0.0))
    rng = np.random.default_rng(start_seed)
    g = rng.normal(size=(len(P["bal9"]), 2, 3))
    g = g / np.linalg.norm(g, axis=2)[:, :, None]
    bal9 = P["true_bal9"].copy()
    bal9[:, 0:3] += START_ROTATION * g[:, 0]
    bal9[:, 3:6] += START_TRANSLATION * g[:, 1]
    P["bal9"], P["cams15"], P["pts"] = bal9, O.camera_from_bal(bal9), P["true_pts"].copy()
    return P


def _camera(rng, f=1.0, k1=0.0, k2=0.0):
    """a cams15 row in general position: a random rotation, the centre within 10 of the origin"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    C = rng.uniform(-10, 10, size=3)
    return np.concatenate([Rm.T.ravel(), -Rm @ C, [f, k1, k2]])


def _world(cam, q):
    """the world points of camera-frame points q [n, 3]"""
    Rm, t = pose_of(cam[None])
    return (np.asarray(q) - t[0]) @ Rm[0]                        # R^T (q - t), row-wise


def _project(cam, X):
    Rm, t = pose_of(cam[None])
    q = np.asarray(X) @ Rm[0].T + t[0]
    p = -q[:, :2] / q[:, 2:3]
    n = np.sum(p * p, axis=1)[:, None]
    return cam[12] * (1 + cam[13] * n + cam[14] * n * n) * p


def _frame_points(rng, n, half=0.4, near=6.0, far=12.0):
    """n camera-frame points in front of the camera (z in [-far, -near], |x|, |y| <= half |z|)"""
    z = -rng.uniform(near, far, n)
    return np.stack([rng.uniform(-half, half, n) * -z, rng.uniform(-half, half, n) * -z, z], axis=1)


EDGE = dict(general=0, coplanar=1, two_unusable=2, reflected=3, clustered=4, no_distortion=5)      # camera indices of the edge set
CLUSTER = 0.1                                                # the clustered camera's points lie within this of their centre


def edge_problem():
    """Six hand-placed cameras in general position, each seeing points of its own (EDGE), true poses moved by 0.2 / 0.5:
      general        twelve points, k1 and k2 nonzero: status 0;
      coplanar       twelve points on one plane: status 2;
      two_unusable   k1 = -50; five points within radius 0.03 of the axis, one observation at radius 0.2 (1 + 3 k1 rho^2 =
                     -5 <= 0) and one of a NaN point: n_used = 5, status 1;
      reflected      ten points X' = 2 C - X: the pixels of X, all behind: status 3;
      clustered      twelve points within CLUSTER of a centre nine away: lambda_2 / lambda_9 between 1e-7 and 1e-4, status 2
                     at min_gap 1e-4 and 0 at 1e-7;
      no_distortion  k1 = k2 = 0, ten points: no Newton iteration, status 0.
    Loaded in state mode (from_visibility).  Returns dict(cams15 (the start), true_cams15, pts, row_ptr, pt_idx, uv, bal=False)."""
    import oracle as O
    rng = np.random.default_rng(5)
    cams, pts, obs = [], [], []

    def add(cam, X, uv=None):
        cams.append(cam)
        uv = _project(cam, X) if uv is None else uv
        obs.append([(len(pts) + k, uv[k]) for k in range(len(X))])
        pts.extend(list(X))
    cam = _camera(rng, 1.1, 2e-2, -3e-3)                         # general
    add(cam, _world(cam, _frame_points(rng, 12)))
    cam = _camera(rng, 0.9, -1e-2, 2e-3)                         # coplanar: a plane tilted against the image plane
    q = _frame_points(rng, 12)
    q[:, 2] = -9.0 + 0.3 * q[:, 0] - 0.2 * q[:, 1]
    add(cam, _world(cam, q))
    cam = _camera(rng, 1.0, -50.0, 0.0)                          # two_unusable
    q = _frame_points(rng, 7, half=0.02)
    X, uv = _world(cam, q), _project(cam, _world(cam, q))
    uv[5] = [0.2, 0.0]
    X[6] = np.nan
    add(cam, X, uv)
    cam = _camera(rng, 1.2, 1e-2, 1e-3)                          # reflected
    X = _world(cam, _frame_points(rng, 10))
    Rm, t = pose_of(cam[None])
    add(cam, 2.0 * (-Rm[0].T @ t[0]) - X, _project(cam, X))
    cam = _camera(rng, 1.0, 1e-2, 0.0)                           # clustered
    add(cam, _world(cam, np.array([0.5, -0.4, -9.0]) + rng.uniform(-CLUSTER, CLUSTER, size=(12, 3))))
    cam = _camera(rng, 0.95, 0.0, 0.0)                           # no_distortion
    add(cam, _world(cam, _frame_points(rng, 10)))
    true = np.ascontiguousarray(np.asarray(cams))
    bal9 = O.camera_to_bal(true)
    g = np.random.default_rng(6).normal(size=(len(bal9), 2, 3))
    g = g / np.linalg.norm(g, axis=2)[:, :, None]
    bal9[:, 0:3] += 0.2 * g[:, 0]
    bal9[:, 3:6] += 0.5 * g[:, 1]
    row_ptr = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.uint64)
    pt_idx = np.array([p for o in obs for p, _ in o], dtype=np.uint64)
    uv = np.array([v for o in obs for _, v in o], dtype=np.float64)
    return dict(cams15=O.camera_from_bal(bal9), true_cams15=true, pts=np.asarray(pts, dtype=np.float64), row_ptr=row_ptr, pt_idx=pt_idx,
                uv=uv, bal=False)


def edge_expected(min_gap):
    """status per camera of edge_problem at min_gap 1e-4 and 1e-7"""
    s = np.zeros(6, dtype=np.uint8)
    s[EDGE["coplanar"]] = DEGENERATE
    s[EDGE["two_unusable"]] = TOO_FEW
    s[EDGE["reflected"]] = BEHIND
    s[EDGE["clustered"]] = DEGENERATE if min_gap > 1e-6 else OK
    return s


# ---- the end-to-end run: constant points and intrinsics, the poses from a noisy start and from a resected one ------------
# chosen with host_cameras_lm below on tests/_problems.py's grid_problem (DESIGN 4.10 has the figures); the GPU test asserts
# the ordering for the reference alone, on the problem itself, before it asks the device
E2E_ROTATION_STD, E2E_TRANSLATION_STD = 0.3, 1.0


def host_cameras_lm(P, iterations, lam=1e-4):
    """_solvecheck.host_lm's loop with every point and every intrinsic constant: the damped system is then block diagonal
    over the cameras, (U + lam D) dc = -gc on the six pose parameters, solved exactly camera by camera.  The same acceptance
    and damping update.  Returns the sums of squared residuals [iterations + 1] and the final bal9."""
    import oracle as O
    import _solvecheck as SC
    bal9, pts = P["bal9"].copy(), P["pts"]
    n_cam, n_pts = len(bal9), len(pts)

    def lin(b9):
        r, Jc, Jp = O.residual_jacobian_bal(b9, pts, P["row_ptr"], P["pt_idx"], P["uv"])
        return R_.Problem(r, Jc, Jp, SC.cam_of(P["row_ptr"]), P["pt_idx"].astype(np.int64), n_cam, n_pts)

    Q = lin(bal9)
    e0, nu, out = float(np.sum(Q.r * Q.r)), 2.0, []
    out.append(e0)
    dp = np.zeros((n_pts, 3))
    for _ in range(iterations):
        dc = np.zeros((n_cam, 9))
        with np.errstate(all="ignore"):
            dc[:, :6] = -np.linalg.solve(R_.damp(Q.U[:, :6, :6], lam), Q.gc[:, :6, None])[:, :, 0]
        dc = np.where(np.isfinite(dc), dc, 0.0)
        with np.errstate(all="ignore"):
            Q1 = lin(bal9 + dc)
            e1 = float(np.sum(Q1.r * Q1.r))
        md = float(Q.model_decrease(dc, dp))
        rho = (e0 - e1) / md if md > 0.0 else -1.0
        if rho > 0.0 and e1 < e0:
            lam = min(max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e-20), 1e32)
            nu = 2.0
            bal9, Q, e0 = bal9 + dc, Q1, e1
        else:
            lam = min(max(lam * nu, 1e-20), 1e32)
            nu *= 2.0
        out.append(e0)
    return out, bal9


E2E_EVERY, E2E_OBS_NOISE = 12, 1e-3


def e2e_problem():
    """every E2E_EVERY-th camera of tests/_problems.py's grid_problem with its row, all of the grid's points at the truth,
    observations with noise E2E_OBS_NOISE, and every pose moved by N(0, E2E_ROTATION_STD) in the rotation vector and
    N(0, E2E_TRANSLATION_STD) in the translation.  Returns dict(bal9, true_bal9, pts, row_ptr, pt_idx, uv)."""
    import oracle as O
    from _problems import grid_problem
    G = grid_problem()
    rp = G["row_ptr"].astype(np.int64)
    keep = np.arange(0, len(G["cams15"]), E2E_EVERY)
    sel = np.concatenate([np.arange(rp[c], rp[c + 1]) for c in keep])
    row_ptr = np.concatenate([[0], np.cumsum(rp[keep + 1] - rp[keep])]).astype(np.uint64)
    rng = np.random.default_rng(21)
    uv = G["uv"][sel] + rng.normal(scale=E2E_OBS_NOISE, size=(len(sel), 2))
    true = O.camera_to_bal(np.ascontiguousarray(G["cams15"][keep]))
    bal9 = true.copy()
    bal9[:, 0:3] += rng.normal(scale=E2E_ROTATION_STD, size=(len(keep), 3))
    bal9[:, 3:6] += rng.normal(scale=E2E_TRANSLATION_STD, size=(len(keep), 3))
    return dict(bal9=bal9, true_bal9=true, pts=np.ascontiguousarray(G["pts"]), row_ptr=row_ptr, pt_idx=np.ascontiguousarray(G["pt_idx"][sel]), uv=uv)


def resected_bal9(bal9, ref):
    """bal9 with the poses of the reference's resected cameras (the oracle's to_rodrigues), the others as they are"""
    import oracle as O
    ok = ref["status"] == OK
    c15 = O.camera_from_bal(bal9).copy()
    c15[ok, :9] = ref["R"][ok].astype(np.float64).swapaxes(1, 2).reshape(-1, 9)
    c15[ok, 9:12] = ref["t"][ok].astype(np.float64)
    out = O.camera_to_bal(np.ascontiguousarray(c15))
    out[~ok] = bal9[~ok]
    return out
