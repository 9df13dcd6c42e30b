"""Host reference of per-point Levenberg-Marquardt (BAProblem.refine_points) in numpy.longdouble, its float64
twin, and the bounds its tests use.  numpy only: nothing here touches a device.

Every point is minimised by itself with the cameras held.  Per observation r and Jp come from tests/_jacref.py
(reference_bal / reference_state, longdouble); rho and w = rho' are restated from DESIGN 4.3's table:
    0 squared   rho = s                                       w = 1
    1 Huber     rho = s (s <= a^2), else 2 a sqrt(s) - a^2    w = 1 (s <= a^2), else a / sqrt(s)
    2 Cauchy    rho = a^2 log1p(s / a^2)                      w = 1 / (1 + s / a^2)
    3 soft-L1   rho = 2 a^2 (sqrt(1 + s / a^2) - 1)           w = 1 / sqrt(1 + s / a^2)
A walk at X gives F = sum rho(|r|^2) + |w_X o (X - X0)|^2, V = sum w Jp^T Jp + diag(w_X^2), g = sum w Jp^T r + w_X o r_X.
Round k: the gradient test (max |g| <= gradient_tol); (V + mu diag(d)) delta = -g by a 3x3 Cholesky, d = V's diagonal
clamped to [1e-6, 1e32] (a pivot <= 0 or a non-finite delta: a rejection); the parameter test
(|delta| <= parameter_tol (|X| + parameter_tol)); a walk at X + delta; model = -(2 g.delta + delta^T V delta),
gain = (F - F') / model if model > 0 else -1; accepted iff gain > 0, F' < F and F' finite: the state becomes the trial's,
mu *= max(1/3, 1 - (2 gain - 1)^3), nu = 2, then the function test (F - F' <= function_tol F); rejected: mu *= nu, nu *= 2;
mu held in [1e-20, 1e32].  A tolerance of 0 disables its test.

`dtype` is the precision of the loop: np.longdouble is the reference, np.float64 its *float64 twin* -- the same loop with r
and Jp FORMED in float64, in the kernel's order of operations (tests/_jacref.py's kernel_f64: from_rodrigues, the projection,
jacobian_obs restated in numpy f64), and every sum, solve and comparison in f64: an f64 evaluation with a rounding of its own,
different from the device's but equally valid.  The margins of tests/test_gpu_refine.py are measured against the twin,
never against the device.

Beside F the walk carries a rounding bound of the shape the project uses for sums, B = sum |terms| 2^-52 (depth + 16), depth
the number of terms (the observations and the prior's three rows): what an f64 evaluation of F in any order may differ by.
The terms are positive, so sum |terms| = F.  One floor, for points whose cost is 0 to the rounding of f64 residuals (a point
seen once or twice fits its pixels; exact pixels; a prior-only point): a residual u - o formed in f64 is off by about
e = (|u| + |o|) 2^-52 x 16 (the projection's operations, the count the shape adds to the depth), so no f64 evaluation tells a
cost below sum e^2 from 0, and B is at least that sum (the prior's rows alike, with w (|x| + |x0|)).  The floor is
B = max(., floor), not an addition: it is 1e-29 per observation at pixels of size 1 and reaches a point only when its cost
is below about 1e-14, eight orders under the cost of a point with pixel noise 1e-3."""
import numpy as np

import _jacref as J

LD = np.longdouble
EPS = 2.0 ** -52
LAMBDA_MIN, LAMBDA_MAX = 1e-20, 1e32
CONVERGED, MAX_ROUNDS, UNOBSERVED, FAILED, CONSTANT = range(5)
STATUS = ("converged", "max_rounds", "unobserved", "failed", "constant")
COUNTS = STATUS + ("moved",)
KINDS = {None: 0, "squared": 0, "huber": 1, "cauchy": 2, "soft_l1": 3}


def _rho_w(kind, a, s):
    """(rho(s), rho'(s)) in s's dtype"""
    T = s.dtype.type
    a2 = T(a) * T(a)
    one = T(1)
    if kind == 0:
        return s.copy(), np.ones_like(s)
    if kind == 1:
        big = s > a2
        sb = np.where(big, s, one)
        return np.where(big, T(2) * T(a) * np.sqrt(sb) - a2, s), np.where(big, T(a) / np.sqrt(sb), one)
    q = one + s / a2
    if kind == 2:
        return a2 * np.log1p(s / a2), one / q
    if kind == 3:
        return T(2) * s / (np.sqrt(q) + one), one / np.sqrt(q)
    raise ValueError("loss kind %r" % (kind,))


class Problem:
    """cams: bal9 [n_cam, 9] (bal=True) or cam15 [n_cam, 15]; the list camera-major (row_ptr, pt_idx, uv); loss by name with
    its scale; prior = (X0 [n_pts, 3], w_X [n_pts, 3]) or None; mask [n_pts] bool (constant points) or None"""

    def __init__(self, cams, bal, row_ptr, pt_idx, uv, n_pts, loss=None, loss_scale=1.0, prior=None, mask=None):
        self.cams, self.bal = np.asarray(cams, dtype=np.float64), bool(bal)
        row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.cam_of = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
        self.pt = np.asarray(pt_idx).astype(np.int64)
        self.uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
        self.n_pts = int(n_pts)
        self.kind, self.a = KINDS[loss], float(loss_scale)
        self.count = np.bincount(self.pt, minlength=self.n_pts)
        self.mask = np.zeros(self.n_pts, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        if prior is None:
            self.x0, self.xw = np.zeros((self.n_pts, 3)), np.zeros((self.n_pts, 3))
        else:
            self.xw = np.asarray(prior[1], dtype=np.float64)
            self.x0 = np.where(self.xw != 0.0, np.asarray(prior[0], dtype=np.float64), 0.0)      # a target under weight 0 is never read
        self.observed = (self.count > 0) | np.any(self.xw != 0.0, axis=1)

    def observations(self, X, dtype=LD):
        """(r [n_obs, 2], Jp [n_obs, 2, 3]) at the positions X [n_pts, 3]: in longdouble from the reference forms, or (dtype
        float64, the twin) formed in f64 in the kernel's order; self.mag [n_obs, 2] (f64) = |u| + |o|"""
        Xo = np.asarray(X)[self.pt]
        with np.errstate(all="ignore"):
            if np.dtype(dtype) == np.float64:
                cams = self.cams[self.cam_of]
                Xf = np.asarray(Xo, dtype=np.float64)
                jc, jp, aux = J.kernel_f64("bal" if self.bal else "state", cams, Xf, None if self.bal else np.zeros((len(Xf), 3)))
                fr = cams[:, 6 if self.bal else 12] * aux["rad"].v                       # project_tail: (f rad) p
                u = np.stack([fr * aux["px"].v, fr * aux["py"].v], axis=1)
                self.mag = np.abs(u) + np.abs(self.uv)
                return u - self.uv, J.stack(jc, jp)[2]
            if self.bal:
                ref = J.reference_bal(self.cams[self.cam_of], Xo, self.uv)
            else:
                ref = J.reference_state(self.cams[self.cam_of], np.zeros((len(Xo), 3)), Xo, self.uv)      # (w enters Jc alone)
            self.mag = (np.abs(ref["uv"]) + np.abs(self.uv)).astype(np.float64)
        return ref["r"], ref["Jp"]

    def walk(self, X, dtype=LD, linear=True):
        """dict(F [n_pts], B [n_pts] (f64: the rounding bound on F), V [n_pts, 3, 3], g [n_pts, 3]) in dtype at X [n_pts, 3]"""
        T = np.dtype(dtype).type
        X = np.asarray(X).astype(dtype)
        n = self.n_pts
        with np.errstate(all="ignore"):
            if len(self.pt):
                r, Jp = self.observations(X, dtype)
                s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
                rho, w = _rho_w(self.kind, self.a, s)
            else:
                r, Jp, rho, w = np.zeros((0, 2), dtype), np.zeros((0, 2, 3), dtype), np.zeros(0, dtype), np.zeros(0, dtype)
            F = np.zeros(n, dtype=dtype)
            np.add.at(F, self.pt, rho)
            xw, x0 = self.xw.astype(dtype), self.x0.astype(dtype)
            q = np.where(xw != 0, xw * (X - x0), T(0))
            F = F + ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
            B = np.abs(F).astype(np.float64) * EPS * (self.count + 3 + 16.0)
            floor = np.zeros(n)                                 # a cost that f64 residuals cannot tell from 0 (module docstring)
            if len(self.pt):
                e = self.mag * (16.0 * EPS)
                np.add.at(floor, self.pt, np.sum(e * e, axis=1))
            ep = np.abs(self.xw) * (np.abs(X.astype(np.float64)) + np.abs(self.x0)) * (16.0 * EPS)
            B = np.maximum(B, floor + np.sum(np.where(self.xw != 0, ep * ep, 0.0), axis=1))
            out = dict(F=F, B=B)
            if linear:
                V = np.zeros((n, 3, 3), dtype=dtype)
                g = np.zeros((n, 3), dtype=dtype)
                np.add.at(V, self.pt, w[:, None, None] * np.einsum("nia,nib->nab", Jp, Jp))
                np.add.at(g, self.pt, w[:, None] * np.einsum("nia,ni->na", Jp, r))
                V[:, [0, 1, 2], [0, 1, 2]] += xw * xw
                out.update(V=V, g=g + xw * q)
        return out

    def cost(self, X):
        """(F, B): the longdouble cost of every point at X and its rounding bound"""
        o = self.walk(X, LD, linear=False)
        return o["F"], o["B"]


def solve3(V, g, mu):
    """(delta, ok): (V + mu diag(d)) delta = -g by a 3x3 Cholesky in V's dtype, d = clamp(diag V, 1e-6, 1e32); ok = the three
    pivots are positive and delta is finite"""
    T = V.dtype.type
    with np.errstate(all="ignore"):
        A = V.copy()
        d = np.minimum(np.maximum(V[:, [0, 1, 2], [0, 1, 2]], T(1e-6)), T(1e32))
        A[:, [0, 1, 2], [0, 1, 2]] += mu[:, None] * d
        d1 = A[:, 0, 0]
        l00 = np.sqrt(d1)
        l10, l20 = A[:, 0, 1] / l00, A[:, 0, 2] / l00
        d2 = A[:, 1, 1] - l10 * l10
        l11 = np.sqrt(d2)
        l21 = (A[:, 1, 2] - l20 * l10) / l11
        d3 = (A[:, 2, 2] - l20 * l20) - l21 * l21
        l22 = np.sqrt(d3)
        b = -g
        y0 = b[:, 0] / l00
        y1 = (b[:, 1] - l10 * y0) / l11
        y2 = ((b[:, 2] - l20 * y0) - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = ((y0 - l10 * x1) - l20 * x2) / l00
        delta = np.stack([x0, x1, x2], axis=1)
        ok = (d1 > 0) & (d2 > 0) & (d3 > 0) & np.all(np.isfinite(delta), axis=1)
    return delta, ok


def refine(P, X, rounds=10, lam=1e-4, function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0, dtype=LD):
    """The per-point loop on Problem P from the positions X [n_pts, 3] (f64).  Returns dict(X [n_pts, 3] (dtype; the input's
    values where nothing moved), status [n_pts] uint8, moved [n_pts] bool, counts (COUNTS -> int), F0, F (dtype: the cost at
    the start and at the end), B (f64: the bound on F at the end), rounds: one dict per round with F, Ft (F'), delta,
    accepted, tried (a walk was made), mu (the damping the round used) -- NaN / False for a point that was not running)."""
    T = np.dtype(dtype).type
    n = P.n_pts
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    status = np.full(n, MAX_ROUNDS, dtype=np.uint8)
    status[~P.observed] = UNOBSERVED
    status[P.mask] = CONSTANT
    cur = P.walk(X, dtype)
    cand = P.observed & ~P.mask
    status[cand & ~np.isfinite(cur["F"])] = FAILED
    live = cand & np.isfinite(cur["F"])
    F0 = cur["F"].copy()
    mu, nu = np.full(n, T(min(max(lam, LAMBDA_MIN), LAMBDA_MAX))), np.full(n, T(2))
    moved = np.zeros(n, dtype=bool)
    hist = []
    nan = T(np.nan)
    with np.errstate(all="ignore"):
        for _ in range(int(rounds)):
            rec = dict(F=np.where(live, cur["F"], nan), mu=np.where(live, mu, nan), B=np.where(live, cur["B"], np.nan))
            if gradient_tol > 0.0:
                done = live & (np.max(np.abs(cur["g"]), axis=1) <= T(gradient_tol))
                status[done] = CONVERGED
                live = live & ~done
            delta, ok = solve3(cur["V"], cur["g"], mu)
            ok = ok & live
            if parameter_tol > 0.0:
                dn = np.sqrt(np.sum(delta * delta, axis=1))
                xn = np.sqrt(np.sum(X * X, axis=1))
                done = ok & (dn <= T(parameter_tol) * (xn + T(parameter_tol)))
                status[done] = CONVERGED
                live, ok = live & ~done, ok & ~done
            Xt = np.where(ok[:, None], X + delta, X)
            tri = P.walk(Xt, dtype)
            Vd = np.einsum("pab,pb->pa", cur["V"], delta)
            model = -(T(2) * np.sum(cur["g"] * delta, axis=1) + np.sum(delta * Vd, axis=1))
            gain = np.where(model > 0, (cur["F"] - tri["F"]) / np.where(model > 0, model, T(1)), T(-1))
            acc = ok & (gain > 0) & (tri["F"] < cur["F"]) & np.isfinite(tri["F"])
            rej = live & ~acc
            rec.update(Ft=np.where(ok, tri["F"], nan), delta=np.where(ok[:, None], delta, nan), accepted=acc.copy(), tried=ok.copy(),
                       Bt=np.where(ok, tri["B"], np.nan), model=np.where(ok, model, nan))
            hist.append(rec)
            c = T(2) * gain - T(1)
            mu_acc = np.minimum(np.maximum(mu * np.maximum(T(1) / T(3), T(1) - (c * c) * c), T(LAMBDA_MIN)), T(LAMBDA_MAX))
            mu_rej = np.minimum(np.maximum(mu * nu, T(LAMBDA_MIN)), T(LAMBDA_MAX))
            small = acc & (cur["F"] - tri["F"] <= T(function_tol) * cur["F"]) if function_tol > 0.0 else np.zeros(n, dtype=bool)
            mu = np.where(acc, mu_acc, np.where(rej, mu_rej, mu))
            nu = np.where(acc, T(2), np.where(rej, nu * T(2), nu))
            X = np.where(acc[:, None], Xt, X)
            for k in ("F", "B", "V", "g"):
                sel = acc.reshape((-1,) + (1,) * (cur[k].ndim - 1))
                cur[k] = np.where(sel, tri[k], cur[k])
            moved |= acc
            status[small] = CONVERGED
            live = live & ~small
    counts = dict(zip(STATUS, (int(v) for v in np.bincount(status, minlength=5))))
    counts["moved"] = int(moved.sum())
    return dict(X=X, status=status, moved=moved, counts=counts, F0=F0, F=cur["F"], B=cur["B"], rounds=hist)


# ---- the bound on one round's step (tests/test_gpu_refine.py, check 1) ------------------------------------------------------
# Roundings the weighting adds to one product (sqrt(w) J_a)(sqrt(w) J_b), as tests/test_gpu_robust_loss.py counts them: 12
WEIGHT_OPS = 12


def step_tolerance(P, X, mu, entries=True):
    """Per point, the tolerance on the first round's delta of an f64 evaluation in the device's arithmetic, to first order:
    cond(V_mu) (|dV| / |V_mu| + |dg| / |g|) |delta|, with V_mu = V + mu diag(d) of the longdouble reference and dV, dg the
    entrywise bounds on V and g: _normref.bound (any f64 summation order of the products, (k + 4 + WEIGHT_OPS) 2^-53 S with
    S the sums of absolute products and the prior's own terms among them) plus what the entries of r and Jp themselves may
    be off by in the kernel's arithmetic (_jacref.kernel_f64's running bounds E, with _jacref's margin C), propagated
    through the products; entries=False leaves that part out (the bound of the sums alone, which an f64 evaluation with
    any rounding in r and Jp need not meet: the twin exceeds it on the ragged problem).  Returns (tol [n_pts] f64, delta [n_pts, 3] longdouble, ok [n_pts])."""
    import _normref as NR
    n = P.n_pts
    cur = P.walk(X, LD)
    delta, ok = solve3(cur["V"], cur["g"], np.full(n, LD(mu)))
    with np.errstate(all="ignore"):
        r, Jp = P.observations(np.asarray(X, dtype=np.float64))
        s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        _, w = _rho_w(P.kind, P.a, s)
        aJ, ar = np.abs(Jp).astype(np.float64) * np.sqrt(w.astype(np.float64))[:, None, None], np.abs(r).astype(np.float64) * np.sqrt(w.astype(np.float64))[:, None]
        Xo = np.asarray(X, dtype=np.float64)[P.pt]
        cams_o = P.cams[P.cam_of]
        mode = "bal" if P.bal else "state"
        jc, jp, aux = J.kernel_f64(mode, cams_o, Xo, None if P.bal else np.zeros((len(Xo), 3)))
        Ep = J.stack(jc, jp)[3] * np.sqrt(w.astype(np.float64))[:, None, None]
        f = J.V(cams_o[:, 6 if P.bal else 12])
        Er = np.stack([(f * aux["rad"] * aux["px"]).e, (f * aux["rad"] * aux["py"]).e], axis=1) * np.sqrt(w.astype(np.float64))[:, None]
        SV, Sg, EV, Eg = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3))
        np.add.at(SV, P.pt, np.einsum("nia,nib->nab", aJ, aJ))
        np.add.at(Sg, P.pt, np.einsum("nia,ni->na", aJ, ar))
        np.add.at(EV, P.pt, np.einsum("nia,nib->nab", aJ, Ep) + np.einsum("nia,nib->nab", Ep, aJ))
        np.add.at(Eg, P.pt, np.einsum("nia,ni->na", aJ, Er) + np.einsum("nia,ni->na", Ep, ar))
        SV[:, [0, 1, 2], [0, 1, 2]] += P.xw * P.xw
        Sg += P.xw * np.abs(P.xw * (np.asarray(X, dtype=np.float64) - P.x0))
        dV = NR.bound(SV, P.count + 3 + WEIGHT_OPS) + (J.C * EV if entries else 0.0)
        dg = NR.bound(Sg, P.count + 3 + WEIGHT_OPS) + (J.C * Eg if entries else 0.0)
        A = cur["V"].astype(np.float64).copy()
        d = np.clip(A[:, [0, 1, 2], [0, 1, 2]], 1e-6, 1e32)
        A[:, [0, 1, 2], [0, 1, 2]] += float(mu) * d
        good = ok & np.all(np.isfinite(A.reshape(n, -1)), axis=1)
        sv = np.ones((n, 3))
        sv[good] = np.linalg.svd(A[good], compute_uv=False)
        cond = sv[:, 0] / sv[:, 2]
        gn = np.linalg.norm(cur["g"].astype(np.float64), axis=1)
        rel = np.linalg.norm(dV.reshape(n, -1), axis=1) / sv[:, 0] + np.where(gn > 0, np.linalg.norm(dg, axis=1) / np.where(gn > 0, gn, 1.0), 0.0)
        tol = cond * rel * np.linalg.norm(delta.astype(np.float64), axis=1)
    return tol, delta, ok


# ---- the problems --------------------------------------------------------------------------------------------------------
RAGGED_LENGTHS = (0, 1, 2, 3, 5, 8, 17, 20)                  # a point's list: empty, rank-deficient, short, and above 16


def ragged_problem(seed=5, noise=1e-3, start=0.05):
    """tests/_problems.py's random_problem(7 cameras, 300 points; k2 != 0 on four of the seven) with its list rebuilt ragged:
    point j is observed RAGGED_LENGTHS[j % 8] times, by cameras drawn with replacement among those that see it in front of
    them at a moderate angle (its owner is one) -- repeated measurements of a camera are observations like any other.  Pixels
    carry `noise`, the points start `start` from the truth in a seeded direction.  300 points: two workgroups of 256 with a
    tail wave.  Loaded in bal mode.  Returns dict(bal9, cams15, pts, true_pts, row_ptr, pt_idx, uv, bal=True)."""
    import oracle as O
    from _problems import random_problem
    Q = random_problem(7, 300, 64, seed=seed, k_scale=1e-2)
    bal9 = Q["bal9"].copy()
    bal9[[1, 4, 6], 8] = 0.0                                  # mixed k2 inside a wave
    cams15 = O.camera_from_bal(bal9)
    pts = Q["pts"]
    rng = np.random.default_rng(seed + 1)
    R = cams15[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    q = np.einsum("cij,pj->cpi", R, pts) + cams15[:, None, 9:12]
    sees = (q[:, :, 2] < -0.5) & (np.hypot(q[:, :, 0], q[:, :, 1]) < 1.5 * -q[:, :, 2])
    rows = [[] for _ in range(7)]
    for j in range(300):
        cand = np.flatnonzero(sees[:, j])
        assert len(cand) >= 1
        for c in rng.choice(cand, size=RAGGED_LENGTHS[j % len(RAGGED_LENGTHS)], replace=True):
            rows[int(c)].append(j)
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    pt_idx = np.asarray([j for r in rows for j in r], dtype=np.uint64)
    uv = O.project_observations(cams15, pts, row_ptr, pt_idx) + rng.normal(scale=noise, size=(len(pt_idx), 2))
    g = rng.normal(size=pts.shape)
    return dict(bal9=bal9, cams15=cams15, pts=pts + start * g / np.linalg.norm(g, axis=1)[:, None], true_pts=pts, row_ptr=row_ptr,
                pt_idx=pt_idx, uv=uv, bal=True)


def one_point_problem(n_cam=6, seed=2, noise=1e-3, start=0.3):
    """one point seen once by each of n_cam cameras of random_problem's kind that see it in front: the per-point loop and a
    global loop over all points coincide here.  bal mode."""
    import oracle as O
    from _problems import random_problem
    Q = random_problem(40, 40, 64, seed=seed, k_scale=1e-2)
    cams15 = Q["cams15"]
    R = cams15[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    for j in range(40):
        q = R @ Q["pts"][j] + cams15[:, 9:12]
        see = np.flatnonzero((q[:, 2] < -0.5) & (np.hypot(q[:, 0], q[:, 1]) < -q[:, 2]))
        if len(see) >= n_cam:
            break
    else:
        raise AssertionError("no point is seen by %d cameras" % n_cam)
    see = see[:n_cam]
    bal9 = np.ascontiguousarray(Q["bal9"][see])
    rng = np.random.default_rng(seed + 1)
    pts = Q["pts"][j:j + 1]
    row_ptr = np.arange(n_cam + 1, dtype=np.uint64)
    pt_idx = np.zeros(n_cam, dtype=np.uint64)
    uv = O.project_observations(O.camera_from_bal(bal9), pts, row_ptr, pt_idx) + rng.normal(scale=noise, size=(n_cam, 2))
    g = rng.normal(size=3)
    return dict(bal9=bal9, cams15=O.camera_from_bal(bal9), pts=pts + start * g / np.linalg.norm(g), true_pts=pts, row_ptr=row_ptr,
                pt_idx=pt_idx, uv=uv, bal=True)


def small_problem():
    """four cameras over six points, every point seen by all four, exact pixels (tests/_triangref.py's edge set without its
    appended pairs).  State mode."""
    import _triangref as T
    P = T.edge_problem()
    keep = int(P["row_ptr"][4])
    return dict(cams15=P["cams15"][:4], pts=P["pts"][:6].copy(), true_pts=P["true_pts"][:6], row_ptr=P["row_ptr"][:5], pt_idx=P["pt_idx"][:keep],
                uv=P["uv"][:keep], bal=False)


def hand_placed():
    """small_problem() with two points nobody sees appended, point 2 starting at NaN, point 1 constant and a prior on point 7
    alone: (P, mask, (x0, xw)) -- the statuses are MAX_ROUNDS, CONSTANT, FAILED, MAX_ROUNDS x 3, UNOBSERVED, MAX_ROUNDS"""
    P = small_problem()
    pts = np.vstack([P["pts"], [[0.1, 0.2, 0.3], [0.5, 0.5, 0.5]]])
    pts[2] = np.nan
    mask = np.zeros(8, dtype=bool)
    mask[1] = True
    x0, xw = np.full((8, 3), np.nan), np.zeros((8, 3))
    x0[7], xw[7] = [1.0, -2.0, 3.0], [2.0, 1.0, 0.5]
    return dict(P, pts=pts), mask, (x0, xw)


def of(P, cams=None, **kw):
    """the reference Problem of a problem dict (bal9 when P["bal"], else cams15), or of the cameras given"""
    bal = P.get("bal", True)
    if cams is None:
        cams = P["bal9"] if bal else P["cams15"]
    return Problem(cams, bal, P["row_ptr"], P["pt_idx"], P["uv"], len(P["pts"]), **kw)


def borderline(ref_round):
    """points whose first reference round lies inside the cost's rounding bound: |F - F'| <= B(F) + B(F'), or whose step
    could not be solved -- their accept decision is not compared"""
    with np.errstate(all="ignore"):
        gap = np.abs((ref_round["F"] - ref_round["Ft"]).astype(np.float64))
    return ref_round["tried"] & ~(gap > ref_round["Bt"] + ref_round["B"])
