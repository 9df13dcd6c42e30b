"""Host reference of the damped Gauss-Newton step (BAProblem.solve_step): from a per-observation residual and Jacobian
(BAProblem.residual_jacobian), the blocks U_c, V_p, W_o = Jc_o^T Jp_o, the gradient, Marquardt damping with Ceres'
clamps, the Schur complement S = U_l - W V_l^-1 W^T, b = -gc + W V_l^-1 gp, the back-substitution, and a dense direct
solve of the whole damped system.  numpy only.  Operator products come in np.longdouble together with a scale B made
of absolute values (sum |J_a J_b|, |V_l^-1|) that bounds the rounding of any f64 evaluation order to first order."""
import numpy as np

LD = np.longdouble


def damp_diag(d, lam):
    """the damped diagonal d + lam * clip(d, 1e-6, 1e32)"""
    return d + lam * np.minimum(np.maximum(d, 1e-6), 1e32)


def damp(A, lam):
    """A_l for a stack of square blocks A [m, k, k]"""
    A = np.array(A, copy=True)
    i = np.arange(A.shape[-1])
    A[:, i, i] = damp_diag(A[:, i, i], lam)
    return A


def inv3(A):
    """inverse of a stack of 3x3 matrices by the adjugate, in A's dtype (longdouble works)"""
    a, b, c = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2]
    d, e, f = A[:, 1, 0], A[:, 1, 1], A[:, 1, 2]
    g, h, k = A[:, 2, 0], A[:, 2, 1], A[:, 2, 2]
    adj = np.stack([np.stack([e * k - f * h, c * h - b * k, b * f - c * e], -1),
                    np.stack([f * g - d * k, a * k - c * g, c * d - a * f], -1),
                    np.stack([d * h - e * g, b * g - a * h, a * e - b * d], -1)], -2)
    det = a * adj[:, 0, 0] + b * adj[:, 1, 0] + c * adj[:, 2, 0]
    return adj / det[:, None, None]


class Problem:
    """the blocks of one linearisation: r [n,2], Jc [n,2,9], Jp [n,2,3], cam_of / pt_idx [n]"""

    def __init__(self, r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts, dtype=np.float64):
        n = len(cam_of)
        self.n_cam, self.n_pts, self.dtype = n_cam, n_pts, dtype
        self.r = np.asarray(r, dtype=np.float64).reshape(n, 2).astype(dtype)
        self.Jc = np.asarray(Jc, dtype=np.float64).reshape(n, 2, 9).astype(dtype)
        self.Jp = np.asarray(Jp, dtype=np.float64).reshape(n, 2, 3).astype(dtype)
        self.cam = np.asarray(cam_of, dtype=np.int64)
        self.pt = np.asarray(pt_idx, dtype=np.int64)
        self.U = self._sum(np.einsum("nia,nib->nab", self.Jc, self.Jc), self.cam, n_cam)
        self.V = self._sum(np.einsum("nia,nib->nab", self.Jp, self.Jp), self.pt, n_pts)
        self.gc = self._sum(np.einsum("nia,ni->na", self.Jc, self.r), self.cam, n_cam)
        self.gp = self._sum(np.einsum("nia,ni->na", self.Jp, self.r), self.pt, n_pts)
        self.W = np.einsum("nia,nib->nab", self.Jc, self.Jp)                 # per observation [n, 9, 3]
        aJc, aJp, ar = np.abs(self.Jc), np.abs(self.Jp), np.abs(self.r)
        self.SU = self._sum(np.einsum("nia,nib->nab", aJc, aJc), self.cam, n_cam)
        self.SV = self._sum(np.einsum("nia,nib->nab", aJp, aJp), self.pt, n_pts)
        self.Sgc = self._sum(np.einsum("nia,ni->na", aJc, ar), self.cam, n_cam)
        self.Sgp = self._sum(np.einsum("nia,ni->na", aJp, ar), self.pt, n_pts)
        self.aJc, self.aJp = aJc, aJp

    def _sum(self, per_obs, idx, m):
        out = np.zeros((m,) + per_obs.shape[1:], dtype=per_obs.dtype)
        np.add.at(out, idx, per_obs)
        return out

    # ---- the damped blocks ----------------------------------------------------------------------------------
    def Ul(self, lam):
        return damp(self.U, lam)

    def Vl(self, lam):
        return damp(self.V, lam)

    # ---- operators (in self.dtype), each with its absolute scale ---------------------------------------------
    def points(self, lam, x=None, h=None):
        """t = V_l^-1 (h + W^T x) per point and the scale of its rounding, |V_l^-1| (|Jp|^T |Jc| |x| + Sh + SV |t|)"""
        a = np.zeros((self.n_pts, 3), dtype=self.dtype)
        s = np.zeros((self.n_pts, 3), dtype=self.dtype)
        if h is not None:
            a += np.asarray(h).astype(self.dtype)
            s += self.Sgp
        if x is not None:
            x = np.asarray(x).reshape(self.n_cam, 9).astype(self.dtype)
            xo = x[self.cam]
            np.add.at(a, self.pt, np.einsum("nab,na->nb", self.W, xo))
            np.add.at(s, self.pt, np.einsum("nib,ni->nb", self.aJp, np.einsum("nia,na->ni", self.aJc, np.abs(xo))))
        Vi = inv3(self.Vl(lam))
        t = np.einsum("pab,pb->pa", Vi, a)
        scale = np.einsum("pab,pb->pa", np.abs(Vi), s + np.einsum("pab,pb->pa", self.SV, np.abs(t)))
        return t, scale

    def cameras(self, lam, x, t, tscale, h=None):
        """y = U_l x - W t per camera (h given: y = W t - h instead, x unused) and its scale"""
        t = np.asarray(t).astype(self.dtype)
        to = t[self.pt]
        wt = np.zeros((self.n_cam, 9), dtype=self.dtype)
        np.add.at(wt, self.cam, np.einsum("nab,nb->na", self.W, to))
        s = np.zeros((self.n_cam, 9), dtype=self.dtype)
        np.add.at(s, self.cam, np.einsum("nia,ni->na", self.aJc, np.einsum("nib,nb->ni", self.aJp, np.abs(to) + tscale[self.pt])))
        if h is not None:
            return wt - np.asarray(h).astype(self.dtype), s + self.Sgc
        x = np.asarray(x).reshape(self.n_cam, 9).astype(self.dtype)
        Ul = self.Ul(lam)
        SUl = self.SU + (Ul - self.U)                                       # the damping adds its own (exact) diagonal
        return np.einsum("cab,cb->ca", Ul, x) - wt, s + np.einsum("cab,cb->ca", SUl, np.abs(x))

    def S_times(self, lam, x):
        t, ts = self.points(lam, x=x)
        return self.cameras(lam, x, t, ts)

    def rhs(self, lam):
        t, ts = self.points(lam, h=self.gp)
        return self.cameras(lam, None, t, ts, h=self.gc)

    def back_substitute(self, lam, dc):
        """dp = -V_l^-1 (gp + W^T dc) and its scale"""
        t, ts = self.points(lam, x=dc, h=self.gp)
        return -t, ts

    # ---- dense forms (small problems, f64) --------------------------------------------------------------------
    def dense_S(self, lam):
        nc = self.n_cam
        S = np.zeros((9 * nc, 9 * nc))
        Ul = self.Ul(lam).astype(np.float64)
        for c in range(nc):
            S[9 * c:9 * c + 9, 9 * c:9 * c + 9] = Ul[c]
        Vi = inv3(self.Vl(lam).astype(np.float64))
        W = self.W.astype(np.float64)
        for p in range(self.n_pts):
            obs = np.nonzero(self.pt == p)[0]
            for o1 in obs:
                A = W[o1] @ Vi[p]
                c1 = self.cam[o1]
                for o2 in obs:
                    c2 = self.cam[o2]
                    S[9 * c1:9 * c1 + 9, 9 * c2:9 * c2 + 9] -= A @ W[o2].T
        return S

    def dense_H(self):
        """J^T J of the whole problem (cameras first, then points) and g"""
        nc, npt = self.n_cam, self.n_pts
        n = len(self.cam)
        J = np.zeros((2 * n, 9 * nc + 3 * npt))
        rows = np.arange(n)
        for i in range(2):
            for a in range(9):
                J[2 * rows + i, 9 * self.cam + a] = self.Jc[:, i, a].astype(np.float64)
            for a in range(3):
                J[2 * rows + i, 9 * nc + 3 * self.pt + a] = self.Jp[:, i, a].astype(np.float64)
        return J, J.T @ J, J.T @ self.r.astype(np.float64).reshape(-1)

    def direct(self, lam):
        """(dc, dp) by a dense solve of (H + lam D) delta = -g, D by the clamp rule on diag(H)"""
        _, H, g = self.dense_H()
        i = np.arange(len(g))
        Hl = H.copy()
        Hl[i, i] = damp_diag(H[i, i], lam)
        d = np.linalg.solve(Hl, -g)
        return d[:9 * self.n_cam].reshape(-1, 9), d[9 * self.n_cam:].reshape(-1, 3)

    def schur_direct(self, lam):
        """(dc, dp) by a dense solve of S dc = b and the back-substitution"""
        b, _ = self.rhs(lam)
        dc = np.linalg.solve(self.dense_S(lam), np.asarray(b, dtype=np.float64).reshape(-1)).reshape(-1, 9)
        dp, _ = self.back_substitute(lam, dc)
        return dc, np.asarray(dp, dtype=np.float64)

    def damped_residual(self, lam, dc, dp):
        """(H + lam D) delta + g, dense"""
        _, H, g = self.dense_H()
        i = np.arange(len(g))
        Hl = H.copy()
        Hl[i, i] = damp_diag(H[i, i], lam)
        d = np.concatenate([np.asarray(dc, dtype=np.float64).reshape(-1), np.asarray(dp, dtype=np.float64).reshape(-1)])
        return Hl @ d + g, g

    def model_decrease(self, dc, dp):
        """|r|^2 - |r + Jc dc + Jp dp|^2 in longdouble"""
        dc = np.asarray(dc, dtype=np.float64).astype(LD)
        dp = np.asarray(dp, dtype=np.float64).astype(LD)
        e = np.einsum("nia,na->ni", self.Jc.astype(LD), dc[self.cam]) + np.einsum("nia,na->ni", self.Jp.astype(LD), dp[self.pt])
        r = self.r.astype(LD)
        return np.sum(r * r) - np.sum((r + e) * (r + e))


# ---- PCG, iterate by iterate ----------------------------------------------------------------------------------------
EPS = 2.0 ** -52


def chol_blocks(A):
    """lower Cholesky factors of a stack of SPD blocks [m, k, k], in A's dtype (longdouble works)"""
    k = A.shape[1]
    L = np.zeros_like(A)
    for j in range(k):
        L[:, j, j] = np.sqrt(A[:, j, j] - np.sum(L[:, j, :j] * L[:, j, :j], axis=-1))
        for i in range(j + 1, k):
            L[:, i, j] = (A[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=-1)) / L[:, j, j]
    return L


def chol_inverse(L):
    """(L L^T)^-1 for a stack of lower factors"""
    k = L.shape[1]
    Li = np.zeros_like(L)                                                 # L^-1 by forward substitution
    for i in range(k):
        Li[:, i, i] = 1 / L[:, i, i]
        for j in range(i):
            Li[:, i, j] = -np.sum(L[:, i, j:i] * Li[:, j:i, j], axis=-1) / L[:, i, i]
    return np.einsum("mki,mkj->mij", Li, Li)


def pcg_loop(ops, max_iters, rel_tol, beta_scale=1.0):
    """c2b_problem_solve_step's loop over the operations `ops` provides: x0 = 0, r0 = b, z = M^-1 r, p0 = z0,
    alpha = rz / pq (no update unless pq > 0 and alpha is finite: breakdown, status 2, x the last good iterate),
    x += alpha p, r -= alpha q, z = M^-1 r, stop when |r_k| <= rel_tol |b| (status 0) or after max_iters (1), else
    beta = rz_new / rz, p = z + beta p.  Returns dict(xs, rs (the recurrence residual vectors), rel (|r_k| / |b|),
    status, iterations, rel_residual); xs[k] is the k-th iterate."""
    b = ops.rhs()
    x = ops.zeros_like(b)
    r = b
    z = ops.precond(r)
    p = z
    rr, rz = ops.dot_rr(r, r), ops.dot_rr(r, z)
    bb = rr
    bnorm = ops.sqrt(bb)
    rnorm = bnorm
    xs, rs, rel = [x], [r], [0.0 if bb == 0 else 1.0]
    it, status = 0, 1
    if not (np.isfinite(float(bb)) and np.isfinite(float(rz))):
        status = 2
    elif rnorm <= rel_tol * bnorm:
        status = 0
    else:
        while it < max_iters:
            q = ops.S(p)
            pq = ops.dot_pq(p, q)
            alpha = ops.div(rz, pq)
            if not (pq > 0) or not np.isfinite(float(alpha)):
                status = 2
                break
            x = ops.axpy(x, alpha, p)
            r = ops.axpy(r, -alpha, q)
            z = ops.precond(r)
            it += 1
            rr, rzn = ops.dot_rr(r, r, loop=True), ops.dot_rr(r, z)
            if not (np.isfinite(float(rr)) and np.isfinite(float(rzn))):
                status = 2
                break
            rnorm = ops.sqrt(rr)
            xs.append(x)
            rs.append(r)
            rel.append(rnorm / bnorm)
            if rnorm <= rel_tol * bnorm:
                status = 0
                break
            if it == max_iters:
                break
            p = ops.axpy(z, ops.div(rzn, rz) * beta_scale, p)
            rz = rzn
    return dict(xs=xs, rs=rs, rel=rel, status=status, iterations=it, rel_residual=0.0 if bb == 0 else rnorm / bnorm)


class _LDOps:
    """the loop's operations in longdouble through the implicit S_times / rhs; with rng, every operator output, vector
    update and dot product is moved by a random +-(its first-order scale) * 2^-52: one plausible f64 evaluation"""

    def __init__(self, P, lam, Minv, MScale, rng=None):
        self.P, self.lam, self.Minv, self.MScale, self.rng = P, lam, Minv, MScale, rng

    def _jig(self, v, scale):
        if self.rng is None:
            return v
        s = self.rng.choice(np.array([-1.0, 1.0]), size=np.shape(v)).astype(LD)
        return v + s * np.asarray(scale, dtype=LD) * LD(EPS)

    def zeros_like(self, v):
        return np.zeros_like(v)

    def sqrt(self, v):
        return np.sqrt(v)

    def div(self, a, b):
        return self._jig(a / b, abs(a / b))

    def rhs(self):
        b, s = self.P.rhs(self.lam)
        return self._jig(b, s)

    def S(self, p):
        y, s = self.P.S_times(self.lam, p)
        return self._jig(y, s)

    def precond(self, r):
        z = np.einsum("cab,cb->ca", self.Minv, r)
        return self._jig(z, np.einsum("cab,cb->ca", self.MScale, np.abs(z)))

    def _dot(self, a, b, loop=False):
        return self._jig(np.sum(a * b), np.sum(np.abs(a * b)))

    dot_pq = dot_rr = _dot

    def axpy(self, y, a, x):
        v = y + a * x
        return self._jig(v, np.abs(y) + np.abs(a * x))


def _pcg_ops(P, lam, rng=None):
    Ul = P.Ul(lam).astype(LD)
    L = chol_blocks(Ul)
    Minv = chol_inverse(L)
    # the first-order scale of a Cholesky solve: (M + dM) z = r with |dM| <= c u |L| |L^T|
    MScale = np.einsum("cij,cjk->cik", np.abs(Minv), np.einsum("cij,ckj->cik", np.abs(L), np.abs(L)))
    return _LDOps(P, lam, Minv, MScale, rng)


def energy(P, lam, x):
    """1/2 x^T S x - b^T x (longdouble), the quantity PCG lowers at every iterate"""
    x = np.asarray(x).reshape(P.n_cam, 9).astype(LD)
    Sx, _ = P.S_times(lam, x)
    b, _ = P.rhs(lam)
    return LD(0.5) * np.sum(x * Sx) - np.sum(b * x)


def pcg(P, lam, max_iters, rel_tol, runs=8, seed=0, mult=16.0, floor=1e-13):
    """The reference PCG on a longdouble Problem: c2b_problem_solve_step restated (pcg_loop) with M = the Cholesky factor
    of U_l,c per camera.  For every iterate k: x[k], dp[k] (back-substitution of x[k]), rel[k] = |r_k| / |b| and
    energy[k] = 1/2 x^T S x - b^T x (from the recurrence, -1/2 x^T (b + r)).  `runs` seeded reruns move every operator
    output and dot product by +-(first-order scale) * 2^-52; the bounds are `mult` x the largest deviation of each
    quantity from the unperturbed run, with a floor of `floor` x its size (x, dp, energy) or of 4 eps (rel)."""
    assert P.dtype == LD
    b, bscale = P.rhs(lam)
    base = pcg_loop(_pcg_ops(P, lam), max_iters, rel_tol)

    def derived(res, rng=None):
        xs = res["xs"]
        dps = [P.back_substitute(lam, x) for x in xs]
        dps = [d if rng is None else _LDOps(P, lam, None, None, rng)._jig(d, s) for d, s in dps]
        en = [-LD(0.5) * np.sum(x * (b + r)) for x, r in zip(xs, res["rs"])]
        return xs, dps, [LD(v) for v in res["rel"]], en

    xs, dps, rel, en = derived(base)
    n = len(xs)
    dev = dict(x=np.zeros(n), dp=np.zeros(n), rel=np.zeros(n), energy=np.zeros(n))
    rng = np.random.default_rng(seed)
    for _ in range(runs):
        res = pcg_loop(_pcg_ops(P, lam, rng), max_iters, rel_tol)
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
