"""Host reference of per-camera Levenberg-Marquardt (BAProblem.refine_cameras) in numpy.longdouble, its float64
twin, and the bounds its tests use.  numpy only: nothing here touches a device.  The pattern is tests/_refineref.py's, with
the cameras for the points and 9 for 3.

Every camera is minimised by itself with the points held.  Its parameters are q = bal9[c] (to_vec order).  Per observation r
and Jc come from tests/_jacref.py (reference_bal, longdouble), rho and w = rho' from tests/_refineref.py (_rho_w), the prior
rows from tests/_priorref.py (camera_rows on R = exp([w]x), J_l(w), C = -R^T t).  A walk at q gives
    F = sum rho(|r|^2) + |w_C o (C - C0)|^2 + |w_I o ((f, k1, k2) - I0)|^2,
    U = sum w Jc^T Jc + A^T A,   g = sum w Jc^T r + A^T r_prior,
then the rows and columns of U and the entries of g of the constant parameters are zeroed (F is not masked).  Round k is
_refineref's with a 9x9 Cholesky written here (solve9): gradient test, the damped step (a constant entry's delta is exactly 0:
its row is zero but for the damped diagonal mu 1e-6, its right-hand side 0), parameter test over the nine entries, the trial
walk at q + delta, Nielsen's acceptance and update.

`dtype`: np.longdouble is the reference, np.float64 its *float64 twin* -- r and Jc formed in f64 in the kernel's order
(_jacref.kernel_f64), scaled by sqrt(w) before the products as the kernel scales them, the prior rows formed in f64 from the
f64 record (R = from_rodrigues, J_l, C = -R^T t; prior_center_rows' expressions), and every sum, solve and comparison in
f64.  The order of an f64 sum is the twin's to choose, and no order is more valid than another: Problem.order names it
(ORDERS: "lanes16", the kernel's own -- sixteen strided partial sums and the xor tree --, "sequential", "reverse" and
"pairwise").  A margin measured on the twin is the worst over ORDERS, so that it measures f64 rounding and not the luck of
one order.  Margins are measured against the twin, never against the device.

B is _refineref's rounding bound on F, sum |terms| 2^-52 (depth + 16) with depth = the observations and the priors' six rows,
and the same floor for a cost that f64 residuals cannot tell from 0."""
import numpy as np

import _jacref as J
import _priorref as PR
from _refineref import (COUNTS, CONSTANT, CONVERGED, EPS, FAILED, KINDS, LAMBDA_MAX, LAMBDA_MIN, LD, MAX_ROUNDS, STATUS, UNOBSERVED,
                        WEIGHT_OPS, _rho_w)

ALL = 0x1ff
PRIOR_ROWS = 6
ORDERS = ("lanes16", "sequential", "reverse", "pairwise")     # the f64 twin's summation orders over a camera's row


def _row_sums(terms, cam_of, count, n, order):
    """per camera, the f64 sum of its row's terms [n_obs, ...] in the named order"""
    shape = terms.shape[1:]
    if order == "sequential" or order == "reverse":
        out = np.zeros((n,) + shape, dtype=terms.dtype)
        idx = np.arange(len(cam_of))
        if order == "reverse":
            idx = idx[::-1]
        np.add.at(out, cam_of[idx], terms[idx])
        return out
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    k = np.arange(len(cam_of)) - start[cam_of]                 # an observation's place in its row
    if order == "lanes16":                                   # lane l: observations l, l + 16, ... in turn; then the xor tree
        part = np.zeros((n * 16,) + shape, dtype=terms.dtype)
        np.add.at(part, cam_of * 16 + k % 16, terms)
        part = part.reshape((n, 16) + shape)
        lanes = np.arange(16)
        for off in (8, 4, 2, 1):
            part = part + part[:, lanes ^ off]
        return part[:, 0]
    if order == "pairwise":                                  # a balanced tree over the row, padded with zeros
        width = 1
        while width < max(int(count.max()) if len(count) else 1, 1):
            width *= 2
        part = np.zeros((n, width) + shape, dtype=terms.dtype)
        part[cam_of, k] = terms
        while part.shape[1] > 1:
            part = part[:, 0::2] + part[:, 1::2]
        return part[:, 0]
    raise ValueError("order %r" % (order,))


class Problem:
    """pts [n_pts, 3]; the list camera-major (row_ptr, pt_idx, uv); loss by name with its scale; center = (C0 [n_cam, 3], w_C
    [n_cam, 3]) and intr = (I0, w_I) or None; mask [n_cam] of C2B_CONST_* bits (bit k: parameter k constant) or None"""

    def __init__(self, pts, row_ptr, pt_idx, uv, loss=None, loss_scale=1.0, center=None, intr=None, mask=None, order="lanes16"):
        self.order = order                                   # of the float64 twin's sums (ORDERS); the reference has none
        self.pts = np.asarray(pts, dtype=np.float64)
        row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.n_cam = len(row_ptr) - 1
        self.count = np.diff(row_ptr)
        self.cam_of = np.repeat(np.arange(self.n_cam), self.count)
        self.pt = np.asarray(pt_idx).astype(np.int64)
        self.uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
        self.kind, self.a = KINDS[loss], float(loss_scale)
        self.mask = np.zeros(self.n_cam, dtype=np.int64) if mask is None else np.asarray(mask).astype(np.int64) & ALL
        self.const = ((self.mask[:, None] >> np.arange(9)[None, :]) & 1).astype(bool)                  # [n_cam, 9]
        n = self.n_cam

        def pair(p):
            if p is None:
                return np.zeros((n, 3)), np.zeros((n, 3))
            w = np.asarray(p[1], dtype=np.float64)
            return np.where(w != 0.0, np.asarray(p[0], dtype=np.float64), 0.0), w                      # a target under weight 0 is never read
        self.c0, self.cw = pair(center)
        self.i0, self.iw = pair(intr)
        self.observed = (self.count > 0) | np.any(self.cw != 0.0, axis=1) | np.any(self.iw != 0.0, axis=1)

    def observations(self, q, dtype=LD):
        """(r [n_obs, 2], Jc [n_obs, 2, 9]) at the parameters q [n_cam, 9]; self.mag [n_obs, 2] (f64) = |u| + |o|; with
        dtype float64 also self.Er, self.Ec: the kernel's running bounds on r and Jc"""
        cams = np.asarray(q)[self.cam_of]
        X = self.pts[self.pt]
        with np.errstate(all="ignore"):
            if np.dtype(dtype) == np.float64:
                cams = np.asarray(cams, dtype=np.float64)
                jc, jp, aux = J.kernel_f64("bal", cams, X)
                f = J.V(cams[:, 6])
                u0, u1 = f * aux["rad"] * aux["px"], f * aux["rad"] * aux["py"]
                u = np.stack([u0.v, u1.v], axis=1)
                self.Er = np.stack([u0.e, u1.e], axis=1)
                Jc, self.Ec = J.stack(jc, jp)[:2]
                self.mag = np.abs(u) + np.abs(self.uv)
                return u - self.uv, Jc
            ref = J.reference_bal(cams, X, self.uv)
            self.mag = (np.abs(ref["uv"]) + np.abs(self.uv)).astype(np.float64)
        return ref["r"], ref["Jc"]

    def prior_rows(self, q, dtype=LD):
        """(r [n_cam, 6], A [n_cam, 6, 9]) at q: in longdouble, or (dtype float64, the twin) formed in f64 from the f64 record
        with prior_center_rows' expressions"""
        if np.dtype(dtype) == np.float64:
            return self._prior_rows_f64(np.asarray(q, dtype=np.float64))
        q = np.asarray(q).astype(LD)
        w, t = q[:, 0:3], q[:, 3:6]
        R = J.exp_so3(w)
        rows = PR.camera_rows(R, t, J.left_jacobian_ld(w), q[:, 6:9], PR.center(R, t), self.c0, self.cw, self.i0, self.iw)
        return rows["r"], PR.full_camera_jacobian(rows["A"], self.iw)

    def _prior_rows_f64(self, q):
        n = len(q)
        with np.errstate(all="ignore"):
            Rcm = [x.v for x in J.from_rodrigues(*(J.V(q[:, k]) for k in range(3)))]
            R = np.stack([Rcm[3 * (i % 3) + i // 3] for i in range(9)], axis=1).reshape(n, 3, 3)      # row-major, as the record
            Jl = np.stack([x.v for x in J.left_jacobian(*(J.V(q[:, k]) for k in range(3)))], axis=1).reshape(n, 3, 3)
            t = q[:, 3:6]
            C = np.stack([-((R[:, 0, k] * t[:, 0] + R[:, 1, k] * t[:, 1]) + R[:, 2, k] * t[:, 2]) for k in range(3)], axis=1)
            r = np.zeros((n, 6))
            A = np.zeros((n, 6, 9))
            r[:, :3] = np.where(self.cw != 0.0, self.cw * (C - self.c0), 0.0)
            r[:, 3:] = np.where(self.iw != 0.0, self.iw * (q[:, 6:9] - self.i0), 0.0)
            for j in range(3):
                j0, j1, j2 = Jl[:, 0, j], Jl[:, 1, j], Jl[:, 2, j]
                m0, m1, m2 = t[:, 1] * j2 - t[:, 2] * j1, t[:, 2] * j0 - t[:, 0] * j2, t[:, 0] * j1 - t[:, 1] * j0
                for k in range(3):
                    A[:, k, j] = -(self.cw[:, k] * ((R[:, 0, k] * m0 + R[:, 1, k] * m1) + R[:, 2, k] * m2))
                    A[:, k, 3 + j] = -(self.cw[:, k] * R[:, j, k])
            for m in range(3):
                A[:, 3 + m, 6 + m] = self.iw[:, m]
        return r, A

    def walk(self, q, dtype=LD, linear=True):
        """dict(F [n_cam], B [n_cam] (f64), U [n_cam, 9, 9], g [n_cam, 9]) in dtype at q [n_cam, 9]"""
        q = np.asarray(q).astype(dtype)
        n = self.n_cam
        with np.errstate(all="ignore"):
            if len(self.pt):
                r, Jc = self.observations(q, dtype)
                s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
                rho, w = _rho_w(self.kind, self.a, s)
            else:
                r, Jc, rho, w = np.zeros((0, 2), dtype), np.zeros((0, 2, 9), dtype), np.zeros(0, dtype), np.zeros(0, dtype)
            f64 = np.dtype(dtype) == np.float64
            if f64:
                F = _row_sums(rho, self.cam_of, self.count, n, self.order)
            else:
                F = np.zeros(n, dtype=dtype)
                np.add.at(F, self.cam_of, rho)
            rp, A = self.prior_rows(q, dtype)
            rp, A = rp.astype(dtype), A.astype(dtype)
            F = F + ((rp[:, 0] * rp[:, 0] + rp[:, 1] * rp[:, 1]) + rp[:, 2] * rp[:, 2])
            F = F + ((rp[:, 3] * rp[:, 3] + rp[:, 4] * rp[:, 4]) + rp[:, 5] * rp[:, 5])
            B = np.abs(F).astype(np.float64) * EPS * (self.count + PRIOR_ROWS + 16.0)
            floor = np.zeros(n)
            if len(self.pt):
                e = self.mag * (16.0 * EPS)
                np.add.at(floor, self.cam_of, np.sum(e * e, axis=1))
            qf = q.astype(np.float64)
            wts = np.concatenate([self.cw, self.iw], axis=1)
            # a prior row w (x - x0) formed in f64 is off by about w (|x| + |x0|) 16 eps; |C| <= |t| for the centre's rows
            mags = np.concatenate([np.linalg.norm(qf[:, 3:6], axis=1)[:, None] + np.abs(self.c0), np.abs(qf[:, 6:9]) + np.abs(self.i0)], axis=1)
            ep = wts * mags * (16.0 * EPS)
            B = np.maximum(B, floor + np.sum(ep * ep, axis=1))
            out = dict(F=F, B=B)
            if linear:
                if f64:                                      # (r, Jc) *= sqrt(w), then the products, as loss_scale_obs and the kernel
                    sw = np.sqrt(w)
                    Js, rs = Jc * sw[:, None, None], r * sw[:, None]
                    U = _row_sums(Js[:, 0, :, None] * Js[:, 0, None, :] + Js[:, 1, :, None] * Js[:, 1, None, :], self.cam_of, self.count, n, self.order)
                    g = _row_sums(Js[:, 0] * rs[:, 0, None] + Js[:, 1] * rs[:, 1, None], self.cam_of, self.count, n, self.order)
                else:
                    U = np.zeros((n, 9, 9), dtype=dtype)
                    g = np.zeros((n, 9), dtype=dtype)
                    np.add.at(U, self.cam_of, w[:, None, None] * np.einsum("nia,nib->nab", Jc, Jc))
                    np.add.at(g, self.cam_of, w[:, None] * np.einsum("nia,ni->na", Jc, r))
                U = U + np.einsum("nka,nkb->nab", A, A)
                g = g + np.einsum("nka,nk->na", A, rp)
                free = ~self.const
                U = np.where(free[:, :, None] & free[:, None, :], U, 0)
                g = np.where(free, g, 0)
                out.update(U=U.astype(dtype), g=g.astype(dtype))
        return out

    def cost(self, q):
        """(F, B): the longdouble cost of every camera at q and its rounding bound"""
        o = self.walk(q, LD, linear=False)
        return o["F"], o["B"]


def solve9(U, g, mu):
    """(delta, ok): (U + mu diag(d)) delta = -g by a 9x9 Cholesky in U's dtype, d = clamp(diag U, 1e-6, 1e32); ok = every
    pivot is positive and delta is finite"""
    T = U.dtype.type
    n = len(U)
    idx = np.arange(9)
    with np.errstate(all="ignore"):
        A = U.copy()
        d = np.minimum(np.maximum(U[:, idx, idx], T(1e-6)), T(1e32))
        A[:, idx, idx] += mu[:, None] * d
        Lm = np.zeros_like(A)
        ok = np.ones(n, dtype=bool)
        for j in range(9):
            p = A[:, j, j] - np.sum(Lm[:, j, :j] * Lm[:, j, :j], axis=1)
            ok &= p > 0
            Lm[:, j, j] = np.sqrt(p)
            for i in range(j + 1, 9):
                Lm[:, i, j] = (A[:, i, j] - np.sum(Lm[:, i, :j] * Lm[:, j, :j], axis=1)) / Lm[:, j, j]
        b = -g
        y = np.zeros_like(b)
        for i in range(9):
            y[:, i] = (b[:, i] - np.sum(Lm[:, i, :i] * y[:, :i], axis=1)) / Lm[:, i, i]
        x = np.zeros_like(b)
        for i in range(8, -1, -1):
            x[:, i] = (y[:, i] - np.sum(Lm[:, i + 1:, i] * x[:, i + 1:], axis=1)) / Lm[:, i, i]
        ok &= np.all(np.isfinite(x), axis=1)
    return x, ok


def refine(P, q, rounds=10, lam=1e-4, function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0, dtype=LD):
    """The per-camera loop on Problem P from the parameters q [n_cam, 9] (f64).  Returns dict(q [n_cam, 9] (dtype; the input's
    values where nothing moved), status [n_cam] uint8, moved [n_cam] bool, counts (COUNTS -> int), F0, F (dtype), B (f64: the
    bound on F at the end), rounds: one dict per round with F, Ft (F'), B, Bt, delta, model, accepted, tried, mu -- NaN / False
    for a camera that was not running)."""
    T = np.dtype(dtype).type
    n = P.n_cam
    q = np.asarray(q, dtype=np.float64).astype(dtype)
    const_all = P.mask == ALL
    status = np.full(n, MAX_ROUNDS, dtype=np.uint8)
    status[~P.observed] = UNOBSERVED
    status[const_all] = CONSTANT
    cur = P.walk(q, dtype)
    cand = P.observed & ~const_all
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
            delta, ok = solve9(cur["U"], cur["g"], mu)
            ok = ok & live
            if parameter_tol > 0.0:
                dn = np.sqrt(np.sum(delta * delta, axis=1))
                xn = np.sqrt(np.sum(q * q, axis=1))
                done = ok & (dn <= T(parameter_tol) * (xn + T(parameter_tol)))
                status[done] = CONVERGED
                live, ok = live & ~done, ok & ~done
            qt = np.where(ok[:, None] & ~P.const, q + delta, q)
            tri = P.walk(qt, dtype)
            Ud = np.einsum("pab,pb->pa", cur["U"], delta)
            model = -(T(2) * np.sum(cur["g"] * delta, axis=1) + np.sum(delta * Ud, axis=1))
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
            q = np.where(acc[:, None], qt, q)
            for k in ("F", "B", "U", "g"):
                sel = acc.reshape((-1,) + (1,) * (cur[k].ndim - 1))
                cur[k] = np.where(sel, tri[k], cur[k])
            moved |= acc
            status[small] = CONVERGED
            live = live & ~small
    counts = dict(zip(STATUS, (int(v) for v in np.bincount(status, minlength=5))))
    counts["moved"] = int(moved.sum())
    return dict(q=q, status=status, moved=moved, counts=counts, F0=F0, F=cur["F"], B=cur["B"], rounds=hist)


def step_tolerance(P, q, mu):
    """Per camera, the tolerance on the first round's delta of an f64 evaluation in the device's arithmetic, to first order:
    cond(U_mu) (|dU| / |U_mu| + |dg| / |g|) |delta| with U_mu = U + mu diag(d) of the longdouble reference -- _refineref's
    construction with 9 for 3: dU, dg = _normref.bound at the weighting's operation count (any f64 summation order of the
    products, the priors' own terms among them) plus the kernel's running bounds on r and Jc (_jacref, with its margin C)
    propagated through the products.  Returns (tol [n_cam] f64, delta [n_cam, 9] longdouble, ok [n_cam])."""
    import _normref as NR
    n = P.n_cam
    cur = P.walk(q, LD)
    delta, ok = solve9(cur["U"], cur["g"], np.full(n, LD(mu)))
    with np.errstate(all="ignore"):
        SU, Sg, EU, Eg = np.zeros((n, 9, 9)), np.zeros((n, 9)), np.zeros((n, 9, 9)), np.zeros((n, 9))
        if len(P.pt):
            r, Jc = P.observations(np.asarray(q, dtype=np.float64), np.float64)
            s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
            _, w = _rho_w(P.kind, P.a, s)
            sw = np.sqrt(w)
            aJ, ar = np.abs(Jc) * sw[:, None, None], np.abs(r) * sw[:, None]
            Ec, Er = P.Ec * sw[:, None, None], P.Er * sw[:, None]
            np.add.at(SU, P.cam_of, np.einsum("nia,nib->nab", aJ, aJ))
            np.add.at(Sg, P.cam_of, np.einsum("nia,ni->na", aJ, ar))
            np.add.at(EU, P.cam_of, np.einsum("nia,nib->nab", aJ, Ec) + np.einsum("nia,nib->nab", Ec, aJ))
            np.add.at(Eg, P.cam_of, np.einsum("nia,ni->na", aJ, Er) + np.einsum("nia,ni->na", Ec, ar))
        rp, A = P.prior_rows(q)
        aA, arp = np.abs(A).astype(np.float64), np.abs(rp).astype(np.float64)
        SU += np.einsum("nka,nkb->nab", aA, aA)
        Sg += np.einsum("nka,nk->na", aA, arp)
        # the prior rows' own entries in the device's f64: _priorref's operation counts, the largest of them (7 roundings)
        EA, Erp = PR.DEVICE_OPS_DW * PR.U53 * aA, PR.DEVICE_OPS_R * PR.U53 * arp
        EU += np.einsum("nka,nkb->nab", aA, EA) + np.einsum("nka,nkb->nab", EA, aA)
        Eg += np.einsum("nka,nk->na", aA, Erp) + np.einsum("nka,nk->na", EA, arp)
        depth = P.count + PRIOR_ROWS + WEIGHT_OPS
        dU = NR.bound(SU, depth) + J.C * EU
        dg = NR.bound(Sg, depth) + J.C * Eg
        free = ~P.const
        dU = np.where(free[:, :, None] & free[:, None, :], dU, 0.0)
        dg = np.where(free, dg, 0.0)
        A_ = cur["U"].astype(np.float64).copy()
        idx = np.arange(9)
        A_[:, idx, idx] += float(mu) * np.clip(A_[:, idx, idx], 1e-6, 1e32)
        good = ok & np.all(np.isfinite(A_.reshape(n, -1)), axis=1)
        sv = np.ones((n, 9))
        sv[good] = np.linalg.svd(A_[good], compute_uv=False)
        cond = sv[:, 0] / sv[:, -1]
        gn = np.linalg.norm(cur["g"].astype(np.float64), axis=1)
        rel = np.linalg.norm(dU.reshape(n, -1), axis=1) / sv[:, 0] + np.where(gn > 0, np.linalg.norm(dg, axis=1) / np.where(gn > 0, gn, 1.0), 0.0)
        tol = cond * rel * np.linalg.norm(delta.astype(np.float64), axis=1)
    return tol, delta, ok


def borderline(ref_round):
    """cameras whose reference round lies inside the cost's rounding bound: |F - F'| <= B(F) + B(F'), or whose step could not
    be solved -- their accept decision is not compared"""
    with np.errstate(all="ignore"):
        gap = np.abs((ref_round["F"] - ref_round["Ft"]).astype(np.float64))
    return ref_round["tried"] & ~(gap > ref_round["Bt"] + ref_round["B"])


# ---- the problems --------------------------------------------------------------------------------------------------------
EXTRA_ROWS = (15, 16, 17, 31, 32, 33)                        # the edges of the 16-lane ownership, appended to the dome's rows
START_ROTATION, START_TRANSLATION = 0.02, 0.05               # the displaced start of the poses


def dome(obs_noise, seed=17):
    """tests/_problems.py's dome_problem (81 cameras: a workgroup tail and a partial camblk group; rows of 0, 1 .. 5, 8, 63, 64,
    65, 127, 130, 257 observations among them; k2 = 0 on every fifth camera) with six more cameras, copies of the six cameras
    with the longest rows, their rows cut to EXTRA_ROWS observations; the true points; pixels with obs_noise; every pose started START_ROTATION /
    START_TRANSLATION from the truth in seeded directions.  Returns dict(bal9, cams15, true_bal9, pts, row_ptr, pt_idx, uv)."""
    import oracle as O
    from _problems import dome_problem
    D = dome_problem(seed=0, dup=True, state=False, obs_noise=obs_noise, start_noise=0.0)
    rp = np.asarray(D["row_ptr"], dtype=np.int64)
    true = np.array(D["true_bal9"], dtype=np.float64)
    pt_idx, uv = np.asarray(D["pt_idx"]), np.asarray(D["uv"], dtype=np.float64).reshape(-1, 2)
    pts = np.array(D["true_pts"], dtype=np.float64)
    lens = np.diff(rp)
    donors = [int(c) for c in np.argsort(-lens, kind="stable") if lens[c] >= max(EXTRA_ROWS)][:len(EXTRA_ROWS)]
    assert len(donors) == len(EXTRA_ROWS)
    add_idx, add_uv, add_len = [], [], []
    for c, m in zip(donors, EXTRA_ROWS):
        add_idx.append(pt_idx[rp[c]:rp[c] + m])
        add_uv.append(uv[rp[c]:rp[c] + m])
        add_len.append(m)
    true = np.vstack([true, true[donors]])
    row_ptr = np.concatenate([rp, rp[-1] + np.cumsum(add_len)]).astype(np.uint64)
    pt_idx = np.concatenate([pt_idx] + add_idx).astype(np.uint64)
    uv = np.vstack([uv] + add_uv)
    cams15_true = O.camera_from_bal(true)
    rng = np.random.default_rng(seed + 1)
    uv = O.project_observations(cams15_true, pts, row_ptr, pt_idx) + (rng.normal(scale=obs_noise, size=uv.shape) if obs_noise else 0.0)
    g = np.random.default_rng(seed).normal(size=(len(true), 2, 3))
    g = g / np.linalg.norm(g, axis=2)[:, :, None]
    bal9 = true.copy()
    bal9[:, 0:3] += START_ROTATION * g[:, 0]
    bal9[:, 3:6] += START_TRANSLATION * g[:, 1]
    return dict(bal9=bal9, cams15=O.camera_from_bal(bal9), true_bal9=true, pts=pts, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv)


def dome_priors(P, seed=3):
    """centre and intrinsics priors for dome(): targets near the truth, weights that differ per component, every fourth camera
    without a centre prior (weights 0, NaN targets), every third without an intrinsics prior, one component of weight 0 with a
    NaN target in the others"""
    import oracle as O
    rng = np.random.default_rng(seed)
    n = len(P["bal9"])
    c15 = O.camera_from_bal(P["true_bal9"])
    R = c15[:, :9].reshape(-1, 3, 3).swapaxes(1, 2)
    C = -np.einsum("nik,ni->nk", R, c15[:, 9:12])
    c0 = C + rng.normal(scale=0.01, size=(n, 3))
    cw = rng.uniform(0.5, 2.0, size=(n, 3))
    i0 = P["true_bal9"][:, 6:9] + rng.normal(scale=1e-3, size=(n, 3))
    iw = rng.uniform(1.0, 5.0, size=(n, 3))
    cw[::4] = 0.0
    c0[::4] = np.nan
    iw[::3] = 0.0
    i0[::3] = np.nan
    cw[1::4, 1] = 0.0
    c0[1::4, 1] = np.nan
    iw[1::3, 2] = 0.0
    i0[1::3, 2] = np.nan
    return dict(center=(c0, cw), intr=(i0, iw))


def intrinsics_mask(n):
    """f, k1, k2 held on every third camera"""
    m = np.zeros(n, dtype=np.uint16)
    m[::3] = 0x1c0
    return m


def of(P, **kw):
    return Problem(P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], **kw)


def twin_worst_ratio(Q, q0, ref_q, rounds, run, **kw):
    """the float64 twin's worst (F_ld(q_twin) - F_ld(q_ref)) / B over the cameras `run`, the worst over ORDERS: (worst, dict
    order -> its worst).  Q's own order is put back."""
    Fr, B = Q.cost(ref_q)
    keep, per = Q.order, {}
    try:
        for order in ORDERS:
            Q.order = order
            Ft, _ = Q.cost(refine(Q, q0, rounds=rounds, dtype=np.float64, **kw)["q"])
            with np.errstate(all="ignore"):
                per[order] = float(np.max(((Ft - Fr).astype(np.float64) / B)[run]))
    finally:
        Q.order = keep
    return max(per.values()), per


def hand_placed():
    """Six cameras of dome(0) over its points: camera 0 as it is (MAX_ROUNDS), 1 with all nine parameters constant (CONSTANT;
    its parameters are NaN: nothing of it is read), 2 with an empty row and no prior (UNOBSERVED), 3 starting at NaN (FAILED),
    4 with an empty row and a centre prior on its translation (the rotation constant: pulled onto its target), 5 with its pose
    constant.  Returns (P, mask, priors)."""
    D = dome(0.0)
    rp = np.asarray(D["row_ptr"], dtype=np.int64)
    lens = np.diff(rp)
    pick = [int(c) for c in np.flatnonzero(lens >= 12)[:6]]
    keep_rows = [True, True, False, True, False, True]
    bal9 = D["bal9"][pick].copy()
    idx, uv, n = [], [], []
    for c, k in zip(pick, keep_rows):
        sl = slice(rp[c], rp[c] + (12 if k else 0))
        idx.append(D["pt_idx"][sl])
        uv.append(D["uv"][sl])
        n.append(12 if k else 0)
    bal9[1] = np.nan
    bal9[3, 0] = np.nan
    mask = np.array([0, 0x1ff, 0, 0, 0x007, 0x03f], dtype=np.uint16)
    c0, cw = np.full((6, 3), np.nan), np.zeros((6, 3))
    c0[4], cw[4] = [1.0, -2.0, 3.0], [2.0, 1.0, 0.5]
    P = dict(bal9=bal9, pts=D["pts"], row_ptr=np.concatenate([[0], np.cumsum(n)]).astype(np.uint64),
             pt_idx=np.concatenate(idx).astype(np.uint64), uv=np.vstack(uv))
    return P, mask, dict(center=(c0, cw), intr=None)
