"""Host reference of the explicit Schur complement on a tests/_schurref.py Problem, restated from the definition
in the Problem's dtype (longdouble works).  With W_o = Jc_o^T Jp_o (9x3; the Problem's Jacobian already carries a loss's
sqrt(w) and a mask's zeros) and Ws(c, p) = the sum of W_o over the observations of the pair (c, p):
  pattern   the covisibility graph of the list at min_shared = 1 (_covisref.graph) plus the diagonal;
  S_e    = - sum_{p seen by both} Ws(c, p) V_l,p^-1 Ws(c', p)^T                 for an edge e = (c, c');
  S_cc   = U_l,c - sum_p Ws(c, p) V_l,p^-1 Ws(c, p)^T                            (S's own diagonal: a duplicated pair's cross terms are in),
each with the absolute-value scale of its sum.  With rng every intermediate is moved by +-(its first-order absolute scale) *
2^-52, one plausible f64 evaluation, by the model of _precondref._damped_inverse / blocks: V and its backward-stable solve, the
pair sums, every term, every block's sum.  blocks_bound turns 8 such reruns into the bound a device block is held to, and
pcg is _precondref.pcg with an operator that multiplies by the (perturbed) stored blocks, so that its bounds describe the
explicit arithmetic.  numpy only."""
import numpy as np

import _covisref as CR
import _precondref as PR
import _schurref as R

LD, EPS = R.LD, R.EPS
_jig = PR._jig


def row_ptr_of(P):
    """the camera-major row pointer of the Problem's list"""
    return np.concatenate([[0], np.cumsum(np.bincount(P.cam, minlength=P.n_cam))]).astype(np.uint64)


def pattern(P):
    """(nbr_ptr [n_cam + 1] uint64, nbr [n_edges] uint32) of S's off-diagonal blocks.  The Problem's rows need not be in camera
    order (a stacked system appends its priors' rows, each on a (camera, point) pair of the list): they are put in it first."""
    nbr_ptr, nbr, _ = CR.graph(row_ptr_of(P), P.pt[np.argsort(P.cam, kind="stable")], 1)
    return nbr_ptr, nbr


def _edge_ids(nbr_ptr, nbr, n_cam):
    eid = np.full((n_cam, n_cam), -1, dtype=np.int64)
    row = np.repeat(np.arange(n_cam), np.diff(nbr_ptr.astype(np.int64)))
    eid[row, nbr.astype(np.int64)] = np.arange(len(nbr))
    return eid, row


def blocks(P, lam, rng=None):
    """dict(nbr_ptr, nbr, D [n_cam, 9, 9], SD, E [n_edges, 9, 9], SE): the definition, pair by pair, and the absolute-value scale of
    every block's sum (|Ws| (|V_l^-1| + its first-order error) |Ws'|^T summed; the diagonal also SU and the damping's own entries)"""
    nbr_ptr, nbr = pattern(P)
    eid, _ = _edge_ids(nbr_ptr, nbr, P.n_cam)
    Vi, SVi = PR._damped_inverse(P, lam, rng)
    aVi = np.abs(Vi)
    # the pairs (point, camera) in that order, and each pair's sum of W over its observations
    key = P.pt * P.n_cam + P.cam
    order = np.argsort(key, kind="stable")
    new = np.concatenate([[True], key[order][1:] != key[order][:-1]]) if len(key) else np.zeros(0, dtype=bool)
    first = np.flatnonzero(new)
    gid = np.empty(len(key), dtype=np.int64)
    gid[order] = np.cumsum(new) - 1
    gp, gc = P.pt[order][first], P.cam[order][first]
    aW = np.einsum("nia,nib->nab", P.aJc, P.aJp)
    W = _jig(P.W, aW, rng)
    Ws, aWs = np.zeros((len(first), 9, 3), dtype=P.dtype), np.zeros((len(first), 9, 3), dtype=P.dtype)
    np.add.at(Ws, gid, W)
    np.add.at(aWs, gid, aW)
    Ws = _jig(Ws, aWs, rng)
    Ul = P.Ul(lam)
    if rng is not None:
        Ul = _jig(Ul, P.SU + (Ul - P.U), rng)
        Ul = (Ul + Ul.transpose(0, 2, 1)) / 2
    D, SD = Ul.copy(), P.SU + (P.Ul(lam) - P.U)
    E, SE = np.zeros((len(nbr), 9, 9), dtype=P.dtype), np.zeros((len(nbr), 9, 9), dtype=P.dtype)
    RD, RE = np.zeros_like(D), np.zeros_like(E)                  # what the sums round at: the terms' own absolute values
    start = np.flatnonzero(np.concatenate([[True], gp[1:] != gp[:-1]])) if len(gp) else np.empty(0, dtype=np.int64)
    for a, b in zip(start, np.concatenate([start[1:], [len(gp)]])):
        p, cams = gp[a], gc[a:b]
        T = -np.einsum("iab,bc,jdc->ijad", Ws[a:b], Vi[p], Ws[a:b])
        aT = np.einsum("iab,bc,jdc->ijad", aWs[a:b], aVi[p], aWs[a:b])
        sT = np.einsum("iab,bc,jdc->ijad", aWs[a:b], aVi[p] + SVi[p], aWs[a:b])
        T = _jig(T, aT, rng)
        i = np.arange(len(cams))
        np.add.at(D, cams, T[i, i])
        np.add.at(SD, cams, sT[i, i])
        np.add.at(RD, cams, aT[i, i])
        ii, jj = np.nonzero(~np.eye(len(cams), dtype=bool))
        e = eid[cams[ii], cams[jj]]
        assert (e >= 0).all()
        np.add.at(E, e, T[ii, jj])
        np.add.at(SE, e, sT[ii, jj])
        np.add.at(RE, e, aT[ii, jj])
    D, E = _jig(D, RD + np.abs(Ul), rng), _jig(E, RE, rng)
    return dict(nbr_ptr=nbr_ptr, nbr=nbr, D=D, SD=SD, E=E, SE=SE)


def blocks_bound(P, lam, runs=8, seed=0, mult=16.0, floor=1e-13):
    """The longdouble blocks and, per block, the bound an f64 evaluation is held to in the Frobenius norm: `mult` x the largest
    deviation over `runs` seeded perturbed reruns, floored at `floor` x the norm of the absolute-value scale of its sum --
    _precondref.blocks_bound's rule.  Returns blocks()'s dict plus bound_D [n_cam] and bound_E [n_edges]."""
    assert P.dtype == LD
    ref = blocks(P, lam)
    rng = np.random.default_rng(seed)
    dev_D, dev_E = np.zeros(P.n_cam), np.zeros(len(ref["nbr"]))
    norm = lambda A: np.linalg.norm(A.astype(np.float64), axis=(1, 2)) if len(A) else np.zeros(0)
    for _ in range(runs):
        per = blocks(P, lam, rng)
        dev_D = np.maximum(dev_D, norm(per["D"] - ref["D"]))
        dev_E = np.maximum(dev_E, norm(per["E"] - ref["E"]))
    ref["bound_D"] = np.maximum(mult * dev_D, floor * norm(ref["SD"]))
    ref["bound_E"] = np.maximum(mult * dev_E, floor * norm(ref["SE"]))
    return ref


def dense(ref, n_cam):
    """the blocks assembled into S [9 n_cam, 9 n_cam] (float64)"""
    S = np.zeros((9 * n_cam, 9 * n_cam))
    _, row = _edge_ids(ref["nbr_ptr"], ref["nbr"], n_cam)
    for c in range(n_cam):
        S[9 * c:9 * c + 9, 9 * c:9 * c + 9] = ref["D"][c].astype(np.float64)
    for e, (c, q) in enumerate(zip(row, ref["nbr"].astype(np.int64))):
        S[9 * c:9 * c + 9, 9 * q:9 * q + 9] = ref["E"][e].astype(np.float64)
    return S


def spmv(nbr_ptr, nbr, D, E, x):
    """(y, scale): y_c = D_c x_c + sum_e E_e x_nbr(e) in the arrays' dtype and the absolute-value scale of that sum"""
    n_cam = len(D)
    row = np.repeat(np.arange(n_cam), np.diff(np.asarray(nbr_ptr).astype(np.int64)))
    col = np.asarray(nbr).astype(np.int64)
    y = np.einsum("cab,cb->ca", D, x)
    s = np.einsum("cab,cb->ca", np.abs(D), np.abs(x))
    if len(col):
        np.add.at(y, row, np.einsum("eab,eb->ea", E, x[col]))
        np.add.at(s, row, np.einsum("eab,eb->ea", np.abs(E), np.abs(x[col])))
    return y, s


class _ExplicitOps(R._LDOps):
    """_schurref._LDOps whose operator multiplies by the stored blocks; under rng the blocks are themselves one perturbed
    evaluation, made once (the device builds S once per solve), and every product rounds at the scale of its own sum"""

    def __init__(self, P, lam, Minv, MScale, rng=None):
        super().__init__(P, lam, Minv, MScale, rng)
        self.B = blocks(P, lam, rng)

    def S(self, p):
        y, s = spmv(self.B["nbr_ptr"], self.B["nbr"], self.B["D"], self.B["E"], p)
        return self._jig(y, s)


def _ops(P, lam, kind, rng=None):
    base = PR._ops(P, lam, kind, rng)
    return _ExplicitOps(P, lam, base.Minv, base.MScale, rng)


def pcg(P, lam, max_iters, rel_tol, kind="block_jacobi", runs=8, seed=0, mult=16.0, floor=1e-13):
    """_precondref.pcg (its text) with _ops above in place of its own: the same iterates' quantities, the same seeded reruns,
    the same rule for the bounds, the operator being the explicit one"""
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
