"""Extended-precision reference of the robust losses of the step (BAProblem.set_loss).  Per observation
s = r0^2 + r1^2, rho(s) with scale a > 0 (Ceres' definitions) and the weight w = rho'(s):
    0 squared   rho = s                                       w = 1
    1 Huber     rho = s (s <= a^2), else 2 a sqrt(s) - a^2    w = 1 (s <= a^2), else a / sqrt(s)
    2 Cauchy    rho = a^2 log1p(s / a^2)                      w = 1 / (1 + s / a^2)
    3 soft-L1   rho = 2 a^2 (sqrt(1 + s / a^2) - 1)           w = 1 / sqrt(1 + s / a^2)
The step is iteratively reweighted least squares: problem() hands sqrt(w) (r, Jc, Jp) to _schurref.Problem, and the
whole reference of the squared-loss step (operators, dense S, direct, pcg) applies to it unchanged."""
import numpy as np

import _schurref as R

LD = np.longdouble
KINDS = {None: 0, "squared": 0, "huber": 1, "cauchy": 2, "soft_l1": 3}


def _kind(kind):
    return KINDS[kind] if not isinstance(kind, (int, np.integer)) else int(kind)


def _s(r):
    r = np.asarray(r, dtype=np.float64).astype(LD).reshape(-1, 2)
    return r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]


def weights_of_s(kind, a, s):
    """w = rho'(s) in longdouble, s [n] (longdouble); s = 0 gives exactly 1 in every kind"""
    kind, a2, s = _kind(kind), LD(a) * LD(a), np.asarray(s, dtype=LD)
    if kind == 0:
        return np.ones_like(s)
    if kind == 1:
        return np.where(s <= a2, LD(1), LD(a) / np.sqrt(np.where(s <= a2, LD(1), s)))
    if kind == 2:
        return LD(1) / (LD(1) + s / a2)
    if kind == 3:
        return LD(1) / np.sqrt(LD(1) + s / a2)
    raise ValueError("loss kind %r" % (kind,))


def cost_of_s(kind, a, s):
    """rho(s) in longdouble, s [n] (longdouble).  soft-L1 as 2 s / (sqrt(1 + s / a^2) + 1): the same function without
    the cancellation of sqrt(1 + x) - 1"""
    kind, a2, s = _kind(kind), LD(a) * LD(a), np.asarray(s, dtype=LD)
    if kind == 0:
        return s.copy()
    if kind == 1:
        return np.where(s <= a2, s, LD(2) * LD(a) * np.sqrt(s) - a2)
    if kind == 2:
        return a2 * np.log1p(s / a2)
    if kind == 3:
        return LD(2) * s / (np.sqrt(LD(1) + s / a2) + LD(1))
    raise ValueError("loss kind %r" % (kind,))


def weights(kind, a, r):
    """w [n] (longdouble) of the residuals r [n,2] (f64)"""
    return weights_of_s(kind, a, _s(r))


def cost(kind, a, r):
    """rho(s) [n] (longdouble) of the residuals r [n,2]: the robust cost is its sum"""
    return cost_of_s(kind, a, _s(r))


def reweighted(kind, a, r, Jc, Jp):
    """(sqrt(w) r [n,2], sqrt(w) Jc [n,2,9], sqrt(w) Jp [n,2,3]) in longdouble; kind 0 returns the inputs' values exactly"""
    n = np.asarray(r).size // 2
    r = np.asarray(r, dtype=np.float64).reshape(n, 2).astype(LD)
    Jc = np.asarray(Jc, dtype=np.float64).reshape(n, 2, 9).astype(LD)
    Jp = np.asarray(Jp, dtype=np.float64).reshape(n, 2, 3).astype(LD)
    if _kind(kind) == 0:
        return r, Jc, Jp
    sw = np.sqrt(weights(kind, a, r))
    return sw[:, None] * r, sw[:, None, None] * Jc, sw[:, None, None] * Jp


def problem(kind, a, r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts, dtype=np.float64):
    """_schurref.Problem of the reweighted linearisation (Problem takes f64 arrays: the weighted entries round once)"""
    wr, wJc, wJp = reweighted(kind, a, r, Jc, Jp)
    return R.Problem(wr.astype(np.float64), wJc.astype(np.float64), wJp.astype(np.float64), cam_of, pt_idx, n_cam, n_pts, dtype=dtype)
