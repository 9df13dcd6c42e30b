"""Host reference of the outlier filter (BAProblem.filter_observations).  The projection is the CPU oracle's --
bit-equal to the device's by the parity suite -- and the predicate is the five operations the kernel performs, as five
numpy operations (numpy fuses nothing): du = u - x; dv = v - y; r2 = du * du + dv * dv; keep = r2 <= max_error^2 and, with
in_front, q.z < 0.  A longdouble twin of r2 and q.z says whether a threshold can be decided in double at all, and
thresholds() places thresholds where it can: in the middle of a gap between two adjacent residuals."""
import numpy as np

import oracle as O
from _problems import dome_problem, random_problem

LD = np.longdouble
GAP = 1e-9                                   # the least relative gap between the two residuals a threshold is placed between


def cam_of(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def residuals(cams15, pts, row_ptr, pt_idx, uv):
    """(r2, qz) per observation in double: the oracle's projection, then the predicate's operations one by one; q.z is the
    oracle's project_world"""
    cams15, pts, uv = np.asarray(cams15, dtype=np.float64).reshape(-1, 15), np.asarray(pts, dtype=np.float64), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    proj = O.project_observations(cams15, pts, row_ptr, pt_idx).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        du = proj[:, 0] - uv[:, 0]
        dv = proj[:, 1] - uv[:, 1]
        uu = du * du
        vv = dv * dv
        r2 = uu + vv
    c = cam_of(row_ptr)
    pi = np.asarray(pt_idx, dtype=np.int64)
    qz = np.array([O.project_world(cams15[a], pts[b])[2] for a, b in zip(c, pi)], dtype=np.float64).reshape(-1)
    return r2, qz


def residuals_ld(cams15, pts, row_ptr, pt_idx, uv):
    """the longdouble twin: r2 from the same (double) projection with the tail in longdouble, q.z = R X + t in longdouble;
    every point's distance from its camera's centre, the scale |q.z| is held against; and the sum of the magnitudes of
    q.z's four terms, the scale of its rounding"""
    cams15, pts, uv = np.asarray(cams15, dtype=np.float64).reshape(-1, 15), np.asarray(pts, dtype=np.float64), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    proj = O.project_observations(cams15, pts, row_ptr, pt_idx).reshape(-1, 2).astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = proj[:, 0] - uv[:, 0].astype(LD), proj[:, 1] - uv[:, 1].astype(LD)
        r2 = du * du + dv * dv
    c = cam_of(row_ptr)
    X = pts[np.asarray(pt_idx, dtype=np.int64)].astype(LD)
    K = cams15[c].astype(LD)                                     # R is column-major: R[i, j] = K[3 j + i]
    q = np.stack([K[:, i] * X[:, 0] + K[:, 3 + i] * X[:, 1] + K[:, 6 + i] * X[:, 2] + K[:, 9 + i] for i in range(3)], axis=1)
    mag = np.abs(K[:, 2] * X[:, 0]) + np.abs(K[:, 5] * X[:, 1]) + np.abs(K[:, 8] * X[:, 2]) + np.abs(K[:, 11])
    return r2, q[:, 2], np.sqrt(np.sum(q * q, axis=1)), mag      # |q| = |X - centre|: R is a rotation; mag: the terms of q.z


def max_err2(max_error):
    """max_error * max_error, formed once, in double"""
    return np.float64(max_error) * np.float64(max_error)


def keep_mask(r2, qz, max_error, in_front=False):
    with np.errstate(invalid="ignore"):
        keep = r2 <= max_err2(max_error)                         # NaN compares false
        if in_front:
            keep = keep & (qz < 0.0)
    return keep


def filtered(row_ptr, pt_idx, uv, keep):
    """the filtered (row_ptr, pt_idx, uv): the old order inside every row"""
    c = cam_of(row_ptr)
    counts = np.bincount(c[keep], minlength=len(row_ptr) - 1)
    new_rows = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return new_rows, np.ascontiguousarray(np.asarray(pt_idx, dtype=np.uint64)[keep]), np.ascontiguousarray(np.asarray(uv).reshape(-1, 2)[keep])


def reference(cams15, pts, row_ptr, pt_idx, uv, max_error, in_front=False):
    """(keep, row_ptr, pt_idx, uv, n_removed) of one filter"""
    r2, qz = residuals(cams15, pts, row_ptr, pt_idx, uv)
    keep = keep_mask(r2, qz, max_error, in_front)
    rows, pi, obs = filtered(row_ptr, pt_idx, uv, keep)
    return keep, rows, pi, obs, int(len(keep) - keep.sum())


def threshold_at(r2, percentile, gap=GAP):
    """max_error = sqrt of the midpoint of two adjacent sorted residuals whose relative gap is at least `gap`, the pair
    nearest the given percentile; returns (max_error, lo, hi) with lo < max_error^2 < hi required of the caller's check"""
    s = np.sort(r2[np.isfinite(r2)])
    n = len(s)
    if n < 2:
        raise ValueError("threshold_at: fewer than two finite residuals")
    k0 = min(max(int(round(percentile / 100.0 * (n - 1))), 0), n - 2)
    for d in range(n):
        for k in (k0 - d, k0 + d):
            if 0 <= k <= n - 2 and s[k + 1] - s[k] >= gap * s[k + 1] and s[k + 1] > 0.0:
                return float(np.sqrt(0.5 * (s[k] + s[k + 1]))), float(s[k]), float(s[k + 1])
    raise ValueError("threshold_at: no two adjacent residuals are %g apart" % gap)


# ---- the cases the GPU tests run, built once and never changed -------------------------------------------------------------
BEHIND = 6                                   # points moved behind one of their cameras for the in_front cases
_cache = {}


def dome_case(dup, state, behind=False):
    """dome_problem(dup, state) as the GPU tests load it, with `thresholds` = the 50th- and 90th-percentile thresholds.
    behind: BEHIND shared points are moved to the camera-frame place (0.3, 0.1 k, 5) of the first camera that sees each
    -- behind it -- and that camera's observation of the point becomes its exact projection there, so the residual test
    keeps it (r2 == 0) and only the in-front test can remove it."""
    key = (bool(dup), bool(state), bool(behind))
    if key in _cache:
        return _cache[key]
    P = dict(dome_problem(dup=dup, state=state))
    P["moved"] = np.zeros(0, dtype=np.int64)
    if behind:
        pts, uv = P["pts"].copy(), P["uv"].copy()
        c = cam_of(P["row_ptr"])
        pi = P["pt_idx"].astype(np.int64)
        seen = np.bincount(pi, minlength=len(pts))
        chosen = [p for p in range(41, len(pts)) if seen[p] >= 3][:BEHIND]       # shared points (tests/_problems.py: 41 ..)
        at = []
        for k, p in enumerate(chosen):
            o = int(np.flatnonzero(pi == p)[0])
            pts[p] = O.to_world(P["cams15"][c[o]], np.array([0.3, 0.1 * k, 5.0]))
            at.append(o)
        for o in at:                                             # once every point is where it stays
            uv[o] = O.project_observations(P["cams15"][c[o]:c[o] + 1], pts, np.array([0, 1], dtype=np.uint64), P["pt_idx"][o:o + 1])[0]
        P["pts"], P["uv"], P["moved"] = pts, uv, np.array(at, dtype=np.int64)
    P["r2"], P["qz"] = residuals(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    P["thresholds"] = tuple(threshold_at(P["r2"], q)[0] for q in (50, 90))
    _cache[key] = P
    return P


def case_reference(P, max_error, in_front=False):
    """reference() of a case from its stored residuals: (keep, row_ptr, pt_idx, uv, n_removed)"""
    keep = keep_mask(P["r2"], P["qz"], max_error, in_front)
    rows, pi, obs = filtered(P["row_ptr"], P["pt_idx"], P["uv"], keep)
    return keep, rows, pi, obs, int(len(keep) - keep.sum())


DOME_CASES = [(dup, state, behind) for dup in (True, False) for state in (False, True) for behind in (False, True)]

COUNT_EDGES = (0, 1, 63, 64, 65, 191, 192, 193, 1535, 1536, 1537, 3073)     # a wave takes 192 observations, a workgroup 1 536


def count_case(n_obs):
    """The first n_obs observations of one random_problem list with every fifth camera empty and every observation noisy
    (trailing cameras become empty too); `threshold` = its 50th-percentile threshold (None below two observations)."""
    if "count_base" not in _cache:
        B = random_problem(40, 5000, 110, seed=77, noise=1e-3, empty_every=5)
        assert int(B["row_ptr"][-1]) >= max(COUNT_EDGES)
        _cache["count_base"] = B
    key = ("count", n_obs)
    if key not in _cache:
        B = _cache["count_base"]
        P = dict(B)
        P["row_ptr"] = np.minimum(B["row_ptr"], np.uint64(n_obs)).astype(np.uint64)
        P["pt_idx"], P["uv"] = B["pt_idx"][:n_obs].copy(), B["uv"][:n_obs].copy()
        P["bal"] = True
        P["threshold"] = None
        P["r2"], P["qz"] = residuals(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
        if n_obs >= 2:
            P["threshold"] = threshold_at(P["r2"], 50)[0]
        _cache[key] = P
    return _cache[key]
