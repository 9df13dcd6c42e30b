"""Host reference of consensus triangulation (BAProblem.triangulate_points_robust) in numpy.longdouble, and the
problems its CPU and GPU tests share.  numpy only: nothing here touches a device.

The rules (include/city2ba_hip_experimental.h has them in full), per point p whose row of the transpose is its
observations in ascending index:
  constant under the mask; else the sample = the usable observations (_triangref.rays) among the row's first 64 entries,
  m of them; m < 2: too few; pair k = 0, 1, ... < max_hypotheses by `pairs` (the gap from m // 2 down to 1, wide first);
  hypothesis k is formed when the two-ray midpoint passes _triangref's acceptance (lambda_min >= 1 - cos(min_angle), the
  Cholesky pivots > 0, X finite); none formed: degenerate; the score of k = how many usable observations of the whole row
  X_k reprojects within max_error (r^2 <= max_error^2) at q.z < 0; the highest score wins, the lowest k among equals;
  fewer than min_inliers: no consensus; else the refit is _triangref.reference on the list restricted to the inliers: its
  X, its status (degenerate, behind, triangulated) and its bound.
hyp / n_inl are set once a hypothesis was selected, whatever the status after it.  inlier[o] = 0 for the observations of a
triangulated point that are not inliers, 1 everywhere else.

A point is EXCUSED when any decision the rules take for it lies within CAP (relative) of its threshold: a two-ray
lambda_min against the parallax threshold, an r^2 against max_error^2 (every formed hypothesis, every usable observation),
a q.z against 0 (|q.z| <= CAP |q|) where r^2 <= max_error^2, the refit's lambda_min.  The tests demand that no point of
their problems is excused, so every point is compared with ==."""
import numpy as np

import _schurref as R
import _triangref as T

LD = T.LD
CAP = T.CAP
OK, TOO_FEW, DEGENERATE, BEHIND, CONSTANT, NO_CONSENSUS = range(6)
STATUS = T.STATUS + ("no_consensus",)
SAMPLE = 64


def pairs(m, max_hypotheses):
    """the enumeration, literally: [(lo, hi)] of at most max_hypotheses pairs of a sample of m"""
    out = []
    for g in range(m // 2, 0, -1):
        for i in range(m):
            if 2 * g == m and i >= g:
                continue
            j = (i + g) % m
            out.append((min(i, j), max(i, j)))
            if len(out) == max_hypotheses:
                return out
    return out


def _project(cam, X):
    """cam [n, 15], X [K, 3] longdouble -> (r-independent) u, v [K, n], q [K, n, 3]"""
    q = np.stack([cam[None, :, i] * X[:, None, 0] + cam[None, :, 3 + i] * X[:, None, 1] + cam[None, :, 6 + i] * X[:, None, 2] + cam[None, :, 9 + i]
                  for i in range(3)], axis=-1)
    with np.errstate(all="ignore"):
        px, py = -q[..., 0] / q[..., 2], -q[..., 1] / q[..., 2]
        n = px * px + py * py
        fr = cam[None, :, 12] * (1 + cam[None, :, 13] * n + cam[None, :, 14] * n * n)
    return fr * px, fr * py, q


def _two_ray(d1, d2, C1, C2):
    """the midpoint of two rays: (X [K, 3], lambda_min [K], pivots > 0 and X finite [K]).  lambda_min(2 I - d1 d1^T - d2 d2^T)
    = 1 - |d1 . d2|, formed without cancellation as |d1 x d2|^2 / (1 + |d1 . d2|)"""
    eye = np.eye(3, dtype=LD)[None]
    P1, P2 = eye - d1[:, :, None] * d1[:, None, :], eye - d2[:, :, None] * d2[:, None, :]
    A = P1 + P2
    b = np.einsum("kij,kj->ki", P1, C1) + np.einsum("kij,kj->ki", P2, C2)
    c = np.abs(np.sum(d1 * d2, axis=1))
    cr = np.cross(d1, d2)
    lam = np.sum(cr * cr, axis=1) / (1 + c)
    with np.errstate(all="ignore"):
        L = R.chol_blocks(A)
        X = np.einsum("kij,kj->ki", R.inv3(A), b)
    piv = np.stack([L[:, k, k] for k in range(3)], axis=1)
    return X, lam, np.all(piv > 0, axis=1) & np.all(np.isfinite(X), axis=1)


def restrict(row_ptr, pt_idx, uv, keep):
    """the camera-major list filtered by keep (stable inside every row)"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    keep = np.asarray(keep, dtype=bool)
    cam_of = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    new_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_of[keep], minlength=len(row_ptr) - 1))]).astype(np.uint64)
    return new_ptr, np.asarray(pt_idx)[keep], np.asarray(uv).reshape(-1, 2)[keep]


def reference(cams15, centers, row_ptr, pt_idx, uv, n_pts, min_angle, max_error, min_inliers=3, max_hypotheses=64, pt_mask=None,
              bound=True):
    """dict(status, hyp, n_inl [n_pts], X [n_pts, 3] longdouble (NaN where status != 0), inlier [n_obs] uint8, excused (sorted
    point indices), bound [n_pts], counts (dict by STATUS), decisions (how many inlier decisions were taken)); min_angle in
    radians"""
    cams15, centers, uv = (np.asarray(v, dtype=np.float64) for v in (cams15, centers, uv))
    uv = uv.reshape(-1, 2)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    pt = np.asarray(pt_idx).astype(np.int64)
    n_obs = len(pt)
    cam_of = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    thr, E2 = T.threshold(min_angle), LD(max_error) * LD(max_error)
    d, usable = T.rays(cams15, uv, cam_of)
    camL, C, uvL = cams15.astype(LD)[cam_of], centers.astype(LD)[cam_of], uv.astype(LD)
    order = np.argsort(pt, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=n_pts))])
    status = np.full(n_pts, TOO_FEW, dtype=np.uint8)
    hyp = np.full(n_pts, -1, dtype=np.int32)
    n_inl = np.zeros(n_pts, dtype=np.int32)
    tentative = np.ones(n_obs, dtype=bool)                       # the inlier sets of the points that reach the refit
    reached, excused, decisions = [], set(), 0
    for p in range(n_pts):
        if pt_mask is not None and pt_mask[p]:
            status[p] = CONSTANT
            continue
        row = order[ptr[p]:ptr[p + 1]]
        sample = [o for o in row[:SAMPLE] if usable[o]]
        m = len(sample)
        if m < 2:
            continue
        pr = pairs(m, max_hypotheses)
        lo, hi = np.array([sample[a] for a, _ in pr]), np.array([sample[b] for _, b in pr])
        X, lam, solved = _two_ray(d[lo], d[hi], C[lo], C[hi])
        if (np.abs(lam - thr) <= CAP * thr).any():
            excused.add(p)
        formed = (lam >= thr) & solved
        if not formed.any():
            status[p] = DEGENERATE
            continue
        use = row[usable[row]]
        u, v, q = _project(camL[use], X)
        with np.errstate(all="ignore"):
            du, dv = u - uvL[None, use, 0], v - uvL[None, use, 1]
            r2 = du * du + dv * dv
            close = r2 <= E2
            inl = close & (q[..., 2] < 0)
            near = (np.abs(r2 - E2) <= CAP * E2) | (close & (np.abs(q[..., 2]) <= CAP * np.sqrt(np.sum(q * q, axis=-1))))
        decisions += int(formed.sum()) * len(use)
        if near[formed].any():
            excused.add(p)
        score = np.where(formed, inl.sum(axis=1), -1)
        k = int(np.argmax(score))                                 # the first of the highest: the lowest k
        hyp[p], n_inl[p] = k, int(score[k])
        if score[k] < min_inliers:
            status[p] = NO_CONSENSUS
            continue
        reached.append(p)
        tentative[row] = False
        tentative[use[inl[k]]] = True
    # the refit: _triangref's own reference on the list restricted to the inliers
    Xout = np.full((n_pts, 3), np.nan, dtype=LD)
    bnd = np.zeros(n_pts)
    reached = np.array(reached, dtype=np.int64)
    if len(reached):
        rp, ri, ruv = restrict(row_ptr, pt, uv, tentative)
        ref = T.reference(cams15, centers, rp, ri, ruv, n_pts, min_angle, bound=bound)
        assert (ref["n_used"][reached] == n_inl[reached]).all()
        status[reached] = ref["status"][reached]
        excused |= set(int(v) for v in T.cap_violations(ref) if v in set(reached.tolist()))
        ok = reached[ref["status"][reached] == T.OK]
        Xout[ok] = ref["X"][ok]
        if bound:
            bnd[ok] = ref["bound"][ok]
    inlier = np.ones(n_obs, dtype=np.uint8)
    is_ok = status == OK
    inlier[is_ok[pt] & ~tentative] = 0
    return dict(status=status, hyp=hyp, n_inl=n_inl, X=Xout, inlier=inlier, excused=sorted(excused), bound=bnd if bound else None,
                counts=counts_of(status), decisions=decisions)


def counts_of(status):
    return dict(zip(STATUS, (int(v) for v in np.bincount(status, minlength=6))))


# ---- the problems -------------------------------------------------------------------------------------------------------
DOME_CASES = T.DOME_CASES
MAX_ERROR = 0.01
SECOND_MAX_ERROR = 0.003                                     # a second, tighter pass over a list the first has cleaned
SWAP_SEED, SWAP_CHANCE = 5, 0.1


def wrong_match_dome(state, obs_noise):
    """_triangref.dome_case (every point START from the truth) with wrong matches: through the cameras in ascending order
    and the observations j of a row in order, with chance SWAP_CHANCE the point index of j is swapped with that of a
    drawn observation of the same row (rows of two or more; nothing happens when both name the same point).  The pixels
    stay: both observations then hand their point a ray of another point."""
    P = T.dome_case(state, obs_noise)
    rng = np.random.default_rng(SWAP_SEED)
    pt = P["pt_idx"].copy()
    wrong = np.zeros(len(pt), dtype=bool)
    rp = P["row_ptr"].astype(np.int64)
    for c in range(len(rp) - 1):
        b, e = int(rp[c]), int(rp[c + 1])
        for j in range(b, e):
            if e - b >= 2 and rng.random() < SWAP_CHANCE:
                k = int(rng.integers(b, e))
                if pt[j] != pt[k]:
                    pt[j], pt[k] = pt[k], pt[j]
    wrong = pt != P["pt_idx"]
    P["true_pt_idx"] = P["pt_idx"]
    P["pt_idx"] = pt
    P["wrong"] = wrong
    return P


EDGE = dict(two_ray=0, two_wrong=1, tie=2, narrow=3, f_zero=4, behind=5, masked=6)        # point indices of the edge set


def edge_problem():
    """Seven points, each with cameras of its own (one observation per camera; T._cam: at its centre, looking down -z, R = I),
    at MAX_ERROR, one degree:
      two_ray    two right rays: triangulated at min_inliers = 2, no consensus at 3;
      two_wrong  five rays, the second and the fourth of them rays to a point 1 away: triangulated from the other three,
                 the mask marks exactly those two;
      tie        rays b0 a0 a1 b1 to two points A and B 1.5 apart: the mixed pairs k = 0, 1, 2, 4 agree with nothing, (a0, a1)
                 is pair 3 and (b0, b1) pair 5, both with score 2: the lower k wins, the point is A at min_inliers = 2 with
                 the b rays as outliers; no consensus at 3;
      narrow     three cameras 0.03 apart at distance 10 (0.17 degrees): no hypothesis is formed, degenerate;
      f_zero     three right rays and a camera with f = 0 observing (0, 0), which is what it projects everything to: it fits
                 but is unusable, never an inlier;
      behind     cameras at (-4, 0, 10) and (4, 0, 10) see the point T = 0 exactly, one at (0, 4, 10) sees (0, 0, 0.08), 0.003
                 from T's pixel, and one sits 0.01 above T looking down at it: T is the consensus of all four, in front of
                 all four; the midpoint of the four rays lies about 0.03 above T, behind the fourth camera;
      masked     three right rays, the point constant under the mask.
    Loaded in state mode.  Returns dict(cams15, pts, true_pts, row_ptr, pt_idx, uv, pt_mask, bal=False)."""
    cams, obs = [], []

    def add(center, p, target, **kw):
        cam = T._cam(center, **kw)
        cams.append(cam)
        obs.append((p, T._project(cam, target) if kw.get("f", 1.0) != 0.0 else np.zeros(2)))
    pts = np.array([[0.3, -0.2, 0.1], [-1.0, 0.5, 0.0], [0.5, 0.5, 0.0], [1.0, 1.0, 0.0], [-0.5, -1.0, 0.2], [0.0, 0.0, 0.0], [1.5, -1.0, 0.3]])
    e = EDGE
    add([-3, 0, 10.0], e["two_ray"], pts[0], f=1.1, k1=1e-2, k2=-2e-3)
    add([3, 1, 11.0], e["two_ray"], pts[0])
    other = pts[1] + [1.0, 0.0, 0.0]
    for k, (c, tgt) in enumerate((([-3, -2, 10.0], pts[1]), ([3, -2, 11.0], other), ([3, 2, 9.0], pts[1]), ([-3, 2, 12.0], other), ([0, 3, 10.0], pts[1]))):
        add(c, e["two_wrong"], tgt, f=1.0 + 0.05 * k, k1=1e-2 * (k % 2), k2=1e-2 * (k % 3 == 0))
    A, B = pts[2], pts[2] + [1.5, 0.0, 0.0]
    add([-3, 3, 10.0], e["tie"], B)
    add([-2, -3, 11.0], e["tie"], A, k2=5e-3)
    add([3, -1, 9.0], e["tie"], A)
    add([2, 4, 12.0], e["tie"], B)
    for c in ([1.0, 1.0, 10.0], [1.03, 1.0, 10.0], [1.0, 1.03, 10.0]):
        add(c, e["narrow"], pts[3])
    add([-3, -2, 10.0], e["f_zero"], pts[4])
    add([3, 0, 10.0], e["f_zero"], pts[4], f=0.0)
    add([3, -2, 11.0], e["f_zero"], pts[4], k1=-1e-2)
    add([0, 3, 9.0], e["f_zero"], pts[4])
    add([-4, 0, 10.0], e["behind"], pts[5])
    add([4, 0, 10.0], e["behind"], pts[5])
    add([0, 4, 10.0], e["behind"], [0.0, 0.0, 0.08])
    add([0, 0, 0.01], e["behind"], pts[5])
    for c in ([-3, 0, 10.0], [3, 0, 10.0], [0, 3, 10.0]):
        add(c, e["masked"], pts[6])
    start = pts + np.random.default_rng(4).normal(scale=0.3, size=pts.shape)
    mask = np.zeros(len(pts), dtype=bool)
    mask[e["masked"]] = True
    return dict(cams15=np.ascontiguousarray(np.asarray(cams)), pts=start, true_pts=pts, row_ptr=np.arange(len(cams) + 1, dtype=np.uint64),
                pt_idx=np.array([p for p, _ in obs], dtype=np.uint64), uv=np.array([v for _, v in obs], dtype=np.float64), pt_mask=mask, bal=False)


def edge_expected(min_inliers):
    """(status, hyp, the zeros of the inlier mask) of edge_problem at min_inliers = 2 or 3"""
    e = EDGE
    s = np.zeros(7, dtype=np.uint8)
    s[e["two_ray"]] = s[e["tie"]] = OK if min_inliers == 2 else NO_CONSENSUS
    s[e["narrow"]] = DEGENERATE
    s[e["behind"]] = BEHIND
    s[e["masked"]] = CONSTANT
    hyp = {e["two_ray"]: 0, e["tie"]: 3, e["narrow"]: -1, e["masked"]: -1}
    zeros = [3, 5] + ([7, 10] if min_inliers == 2 else []) + [15]       # two_wrong's wrong rays, tie's b rays, the f = 0 camera
    return s, hyp, np.array(sorted(zeros))
