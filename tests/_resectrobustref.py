"""Host reference of consensus resection (BAProblem.resect_cameras_robust) in numpy.longdouble, and the
problems its CPU and GPU tests share.  numpy only: nothing here touches a device.

The rules (include/city2ba_hip_experimental.h has them in full), per camera c whose row of the list is walked in ascending
order, usable(o) as _resectref.pixel_rays plus a finite point:
  constant under the mask's pose bits; fewer than min_inliers usable observations in the whole row: too few; the sample =
  the usable observations among the row's first 64 entries, m of them; triple k = 0, 1, ... < max_hypotheses by `triples`
  (the gap from m // 3 down to 1, wide first); the three-point poses of a triple are the real (l1, l2, l3), all > 0, with
  li^2 + lj^2 - 2 li lj (bi . bj) = |Xi - Xj|^2 for the three pairs, polished by Newton, formed unless the points are
  collinear or the equations' Jacobian is ill-conditioned (|det J| <= COND (2 max l)^3), duplicates merged; none formed in any triple:
  degenerate; the score of a pose = how many usable observations of the whole row it reprojects within max_error at
  q.z < 0; the highest score wins, the lowest k among equals, the smallest l1 among that triple's solutions; fewer than
  min_inliers: no consensus; else the refit is _resectref.reference on the list restricted to the inliers: its pose, its
  status (degenerate, behind, resected) and its bounds.
hyp / n_inl are set once a hypothesis was selected, whatever the status after it.  inlier[o] = 0 for the observations of a
resected camera that are not inliers, 1 everywhere else.

Candidates are found here otherwise than on the device (Durand-Kerner on one quartic there): for each of the
three cyclic renumberings of the triple, the quartic in the ratio of two depths, its roots as the eigenvalues of the
companion matrix (numpy.roots, float64), every root that is real within ROOT_IMAG, both depths the third equation then
allows -- far more starts than solutions; Newton in the working precision, the acceptance test and the merge leave the
solutions.

A camera is EXCUSED when any decision the rules take for it lies within CAP (relative) of its threshold: an r^2 against
max_error^2 (every formed solution, every usable observation), a q.z against 0 (|q.z| <= CAP |q|) where r^2 <=
max_error^2, the collinearity and the conditioning test, the duplicate merge, two solutions of the winning triple with
equal score and l1 within CAP, the refit's own cap_violations -- or when the same rules run in float64 give another
status, hyp, n_inl or inlier set for it.  The tests demand that no camera of their problems is excused, so every camera
is compared with ==."""
import numpy as np

import _resectref as T
import _triangrobustref as TR

LD = T.LD
CAP = T.CAP
OK, TOO_FEW, DEGENERATE, BEHIND, CONSTANT, NO_CONSENSUS = range(6)
STATUS = T.STATUS + ("no_consensus",)
SAMPLE = 64
MIN_INLIERS = 6
COLLINEAR = 1e-12           # |(X2 - X1) x (X3 - X1)|^2 < COLLINEAR |X2 - X1|^2 |X3 - X1|^2: no solution is formed
COND = 1e-5                 # |det J| <= COND (2 max(l))^3 of the equations' Jacobian: the solution is not formed
MERGE = 1e-9                # two solutions within MERGE max(l) of each other are one
ACCEPT = 1e-9               # a Newton run counts when its last step was at most ACCEPT max(l)
NEWTON_STEPS, NEWTON_TOL = 8, 1e-14
ROOT_IMAG = 1e-2            # a root of the quartic is a start when |imag| <= ROOT_IMAG (1 + |real|)
restrict = TR.restrict


def triples(m, max_hypotheses):
    """the enumeration, literally: [(i0, i1, i2)] ascending, of at most max_hypotheses triples of a sample of m"""
    out = []
    for g in range(m // 3, 0, -1):
        for i in range(m):
            if 3 * g == m and i >= g:
                continue
            out.append(tuple(sorted((i, (i + g) % m, (i + 2 * g) % m))))
            if len(out) == max_hypotheses:
                return out
    return out


def _quartic(a2, b2, c2, ca, cb, cg):
    """coefficients (ascending) of the quartic in v = l3 / l1: a2 = |X2 - X3|^2, b2 = |X1 - X3|^2, c2 = |X1 - X2|^2, ca =
    b2 . b3, cb = b1 . b3, cg = b1 . b2.  With u = l2 / l1 = N(v) / D(v) from the difference of the first two equations
    over the third, b2 (N^2 - 2 cg N D + D^2) = c2 (1 - 2 cb v + v^2) D^2."""
    N = np.array([(c2 - a2) - b2, -2 * cb * (c2 - a2), (c2 - a2) + b2])
    D = np.array([-2 * b2 * cg, 2 * b2 * ca])
    Q = np.array([1.0, -2 * cb, 1.0])
    P = np.polynomial.polynomial
    DD = P.polymul(D, D)
    lhs = P.polyadd(P.polyadd(P.polymul(N, N), -2 * cg * P.polymul(N, D)), DD)
    return P.polysub(b2 * lhs, c2 * P.polymul(Q, DD))


_starts_seen = {}


def _starts(b, X):
    """far more starting depths [n, 3] (float64) than the triple has solutions; kept per triple, since the float64 twin of a
    reference run asks for the same ones"""
    b, X = b.astype(np.float64), X.astype(np.float64)
    key = b.tobytes() + X.tobytes()
    if key not in _starts_seen:
        if len(_starts_seen) > 20000:
            _starts_seen.clear()
        with np.errstate(all="ignore"):
            _starts_seen[key] = _starts_loud(b, X)
    return _starts_seen[key]


def _starts_loud(b, X):
    out = []
    for s in range(3):
        i, j, k = s, (s + 1) % 3, (s + 2) % 3                    # the roles of points 1, 2, 3
        a2, b2, c2 = np.sum((X[j] - X[k]) ** 2), np.sum((X[i] - X[k]) ** 2), np.sum((X[i] - X[j]) ** 2)
        ca, cb, cg = b[j] @ b[k], b[i] @ b[k], b[i] @ b[j]
        co = _quartic(a2 / b2, 1.0, c2 / b2, ca, cb, cg)
        if not np.all(np.isfinite(co)) or not np.any(co[1:] != 0):
            continue
        with np.errstate(all="ignore"):
            roots = np.roots(co[::-1])
        for z in roots:
            if not np.isfinite(z) or abs(z.imag) > ROOT_IMAG * (1 + abs(z.real)):
                continue
            v = z.real
            l1 = np.sqrt(b2 / max(1 - 2 * cb * v + v * v, 1e-300))
            disc = c2 - l1 * l1 * (1 - cg * cg)
            root = np.sqrt(max(disc, 0.0))
            for l2 in (l1 * cg + root, l1 * cg - root):
                lam = np.zeros(3)
                lam[i], lam[j], lam[k] = l1, l2, v * l1
                out.append(lam)
    return np.array(out).reshape(-1, 3)


def _equations(lam, cos, d2):
    """F [n, 3] and J [n, 3, 3] of the pairs (1, 2), (1, 3), (2, 3); cos = (c12, c13, c23), d2 the squared distances"""
    l1, l2, l3 = lam[:, 0], lam[:, 1], lam[:, 2]
    c12, c13, c23 = cos
    F = np.stack([l1 * l1 + l2 * l2 - 2 * l1 * l2 * c12 - d2[0], l1 * l1 + l3 * l3 - 2 * l1 * l3 * c13 - d2[1],
                  l2 * l2 + l3 * l3 - 2 * l2 * l3 * c23 - d2[2]], axis=1)
    z = np.zeros_like(l1)
    J = np.stack([np.stack([2 * (l1 - l2 * c12), 2 * (l2 - l1 * c12), z], axis=1),
                  np.stack([2 * (l1 - l3 * c13), z, 2 * (l3 - l1 * c13)], axis=1),
                  np.stack([z, 2 * (l2 - l3 * c23), 2 * (l3 - l2 * c23)], axis=1)], axis=1)
    return F, J


def _det3(J):
    return (J[:, 0, 0] * (J[:, 1, 1] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 1]) - J[:, 0, 1] * (J[:, 1, 0] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 0])
            + J[:, 0, 2] * (J[:, 1, 0] * J[:, 2, 1] - J[:, 1, 1] * J[:, 2, 0]))


def _solve3(J, F):
    """J^-1 F by cofactors, in J's dtype"""
    det = _det3(J)
    out = []
    for k in range(3):
        Jk = J.copy()
        Jk[:, :, k] = F
        out.append(_det3(Jk) / det)
    return np.stack(out, axis=1)


def three_point(b, X, dtype=LD, measures=None):
    """the solutions of one triple: (lam [n, 3] in `dtype`, near: a decision within CAP of its threshold).  b [3, 3] unit
    rays, X [3, 3] points, in `dtype`.  measures: a list that gets |det J| / (2 max l)^3 of every solution left after the merge."""
    none = np.zeros((0, 3), dtype=dtype)
    e12, e13 = X[1] - X[0], X[2] - X[0]
    cr = np.cross(e12, e13)
    lhs, rhs = np.sum(cr * cr), dtype(COLLINEAR) * np.sum(e12 * e12) * np.sum(e13 * e13)
    near = bool(rhs > 0 and abs(lhs - rhs) <= CAP * rhs)          # (rhs == 0: two of the points are one, in any precision)
    if not lhs >= rhs:                                            # (a NaN forms nothing)
        return none, near
    cos = (np.sum(b[0] * b[1]), np.sum(b[0] * b[2]), np.sum(b[1] * b[2]))
    d2 = (np.sum(e12 * e12), np.sum(e13 * e13), np.sum((X[2] - X[1]) ** 2))
    lam = _starts(b, X).astype(dtype)
    if not len(lam):
        return none, near
    last = np.full(len(lam), np.inf, dtype=dtype)
    live = np.ones(len(lam), dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_STEPS):
            F, J = _equations(lam, cos, d2)
            step = _solve3(J, F)
            step = np.where(live[:, None], step, 0)
            lam = lam - step
            size = np.max(np.abs(step), axis=1)
            last = np.where(live, size, last)
            live = live & ~(size <= dtype(NEWTON_TOL) * np.max(lam, axis=1))
            if not live.any():
                break
        good = np.all(np.isfinite(lam), axis=1) & np.all(lam > 0, axis=1) & (last <= dtype(ACCEPT) * np.max(lam, axis=1))
        lam = lam[good]
        _, J = _equations(lam, cos, d2)
        det = np.abs(_det3(J))
        rows = (2 * np.max(lam, axis=1)) ** 3 * dtype(COND)       # (every entry of J is at most 2 max(l) in magnitude)
    # the merge first, among everything accepted (a start is not a decision); then the conditioning of what is left
    keep = []
    for n in range(len(lam)):
        scale = dtype(MERGE)
        dup = False
        for q in keep:
            dist, thr = np.max(np.abs(lam[n] - lam[q])), scale * max(np.max(lam[n]), np.max(lam[q]))
            if dist <= thr:
                dup = True
                break
            if dist <= thr * (1 + CAP):
                near = True
        if not dup:
            keep.append(n)
    keep = np.array(keep, dtype=np.int64)
    if not len(keep):
        return none, near
    lam, det, rows = lam[keep], det[keep], rows[keep]
    near = near or bool((np.abs(det - rows) <= CAP * rows).any())
    if measures is not None:
        measures.extend(float(v) for v in det / rows * dtype(COND))
    formed = det > rows
    return lam[formed], near


def _frame(P):
    """the orthonormal frame (columns e1 e2 e3) of the triangle P [3, 3] (rows = vertices)"""
    with np.errstate(all="ignore"):
        e1 = P[1] - P[0]
        e1 = e1 / np.sqrt(np.sum(e1 * e1))
        e3 = np.cross(e1, P[2] - P[0])
        e3 = e3 / np.sqrt(np.sum(e3 * e3))
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)


def pose_from_depths(lam, b, X):
    """(R [3, 3], t [3]) with q = R X + t from one solution"""
    Rm = _frame(lam[:, None] * b) @ _frame(X).T
    return Rm, lam[0] * b[0] - Rm @ X[0]


def _consensus(intr, pts, row_ptr, pt_idx, uv, max_error, min_inliers, max_hypotheses, cam_mask, dtype):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_cam = len(row_ptr) - 1
    cam_of = np.repeat(np.arange(n_cam), np.diff(row_ptr))
    pt = np.asarray(pt_idx).astype(np.int64)
    n_obs = len(pt)
    b, usable = T.pixel_rays(intr, uv, cam_of)
    b = b.astype(dtype)
    X = np.asarray(pts).astype(dtype)[pt]
    usable = usable & np.all(np.isfinite(X), axis=1)
    uvd = np.asarray(uv).reshape(-1, 2).astype(dtype)
    intr = np.asarray(intr).astype(dtype)
    E2 = dtype(max_error) * dtype(max_error)
    constant = np.zeros(n_cam, dtype=bool) if cam_mask is None else (np.asarray(cam_mask).astype(np.int64) & T.POSE_BITS) != 0
    status = np.full(n_cam, TOO_FEW, dtype=np.uint8)
    hyp = np.full(n_cam, -1, dtype=np.int32)
    n_inl = np.zeros(n_cam, dtype=np.int32)
    tentative = np.ones(n_obs, dtype=bool)
    Rw, tw = np.full((n_cam, 3, 3), np.nan, dtype=dtype), np.full((n_cam, 3), np.nan, dtype=dtype)
    reached, excused = [], set()
    stats = dict(walks=0, decisions=0, triples=0, multi=0, not_first=0, margin=np.inf, solutions=0, cond_rejected=0, cond_median=np.nan)
    measures = []
    for c in range(n_cam):
        if constant[c]:
            status[c] = CONSTANT
            continue
        row = np.arange(row_ptr[c], row_ptr[c + 1])
        use = row[usable[row]]
        if len(use) < min_inliers:
            continue
        sample = [o for o in row[:SAMPLE] if usable[o]]
        best = None                                               # (score, k, l1, inlier set, R, t, tie)
        f, k1, k2 = intr[c]
        for k, tri in enumerate(triples(len(sample), max_hypotheses)):
            o3 = [sample[i] for i in tri]
            lam, near = three_point(b[o3], X[o3], dtype, measures)
            if near:
                excused.add(c)
            stats["triples"] += 1
            stats["multi"] += len(lam) > 1
            mine = None
            for s in np.argsort(lam[:, 0].astype(np.float64), kind="stable") if len(lam) else []:
                Rm, t = pose_from_depths(lam[s], b[o3], X[o3])
                with np.errstate(all="ignore"):
                    q = X[use] @ Rm.T + t
                    px, py = -q[:, 0] / q[:, 2], -q[:, 1] / q[:, 2]
                    n = px * px + py * py
                    fr = f * (1 + k1 * n + k2 * n * n)
                    du, dv = fr * px - uvd[use, 0], fr * py - uvd[use, 1]
                    r2 = du * du + dv * dv
                    close = r2 <= E2
                    inl = close & (q[:, 2] < 0)
                    rel = np.abs(r2 - E2) / E2 if E2 > 0 else np.where(r2 == 0, 0.0, np.inf)
                    edge = (rel <= CAP) | (close & (np.abs(q[:, 2]) <= CAP * np.sqrt(np.sum(q * q, axis=1))))
                stats["walks"] += 1
                stats["decisions"] += len(use)
                fin = np.isfinite(rel.astype(np.float64))
                if fin.any():
                    stats["margin"] = min(stats["margin"], float(rel[fin].min()))
                if edge.any():
                    excused.add(c)
                score = int(inl.sum())
                if mine is None or score > mine[0]:               # ascending l1: the first of the highest is the smallest l1
                    mine = [score, k, lam[s, 0], inl, Rm, t, False, s]
                elif score == mine[0] and abs(lam[s, 0] - mine[2]) <= CAP * lam[s, 0]:
                    mine[6] = True
            if mine is not None and (best is None or mine[0] > best[0]):
                best = mine
        if best is None:
            status[c] = DEGENERATE
            continue
        if best[6]:
            excused.add(c)
        stats["not_first"] += best[7] != 0
        hyp[c], n_inl[c] = best[1], best[0]
        Rw[c], tw[c] = best[4], best[5]
        if best[0] < min_inliers:
            status[c] = NO_CONSENSUS
            continue
        status[c] = OK                                            # the refit decides
        reached.append(c)
        tentative[row] = False
        tentative[use[best[3]]] = True
    if measures:                                                  # the conditioning measure of every merged solution, formed or not
        stats.update(solutions=len(measures), cond_rejected=int((np.array(measures) <= COND).sum()), cond_median=float(np.median(measures)))
    return dict(status=status, hyp=hyp, n_inl=n_inl, tentative=tentative, reached=np.array(reached, dtype=np.int64), excused=excused,
                R=Rw, t=tw, stats=stats)


def reference(cams15, pts, row_ptr, pt_idx, uv, max_error, min_inliers=MIN_INLIERS, min_gap=T.MIN_GAP, max_hypotheses=64, cam_mask=None,
              bound=True, twin=True):
    """dict(status, hyp, n_inl [n_cam], R, t (the refit's, NaN where status != 0), R_hyp, t_hyp (the selected pose), inlier
    [n_obs] uint8, excused (sorted camera indices), bound_R, bound_t, counts (dict by STATUS), stats).  twin: also run
    the rules in float64 and excuse what differs."""
    intr = np.asarray(cams15, dtype=np.float64)[:, 12:15]
    pts, uv = np.asarray(pts, dtype=np.float64), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    pt = np.asarray(pt_idx).astype(np.int64)
    n_cam = len(row_ptr) - 1
    cam_of = np.repeat(np.arange(n_cam), np.diff(row_ptr))
    A = _consensus(intr, pts, row_ptr, pt, uv, max_error, min_inliers, max_hypotheses, cam_mask, LD)
    excused = set(A["excused"])
    if twin:
        B = _consensus(intr, pts, row_ptr, pt, uv, max_error, min_inliers, max_hypotheses, cam_mask, np.float64)
        differs = (A["status"] != B["status"]) | (A["hyp"] != B["hyp"]) | (A["n_inl"] != B["n_inl"])
        differs[np.unique(cam_of[A["tentative"] != B["tentative"]])] = True
        excused |= set(int(c) for c in np.flatnonzero(differs))
    status, reached, tentative = A["status"], A["reached"], A["tentative"]
    Rout, tout = np.full((n_cam, 3, 3), np.nan, dtype=LD), np.full((n_cam, 3), np.nan, dtype=LD)
    bR, bt = np.zeros(n_cam), np.zeros(n_cam)
    refit = None
    if len(reached):
        rp, ri, ruv = restrict(row_ptr, pt, uv, tentative)
        refit = T.reference(cams15, pts, rp, ri, ruv, min_points=min_inliers, min_gap=min_gap, cam_mask=cam_mask, bound=bound)
        assert (refit["n_used"][reached] == A["n_inl"][reached]).all()
        status[reached] = refit["status"][reached]
        in_reach = set(reached.tolist())
        excused |= set(int(v) for v in T.cap_violations(refit) if int(v) in in_reach)
        ok = reached[refit["status"][reached] == T.OK]
        Rout[ok], tout[ok] = refit["R"][ok], refit["t"][ok]
        if bound:
            bR[ok], bt[ok] = refit["bound_R"][ok], refit["bound_t"][ok]
    inlier = np.ones(len(pt), dtype=np.uint8)
    inlier[(status == OK)[cam_of] & ~tentative] = 0
    return dict(status=status, hyp=A["hyp"], n_inl=A["n_inl"], R=Rout, t=tout, R_hyp=A["R"], t_hyp=A["t"], inlier=inlier,
                excused=sorted(excused), bound_R=bR if bound else None, bound_t=bt if bound else None, counts=counts_of(status),
                stats=A["stats"], refit=refit, tentative=tentative)


def counts_of(status):
    return dict(zip(STATUS, (int(v) for v in np.bincount(status, minlength=6))))


# ---- the problems -------------------------------------------------------------------------------------------------------
DOME_CASES = T.DOME_CASES
MAX_ERROR = TR.MAX_ERROR
SWAP_SEED, SWAP_CHANCE = TR.SWAP_SEED, TR.SWAP_CHANCE


def swap_matches(P, seed=SWAP_SEED, chance=SWAP_CHANCE):
    """_triangrobustref.wrong_match_dome's swap loop on any camera-major list: through the cameras in ascending order and
    the observations j of a row in order, with `chance` the point index of j is swapped with that of a drawn observation
    of the same row.  The pixels stay.  Adds true_pt_idx and wrong [n_obs]."""
    P = dict(P)
    rng = np.random.default_rng(seed)
    pt = P["pt_idx"].copy()
    rp = P["row_ptr"].astype(np.int64)
    for c in range(len(rp) - 1):
        b, e = int(rp[c]), int(rp[c + 1])
        for j in range(b, e):
            if e - b >= 2 and rng.random() < chance:
                k = int(rng.integers(b, e))
                if pt[j] != pt[k]:
                    pt[j], pt[k] = pt[k], pt[j]
    P["true_pt_idx"] = P["pt_idx"]
    P["wrong"] = pt != P["pt_idx"]
    P["pt_idx"] = pt
    return P


def wrong_match_dome_cameras(state, obs_noise, start_seed=17):
    """_resectref.dome_case (true points, every pose START_ROTATION / START_TRANSLATION from the truth) with the swap loop"""
    return swap_matches(T.dome_case(state, obs_noise, start_seed=start_seed))


def e2e_problem():
    """_resectref.e2e_problem with the same swap loop"""
    return swap_matches(T.e2e_problem())


EDGE = dict(two_wrong=0, larger_depth=1, collinear_first=2, coplanar=3, five_right=4, two_sets=5, f_zero=6, late=7, masked=8)      # camera indices
LARGER_DEPTH_SEED = 0       # found by edge_larger_depth_seed(); tests/test_resectrobustref.py asserts what it stands for


def _edge_camera(seed, n, f=1.0, k1=0.0, k2=0.0):
    rng = np.random.default_rng(seed)
    cam = T._camera(rng, f, k1, k2)
    return rng, cam, T._world(cam, T._frame_points(rng, n))


def edge_larger_depth_seed(limit=200):
    """the first seed whose camera (eight points, all matched rightly) has a first triple {0, 2, 4} with two or more formed
    solutions of which the true pose is not the one of the smallest l1"""
    for seed in range(limit):
        _, cam, X = _edge_camera(1000 + seed, 8, 1.05, 1e-2, -1e-3)
        b, _ = T.pixel_rays(cam[None, 12:15], T._project(cam, X), np.zeros(8, dtype=np.int64))
        lam, near = three_point(b[[0, 2, 4]], X[[0, 2, 4]].astype(LD))
        Rm, t = T.pose_of(cam[None])
        true_l1 = np.linalg.norm(X[0] @ Rm[0].T + t[0])
        if len(lam) >= 2 and not near and abs(float(lam[:, 0].min()) - true_l1) > 1e-3 * true_l1 and np.abs(lam[:, 0].astype(np.float64) - true_l1).min() < 1e-9:
            return seed
    raise AssertionError("no seed")


def edge_problem():
    """Nine hand-placed cameras in general position, each seeing points of its own (EDGE), at MAX_ERROR, min_inliers 6; true
    poses moved by 0.2 / 0.5 at the start:
      two_wrong        six right observations and two (entries 2 and 5) whose pixels belong nowhere: resected, the mask marks
                       exactly the two;
      larger_depth     eight right observations; the first triple has several solutions and the true pose is not the one
                       of the smallest l1: hyp 0, all eight inliers;
      collinear_first  eight right observations, the points of the first triple {0, 2, 4} on a line: hyp > 0, resected;
      coplanar         ten right observations of points on one plane and two wrong ones: a consensus of ten is found, the
                       refit is degenerate at min_gap 1e-4: hyp and n_inl set, the camera keeps its bits, the mask all ones;
      five_right       five right observations among seven random pixels: no consensus;
      two_sets         sixteen observations, the even entries right for the true pose, the odd ones right for another pose:
                       the sixteen triples of gap 5 mix the two, triple 16 = {0, 4, 8} and triple 17 = {1, 5, 9} both score
                       eight, the lower k wins: the true pose;
      f_zero           f = 0: nothing usable, too few;
      late             seventy random pixels, then ten right observations: the sample never sees a right match;
      masked           ten right observations, the camera constant under the mask.
    Loaded in state mode.  Returns dict(cams15 (the start), true_cams15, pts, row_ptr, pt_idx, uv, cam_mask, bal=False)."""
    import oracle as O
    cams, pts, obs = [], [], []

    def add(cam, X, uv):
        cams.append(cam)
        obs.append([(len(pts) + k, uv[k]) for k in range(len(X))])
        pts.extend(list(X))

    def junk(rng, n):
        return rng.uniform(-0.4, 0.4, size=(n, 2))
    rng, cam, X = _edge_camera(11, 8, 1.1, 2e-2, -3e-3)          # two_wrong
    uv = T._project(cam, X)
    uv[[2, 5]] = junk(rng, 2)
    add(cam, X, uv)
    rng, cam, X = _edge_camera(1000 + LARGER_DEPTH_SEED, 8, 1.05, 1e-2, -1e-3)     # larger_depth
    add(cam, X, T._project(cam, X))
    rng, cam, X = _edge_camera(13, 8, 0.9, -1e-2, 0.0)           # collinear_first
    X[2] = 0.5 * (X[0] + X[4])
    add(cam, X, T._project(cam, X))
    rng = np.random.default_rng(14)                              # coplanar
    cam = T._camera(rng, 0.95, 1e-2, 0.0)
    q = T._frame_points(rng, 12)
    q[:, 2] = -9.0 + 0.3 * q[:, 0] - 0.2 * q[:, 1]
    X = T._world(cam, q)
    uv = T._project(cam, X)
    uv[[3, 8]] = junk(rng, 2)
    add(cam, X, uv)
    rng, cam, X = _edge_camera(15, 12, 1.0, 0.0, 0.0)            # five_right
    uv = T._project(cam, X)
    uv[[0, 2, 3, 5, 7, 9, 10]] = junk(rng, 7)
    add(cam, X, uv)
    rng, cam, X = _edge_camera(16, 16, 1.0, 1e-2, 0.0)           # two_sets
    other = cam.copy()
    other[:12] = T._camera(np.random.default_rng(116))[:12]
    X[1::2] = T._world(other, T._frame_points(rng, 8))
    uv = T._project(cam, X)
    uv[1::2] = T._project(other, X[1::2])
    add(cam, X, uv)
    rng, cam, X = _edge_camera(17, 8, 0.0, 0.0, 0.0)             # f_zero
    add(cam, X, np.zeros((8, 2)))
    rng, cam, X = _edge_camera(18, 80, 1.0, 5e-3, 0.0)           # late
    uv = T._project(cam, X)
    uv[:70] = junk(rng, 70)
    add(cam, X, uv)
    rng, cam, X = _edge_camera(19, 10, 1.0, 0.0, 0.0)            # masked
    add(cam, X, T._project(cam, X))
    true = np.ascontiguousarray(np.asarray(cams))
    bal9 = O.camera_to_bal(true)
    g = np.random.default_rng(6).normal(size=(len(bal9), 2, 3))
    g = g / np.linalg.norm(g, axis=2)[:, :, None]
    bal9[:, 0:3] += 0.2 * g[:, 0]
    bal9[:, 3:6] += 0.5 * g[:, 1]
    mask = np.zeros(len(cams), dtype=np.uint16)
    mask[EDGE["masked"]] = 0x03f
    row_ptr = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.uint64)
    return dict(cams15=O.camera_from_bal(bal9), true_cams15=true, pts=np.asarray(pts, dtype=np.float64), row_ptr=row_ptr,
                pt_idx=np.array([p for o in obs for p, _ in o], dtype=np.uint64), uv=np.array([v for o in obs for _, v in o], dtype=np.float64),
                cam_mask=mask, bal=False)


def edge_expected():
    """(status, {camera: hyp}, {camera: n_inl}, the zeros of the inlier mask) of edge_problem at MAX_ERROR, min_inliers 6"""
    e = EDGE
    s = np.zeros(9, dtype=np.uint8)
    s[e["coplanar"]] = DEGENERATE
    s[e["five_right"]] = s[e["late"]] = NO_CONSENSUS
    s[e["f_zero"]] = TOO_FEW
    s[e["masked"]] = CONSTANT
    hyp = {e["two_wrong"]: 4, e["larger_depth"]: 0, e["two_sets"]: 16, e["f_zero"]: -1, e["masked"]: -1}       # two_wrong: {0, 4, 6} is the first right triple
    n_inl = {e["two_wrong"]: 6, e["larger_depth"]: 8, e["collinear_first"]: 8, e["coplanar"]: 10, e["two_sets"]: 8, e["f_zero"]: 0, e["masked"]: 0}
    zeros = [2, 5] + [8 + 8 + 8 + 12 + 12 + k for k in range(1, 16, 2)]
    return s, hyp, n_inl, np.array(sorted(zeros))
