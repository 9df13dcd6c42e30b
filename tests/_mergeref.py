"""Host reference of landmark merging (BAProblem.merge_points / c2b_merge_partner_rows): one round and the loop,
restated in numpy.  Brute force over all pairs -- no cell grid --, the oracle's project_world / project for the predicate,
the same unfused expressions and the same (d2, q) order as the device, so every output is compared with ==.

One round on (cameras, points, the camera-major list), point p's row = its observations in ascending index:
  held (the mask) and unobserved (an empty row) points take no part;
  candidates of p: every other point q that takes part with d2(p, q) <= radius^2, d2 = (dx dx + dy dy) + dz dz, ordered by
  (d2, q);
  the pair (a, b) = (min, max) is verified when no camera is in both rows and every entry of both rows passes
  du du + dv dv <= max_error^2 and q.z < 0 at m = a + (b - a) * (nb / (na + nb));
  partner[p] = the first verified candidate, else -1; pairs with partner[partner[p]] == p merge onto the lower index.
`borderline` counts the predicate values within 4 ulp of max_error^2: a draw that has one is dropped by the tests."""
import numpy as np

import oracle as O

NONE, CHOSEN, UNOBSERVED, HELD = range(4)
STATUS = ("none", "chosen", "unobserved", "held")


def point_rows(row_ptr, pt_idx, n_pts):
    """per point: (observation indices ascending, their cameras)"""
    row_ptr = np.asarray(row_ptr).astype(np.int64)
    pt_idx = np.asarray(pt_idx).astype(np.int64)
    cam_of_obs = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    order = np.argsort(pt_idx, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pt_idx, minlength=n_pts))])
    return [(order[ptr[p]:ptr[p + 1]], cam_of_obs[order[ptr[p]:ptr[p + 1]]]) for p in range(n_pts)]


def distances2(pts):
    """d2[p, q] = (dx dx + dy dy) + dz dz, unfused"""
    d = pts[:, None, :] - pts[None, :, :]
    with np.errstate(all="ignore"):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def merge_position(A, B, na, nb):
    """a + (b - a) * f, f = nb / (na + nb): a subtraction, a product and a sum per coordinate"""
    f = np.float64(nb) / np.float64(na + nb)
    with np.errstate(all="ignore"):
        return A + (B - A) * f


def fits(cam15, ob, m, e2):
    """(the filter's predicate with in_front at m, r2)"""
    with np.errstate(all="ignore"):
        q = O.project_world(cam15, m)
        uv = O.project(cam15, q)
        du, dv = np.float64(uv[0]) - np.float64(ob[0]), np.float64(uv[1]) - np.float64(ob[1])
        r2 = du * du + dv * dv
    return bool(r2 <= e2 and q[2] < 0.0), float(r2)


def one_round(cams15, pts, row_ptr, pt_idx, uv, radius, max_error, held=None):
    """dict(partner int32 [n], status uint8 [n], counts {name: n}, into int64 [n], pts, pt_idx, merged, borderline, tested,
    rejected): the round's choice and the state after its merge (pts and pt_idx are new arrays)"""
    pts = np.asarray(pts, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n = len(pts)
    rows = point_rows(row_ptr, pt_idx, n)
    held = np.zeros(n, dtype=bool) if held is None else np.asarray(held).astype(bool)
    r2lim, e2 = np.float64(radius) * np.float64(radius), np.float64(max_error) * np.float64(max_error)
    status = np.full(n, NONE, dtype=np.uint8)
    status[[len(rows[p][0]) == 0 for p in range(n)]] = UNOBSERVED
    status[held] = HELD
    takes_part = status == NONE
    d2 = distances2(pts)
    verdict, stats = {}, dict(borderline=0, tested=0, rejected=0)

    def verified(a, b):
        if (a, b) in verdict:
            return verdict[(a, b)]
        (oa, ca), (ob, cb) = rows[a], rows[b]
        ok = not (set(ca.tolist()) & set(cb.tolist()))
        if ok:
            m = merge_position(pts[a], pts[b], len(oa), len(ob))
            for o, c in zip(np.concatenate([oa, ob]), np.concatenate([ca, cb])):
                good, r2 = fits(cams15[c], uv[o], m, e2)
                if abs(r2 - e2) <= 4.0 * np.spacing(e2):
                    stats["borderline"] += 1
                ok = ok and good
        stats["tested"] += 1
        stats["rejected"] += 0 if ok else 1
        verdict[(a, b)] = ok
        return ok

    partner = np.full(n, -1, dtype=np.int32)
    for p in np.flatnonzero(takes_part):
        with np.errstate(invalid="ignore"):
            near = np.flatnonzero(takes_part & (d2[p] <= r2lim))
        near = near[near != p]
        for q in sorted(near.tolist(), key=lambda q: (d2[p, q], q)):
            if verified(min(p, q), max(p, q)):
                partner[p] = q
                status[p] = CHOSEN
                break
    into = np.arange(n)
    new_pts = pts.copy()
    for a in range(n):
        b = int(partner[a])
        if b > a and partner[b] == a:
            new_pts[a] = merge_position(pts[a], pts[b], len(rows[a][0]), len(rows[b][0]))
            into[b] = a
    new_idx = into[np.asarray(pt_idx).astype(np.int64)]
    return dict(partner=partner, status=status, counts={k: int((status == i).sum()) for i, k in enumerate(STATUS)}, into=into, pts=new_pts,
                pt_idx=new_idx, merged=int((into != np.arange(n)).sum()), **stats)


def merge(cams15, pts, row_ptr, pt_idx, uv, radius, max_error, rounds=1, held=None):
    """the loop: dict(pts, pt_idx, map int32 [n], merged, rounds, per_round [merged of each round run], borderline, rejected)"""
    pts = np.asarray(pts, dtype=np.float64).copy()
    idx = np.asarray(pt_idx).astype(np.int64)
    total = np.arange(len(pts))
    out = dict(per_round=[], borderline=0, rejected=0)
    for _ in range(rounds):
        r = one_round(cams15, pts, row_ptr, idx, uv, radius, max_error, held)
        out["per_round"].append(r["merged"])
        out["borderline"] += r["borderline"]
        out["rejected"] += r["rejected"]
        if not r["merged"]:
            break
        pts, idx, total = r["pts"], r["pt_idx"], r["into"][total]
    out.update(pts=pts, pt_idx=idx, map=total.astype(np.int32), merged=int(sum(out["per_round"])), rounds=len(out["per_round"]))
    return out


# ---- the problems the CPU and GPU tests share ------------------------------------------------------------------------------
def simple_cameras(n, behind=()):
    """n cameras looking down -z from z = +10 (R = I, t = (tx, ty, -10)), f = 1 and no distortion; the cameras in `behind`
    stand at z = -10 instead, so that points near the origin are behind them"""
    cams = np.zeros((n, 15))
    cams[:, [0, 4, 8]] = 1.0
    cams[:, 9] = 0.3 * np.cos(np.arange(n) * 1.7)
    cams[:, 10] = 0.3 * np.sin(np.arange(n) * 2.3)
    cams[:, 11] = -10.0
    cams[list(behind), 11] = 10.0
    cams[:, 12] = 1.0
    return cams


def observe(cams15, seen_at, views):
    """the list of `views` = [(camera, point)] in camera-major order, stable inside a camera; each pixel is the oracle's
    projection of seen_at[point]: (row_ptr u64, pt_idx u64, uv)"""
    views = sorted(views, key=lambda cp: cp[0])
    n_cam = len(cams15)
    row_ptr = np.zeros(n_cam + 1, dtype=np.uint64)
    for c, _ in views:
        row_ptr[c + 1] += 1
    row_ptr = np.cumsum(row_ptr).astype(np.uint64)
    pt_idx = np.array([p for _, p in views], dtype=np.uint64)
    uv = np.array([O.project(cams15[c], O.project_world(cams15[c], np.asarray(seen_at[p], dtype=np.float64))) for c, p in views]).reshape(-1, 2)
    return row_ptr, pt_idx, uv


def split_dome(seed=0, split_seed=5, fraction=0.3, jitter=0.0):
    """dome_problem(dup=False, no noise) after the host split_landmarks of `fraction` of its points, point 0 forced into
    the split (a draw that leaves it out swaps it in for the first selected point): dict(P (the split problem, loadable),
    orig_pt_idx, n_orig, twin_of {original: copy}, both {originals whose two halves both kept an observation}).  jitter > 0
    moves every copy by a seeded normal of that scale."""
    import ctypes as C
    from _problems import dome_problem
    from city2ba_amd import _lib as L
    P = dome_problem(seed=seed, dup=False, obs_noise=0.0, start_noise=0.0)
    n = len(P["pts"])
    n_split = int(fraction * n)
    orig = P["pt_idx"].astype(np.uint64).copy()
    for s in range(split_seed, split_seed + 64):                 # the first seed at or after split_seed whose draw holds point 0
        buf = np.zeros((n + n_split + 1, 3))
        buf[:n] = P["pts"]
        idx = orig.copy()
        cnt = C.c_int64(n)
        L.check(L.lib().c2b_split_landmarks(C.byref(cnt), buf.ctypes.data_as(C.c_void_p), len(buf), len(idx), idx.ctypes.data_as(C.c_void_p),
                                            float(fraction), int(s)))
        pts = buf[:cnt.value].copy()
        if (pts[n:] == pts[0]).all(axis=1).any():
            break
    else:
        raise AssertionError("no seed split point 0")
    twin_of = {}
    for k in range(n, len(pts)):
        src = np.flatnonzero((pts[:n] == pts[k]).all(axis=1))
        assert len(src) == 1
        twin_of[int(src[0])] = k
    if jitter:
        pts[n:] += np.random.default_rng(split_seed + 1000).normal(scale=jitter, size=pts[n:].shape)
    seen = np.bincount(idx.astype(np.int64), minlength=len(pts)) > 0
    both = {a for a, b in twin_of.items() if seen[a] and seen[b]}
    Q = dict(P)
    Q.update(pts=pts, pt_idx=idx, true_pts=None)
    return dict(P=Q, orig_pt_idx=orig, n_orig=n, twin_of=twin_of, both=both, split_seed=s)
