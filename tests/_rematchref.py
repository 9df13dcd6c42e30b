"""Host reference of guided re-matching (BAProblem.rematch_observations / c2b_rematch_rows), restated in numpy.
Brute force over all (observation, point) pairs -- no cell grid --, the oracle's projection for the predicate, the same
unfused expressions and the same keys as the device, so every output is compared with ==.

E2 = max_error^2, R2 = radius^2.  fit(o, q): r2(o, q) = du du + dv dv <= E2 and q.z < 0 for point q through o's camera.
  1 fits[o] = fit(o, pt_idx[o]);
  2 trusted[p] = p finite and at least min_fits observations that name p fit it;
  3 o is FITS if it fits, else SKIPPED if its label is not trusted, else failing; FITS and SKIPPED stay, their labels are held
    in their camera;
  4 candidates of a failing o with label p: trusted q != p, not held in o's camera, fit(o, q), and d2(p, q) <= R2 or q is the
    label of a failing observation of the camera;
  5 choice[o] = the candidate with the smallest (r2(o, q), q), -1 without one;
  6 of the failing observations of a camera with one choice the smallest (r2, o) is REASSIGNED, every other failing one REMOVED;
  7 pt_idx[o] = choice[o] where REASSIGNED, then the list is compacted by status != REMOVED, stable inside every row.
r2 >= 0, so the order of the doubles is the order of their bits.

An observation is EXCUSED when a decision taken for it lies within CAP (relative) of its threshold -- see excused()."""
import numpy as np

import _mergeref as M
import _triangref as T
import oracle as O

FITS, SKIPPED, REASSIGNED, REMOVED = range(4)
STATUS = ("fits", "skipped", "reassigned", "removed")
CAP = T.CAP


def fit_tables(cams15, pts, row_ptr, uv, e2):
    """(r2 [n_obs, n_pts], fit [n_obs, n_pts] bool, qz [n_obs, n_pts]: the oracle's q.z where r2 <= E2, NaN elsewhere, cam_of).
    The pixels are the oracle's project(project_world()) of every point through every camera (its batch entry), q.z its
    project_world where the sign decides."""
    cams15 = np.ascontiguousarray(cams15, dtype=np.float64).reshape(-1, 15)
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n_cam, n = len(cams15), len(pts)
    cam_of = np.repeat(np.arange(n_cam), np.diff(np.asarray(row_ptr).astype(np.int64)))
    if not len(uv) or not n:
        z = np.zeros((len(uv), n))
        return z, z.astype(bool), z, cam_of
    every = O.project_observations(cams15, pts, np.arange(n_cam + 1, dtype=np.uint64) * np.uint64(n),
                                   np.tile(np.arange(n, dtype=np.uint64), n_cam)).reshape(n_cam, n, 2)
    with np.errstate(all="ignore"):
        du, dv = every[cam_of, :, 0] - uv[:, None, 0], every[cam_of, :, 1] - uv[:, None, 1]
        r2 = du * du + dv * dv
        near = r2 <= e2
    qz = np.full(r2.shape, np.nan)
    for o, q in np.argwhere(near):
        qz[o, q] = O.project_world(cams15[cam_of[o]], pts[q])[2]
    with np.errstate(invalid="ignore"):
        fit = near & (qz < 0.0)
    return r2, fit, qz, cam_of


def reference(cams15, pts, row_ptr, pt_idx, uv, radius, max_error, min_fits=2, trusted=None, on_purpose=()):
    """dict(fits, trusted, choice int32, status uint8, counts {name: n}, pt_idx, uv, row_ptr (the list after the call), keep,
    excused (observation indices), several (observations with more than one candidate)).  `trusted` given: rule 2 is the
    caller's (Level 0).  on_purpose: what a hand-built problem sets at its threshold deliberately and is therefore no excuse:
    "radius" (a distance equal to the radius, or the next double beyond it), "r2" (two r2 with equal bits)."""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    rp = np.asarray(row_ptr).astype(np.int64)
    lab = np.asarray(pt_idx).astype(np.int64)
    n, n_obs = len(pts), len(lab)
    e2, r2lim = np.float64(max_error) * np.float64(max_error), np.float64(radius) * np.float64(radius)
    r2, fit, qz, cam_of = fit_tables(cams15, pts, rp, uv, e2)
    own = np.arange(n_obs)
    fits = fit[own, lab] if n_obs else np.zeros(0, dtype=bool)
    if trusted is None:
        trusted = np.isfinite(pts).all(axis=1) & (np.bincount(lab[fits], minlength=n) >= min_fits)
    trusted = np.asarray(trusted).astype(bool)
    status = np.where(fits, FITS, np.where(trusted[lab], REMOVED, SKIPPED)).astype(np.uint8) if n_obs else np.zeros(0, dtype=np.uint8)
    failing = (status == REMOVED)
    d2 = M.distances2(pts)
    choice = np.full(n_obs, -1, dtype=np.int32)
    cands = {}
    for c in range(len(rp) - 1):
        row = np.arange(rp[c], rp[c + 1])
        held = set(lab[row[~failing[row]]].tolist())
        given_up = np.zeros(n, dtype=bool)
        given_up[lab[row[failing[row]]]] = True
        for o in row[failing[row]]:
            p = lab[o]
            with np.errstate(invalid="ignore"):
                ok = trusted & fit[o] & ((d2[p] <= r2lim) | given_up)
            ok[p] = False
            cand = [int(q) for q in np.flatnonzero(ok) if int(q) not in held]
            cands[int(o)] = cand
            if cand:
                choice[o] = min(cand, key=lambda q: (r2[o, q], q))
        claimed = {}
        for o in row[failing[row]]:
            if choice[o] >= 0:
                claimed.setdefault(int(choice[o]), []).append(int(o))
        for q, os_ in claimed.items():
            status[min(os_, key=lambda o: (r2[o, q], o))] = REASSIGNED
    keep = status != REMOVED
    new_lab = np.where(status == REASSIGNED, choice.astype(np.int64), lab)
    new_rp = np.concatenate([[0], np.cumsum(np.bincount(cam_of[keep], minlength=len(rp) - 1))]).astype(np.uint64)
    out = dict(fits=fits, trusted=trusted, choice=choice, status=status, counts={k: int((status == i).sum()) for i, k in enumerate(STATUS)},
               pt_idx=new_lab[keep].astype(np.uint64), uv=uv[keep], row_ptr=new_rp, keep=keep,
               several=[o for o, cd in cands.items() if len(cd) > 1])
    out["excused"] = excused(r2, fit, qz, d2, lab, trusted, failing, cands, choice, status, cam_of, cams15, pts, e2, r2lim, on_purpose)
    return out


def _close(a, b, equal_is_meant=False):
    """|a - b| <= CAP max(|a|, |b|) (a NaN is far from everything)"""
    with np.errstate(invalid="ignore"):
        near = np.abs(a - b) <= CAP * np.maximum(np.abs(a), np.abs(b))
        return near & (a != b) if equal_is_meant else near


def excused(r2, fit, qz, d2, lab, trusted, failing, cands, choice, status, cam_of, cams15, pts, e2, r2lim, on_purpose):
    """The observations for which a decision lies within CAP (relative) of its threshold:
      an r2 against E2, for the observation's own label and for any trusted point;
      |q.z| <= CAP |q| where r2 <= E2 (own label or a trusted point);
      for a failing observation, a d2(label, q) against R2 for a trusted q it reprojects within E2 of (elsewhere the
      distance decides nothing) -- unless the problem sets the radius there on purpose;
      two candidates of one observation, or two claimants of one point, whose r2 differ by less than CAP relative -- unless
      the bits are equal by construction."""
    n_obs = len(lab)
    bad = np.zeros(n_obs, dtype=bool)
    if not n_obs:
        return []
    judged = np.tile(trusted, (n_obs, 1))
    judged[np.arange(n_obs), lab] = True
    bad |= (_close(r2, e2) & judged).any(axis=1)
    for o, q in np.argwhere(np.isfinite(qz) & judged):
        v = O.project_world(cams15[cam_of[o]], pts[q])
        if abs(v[2]) <= CAP * np.linalg.norm(v):
            bad[o] = True
    for o in np.flatnonzero(failing):
        with np.errstate(invalid="ignore"):
            within = trusted & (r2[o] <= e2)
        within[lab[o]] = False
        if "radius" not in on_purpose and _close(d2[lab[o]], r2lim)[within].any():
            bad[o] = True
        cd = cands[int(o)]
        for i, a in enumerate(cd):
            for b in cd[i + 1:]:
                if _close(r2[o, a], r2[o, b], "r2" in on_purpose):
                    bad[o] = True
    for q in set(choice[choice >= 0].tolist()):
        os_ = np.flatnonzero(choice == q)
        for i, a in enumerate(os_):
            for b in os_[i + 1:]:
                if cam_of[a] == cam_of[b] and _close(r2[a, q], r2[b, q], "r2" in on_purpose):
                    bad[a] = bad[b] = True
    return np.flatnonzero(bad).tolist()


def seen_twice(row_ptr, pt_idx):
    """the (camera, point) pairs that occur more than once in the list"""
    rp = np.asarray(row_ptr).astype(np.int64)
    cam_of = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    pairs, count = np.unique(np.stack([cam_of, np.asarray(pt_idx).astype(np.int64)], axis=1), axis=0, return_counts=True)
    return {tuple(p) for p in pairs[count > 1].tolist()}


# ---- the problems the CPU and GPU tests share ------------------------------------------------------------------------------
DOME_CASES = T.DOME_CASES
MAX_ERROR, MIN_FITS = 0.01, 2
JOIN_SEED, JOIN_CHANCE, JOIN_NEIGHBOURS = 11, 0.05, 4


def wrong_label_dome(state, obs_noise):
    """_triangrobustref.wrong_match_dome (swaps inside a camera) with the points at the truth -- a repair judges observations
    against established points -- and joins on top: through the observations in order, with chance JOIN_CHANCE an observation
    takes the label of one of the JOIN_NEIGHBOURS nearest other points of its TRUE point.  Adds radius = the largest distance
    from a point to its JOIN_NEIGHBOURS-th nearest neighbour, wrong = (pt_idx != true_pt_idx)."""
    import _triangrobustref as R
    P = R.wrong_match_dome(state, obs_noise)
    P["pts"] = P["true_pts"].copy()
    d2 = M.distances2(P["pts"])
    np.fill_diagonal(d2, np.inf)
    nearest = np.argsort(d2, axis=1, kind="stable")[:, :JOIN_NEIGHBOURS]
    rng = np.random.default_rng(JOIN_SEED)
    pt = P["pt_idx"].copy()
    true = P["true_pt_idx"].astype(np.int64)
    for o in range(len(pt)):
        if rng.random() < JOIN_CHANCE:
            pt[o] = nearest[true[o], int(rng.integers(0, JOIN_NEIGHBOURS))]
    P["pt_idx"] = pt
    P["wrong"] = pt != P["true_pt_idx"]
    P["radius"] = float(np.sqrt(np.sort(d2, axis=1)[:, JOIN_NEIGHBOURS - 1].max()))
    return P


def edge_cameras(n):
    """n cameras (_triangref._cam: R = I, looking down -z) on a ring at z = 10: points near the origin are in front of all"""
    return np.array([T._cam([3.0 * np.cos(1.3 * k), 3.0 * np.sin(2.1 * k), 10.0 + 0.25 * (k % 5)], f=1.0 + 0.01 * (k % 7)) for k in range(n)])


def observe(cams15, pts, views):
    """the list of `views` = [(camera, label, seen)] in camera-major order, stable inside a camera: the pixel is the oracle's
    projection of pts[seen] (or of `seen` itself when it is a position; ("uv", u, v) gives the pixel outright), the point
    index is `label`: (row_ptr u64, pt_idx u64, uv)"""
    pts = np.asarray(pts, dtype=np.float64)
    views = sorted(views, key=lambda v: v[0])
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount([v[0] for v in views], minlength=len(cams15)))]).astype(np.uint64)
    uv = np.zeros((len(views), 2))
    for i, (c, _, seen) in enumerate(views):
        if isinstance(seen, tuple):                          # ("uv", u, v): the pixel itself
            uv[i] = seen[1:]
            continue
        X = pts[seen] if np.isscalar(seen) else np.asarray(seen, dtype=np.float64)
        with np.errstate(all="ignore"):
            uv[i] = O.project(cams15[c], O.project_world(cams15[c], X))
    return row_ptr, np.array([v[1] for v in views], dtype=np.uint64), uv


# ---- the edge set: hand-built problems with the expected outputs written out -------------------------------------------------
EDGE_MAX_ERROR = 1e-3                                        # a pixel 1e-3 off is about 0.01 in the world at these depths


class _Edge:
    """Test cameras 0 .. n_test - 1 (edge_cameras unless replaced), then two support cameras that see the points as they are
    -- the first every finite point, the second every trusted one, so a trusted point has two fitting observations and an
    untrusted one a single one -- and a last camera that sees nothing.  see() takes the expected (status, choice) of the
    observation: `base`, and where they differ at min_fits = 0 (`min0`) or just inside the radius (`beyond`)."""

    def __init__(self, n_test):
        self.n_test = n_test
        self.cams = edge_cameras(n_test + 3)
        self.pts, self.trust, self.views, self.expect = [], [], [], []

    def pt(self, xyz, trusted=True):
        self.pts.append(np.asarray(xyz, dtype=np.float64))
        self.trust.append(trusted)
        return len(self.pts) - 1

    def see(self, cam, label, seen, base, min0=None, beyond=None):
        self.views.append((cam, label, seen))
        self.expect.append(dict(base=base, min0=min0 or base, beyond=beyond or base))

    def done(self, **settings):
        s1, s2 = self.n_test, self.n_test + 1
        for q, X in enumerate(self.pts):
            if np.isfinite(X).all():
                self.see(s1, q, q, (FITS, -1))
                if self.trust[q]:
                    self.see(s2, q, q, (FITS, -1))
        order = sorted(range(len(self.views)), key=lambda i: self.views[i][0])          # stable: observe()'s order
        pts = np.array(self.pts).reshape(-1, 3)
        row_ptr, pt_idx, uv = observe(self.cams, pts, self.views)
        want = {v: (np.array([self.expect[i][v][0] for i in order], dtype=np.uint8), np.array([self.expect[i][v][1] for i in order], dtype=np.int32))
                for v in ("base", "min0", "beyond")}
        return dict(cams15=self.cams, pts=pts, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv, want=want, max_error=EDGE_MAX_ERROR, bal=False, **settings)


def _at(a, dx=0.0, dy=0.0, dz=0.0):
    return np.asarray(a, dtype=np.float64) + [dx, dy, dz]


def edge_swaps():
    """radius 0: a two-observation swap (camera 0), a three-cycle (camera 2), a row of 130 entries whose entries 100 and
    120 are swapped (camera 3: the failing entry and the failing label that is its answer both lie past entry 64); cameras 1
    and 4 and the last one see nothing"""
    E = _Edge(5)
    A, B = E.pt([-3.0, -3.0, 0.0]), E.pt([-2.0, -3.0, 0.0])
    E.see(0, B, A, (REASSIGNED, A))
    E.see(0, A, B, (REASSIGNED, B))
    A, B, C = E.pt([0.0, -3.0, 0.0]), E.pt([1.0, -3.0, 0.0]), E.pt([2.0, -3.0, 0.1])
    E.see(2, B, A, (REASSIGNED, A))
    E.see(2, C, B, (REASSIGNED, B))
    E.see(2, A, C, (REASSIGNED, C))
    grid = [E.pt([-3.0 + 0.5 * (k % 13), -1.5 + 0.5 * (k // 13), 0.05 * (k % 3)]) for k in range(130)]
    for k in range(130):
        label = grid[120] if k == 100 else grid[100] if k == 120 else grid[k]
        E.see(3, label, grid[k], (FITS, -1) if label == grid[k] else (REASSIGNED, grid[k]))
    return E.done(radius=0.0)


def edge_neighbours():
    """radius 0.5, one camera per case (the docstring of tests/test_rematchref.py lists them); `beyond`: the same problem at
    the next radius below 0.5"""
    E = _Edge(12)
    anchor = [np.array([-3.0 + 1.5 * (k % 4), -3.0 + 1.5 * (k // 4), 0.0]) for k in range(16)]
    # 0 a join: the true point within the radius, unseen by the camera
    a = anchor[0]
    P, A = E.pt(_at(a, 0.4)), E.pt(a)
    E.see(0, P, A, (REASSIGNED, A))
    # 1 the distance equal to the radius: dx = 0.5 exactly, d2 == R2
    a = anchor[1]
    P, A = E.pt(_at(a, 0.5)), E.pt(a)
    E.see(1, P, A, (REASSIGNED, A), beyond=(REMOVED, -1))
    # 2 the best candidate held by an observation that fits: the second is taken
    a = anchor[2]
    P, Q1, Q2 = E.pt(_at(a, 0.3)), E.pt(a), E.pt(_at(a, 0.004))
    E.see(2, P, _at(a, 0.001), (REASSIGNED, Q2))
    E.see(2, Q1, Q1, (FITS, -1))
    # 3 the best candidate named by a skipped observation: it is untrusted, so it is no candidate; at min_fits = 0 it is trusted,
    #   the observation that named it fails and gives it up
    a = anchor[3]
    P, Q1, Q2 = E.pt(_at(a, 0.3)), E.pt(a, trusted=False), E.pt(_at(a, 0.004))
    E.see(3, P, _at(a, 0.001), (REASSIGNED, Q2), min0=(REASSIGNED, Q1))
    E.see(3, Q1, _at(a, 0.0, 0.7), (SKIPPED, -1), min0=(REMOVED, -1))
    # 4 two failing observations claim one point: the lower r2 wins
    a = anchor[4]
    Q, P1, P2 = E.pt(a), E.pt(_at(a, 0.3)), E.pt(_at(a, 0.0, 0.3))
    E.see(4, P1, _at(a, 0.002), (REMOVED, Q))
    E.see(4, P2, _at(a, 0.001), (REASSIGNED, Q))
    # 5 the same with mirror-image pixels (the camera straight above the point, at the origin): equal bits, the lower o wins
    a = anchor[10]
    assert not a.any()
    E.cams[5] = T._cam([0.0, 0.0, 10.0])
    Q, P1, P2 = E.pt(a), E.pt(_at(a, 0.3)), E.pt(_at(a, 0.0, 0.3))
    E.see(5, P1, _at(a, 0.002), (REASSIGNED, Q))
    E.see(5, P2, _at(a, -0.002), (REMOVED, Q))
    # 6 an untrusted label is skipped; trusted at min_fits = 0, it is put right
    a = anchor[5]
    U, A = E.pt(a, trusted=False), E.pt(_at(a, 0.3))
    E.see(6, U, A, (SKIPPED, -1), min0=(REASSIGNED, A))
    # 7 an untrusted candidate is never chosen
    a = anchor[6]
    P, U = E.pt(_at(a, 0.3)), E.pt(a, trusted=False)
    E.see(7, P, U, (REMOVED, -1), min0=(REASSIGNED, U))
    # 8 a candidate behind the camera: its pixel is met exactly, q.z > 0
    a = anchor[7]
    E.cams[8] = T._cam(_at(a, 0.3, 0.2, -10.0))
    P, Q = E.pt(_at(a, 0.3)), E.pt(a)
    E.see(8, P, Q, (REMOVED, -1))
    # 9 a NaN point: never trusted, whatever min_fits is; the camera's other observation is put right
    a = anchor[8]
    N, P, A = E.pt([np.nan, a[1], 0.0]), E.pt(_at(a, 0.3)), E.pt(a)
    E.see(9, N, A, (SKIPPED, -1))
    E.see(9, P, _at(a, 0.0005), (REASSIGNED, A))
    # 10 an f = 0 camera projects everything to (0, 0): that pixel fits, any other fits nothing
    a = anchor[9]
    E.cams[10] = T._cam([1.0, -2.0, 10.0], f=0.0)
    A, B = E.pt(a), E.pt(_at(a, 0.3))
    E.see(10, A, ("uv", 0.0, 0.0), (FITS, -1))
    E.see(10, B, ("uv", 0.05, 0.0), (REMOVED, -1))
    # 11 80 points within the radius that all fit; 79 are held by fitting observations, the last in key order is taken
    a = anchor[15]
    P = E.pt(_at(a, 0.3))
    Q = [E.pt(_at(a, 1e-4 * k)) for k in range(80)]
    for k in range(79):
        E.see(11, Q[k], Q[k], (FITS, -1))
    E.see(11, P, _at(a, -1e-4), (REASSIGNED, Q[79]))
    return E.done(radius=0.5)


def edge_cells():
    """radius 0.5, three by three cells over x / z: the label in the middle cell and the answer in each of the other eight
    (cameras 0 .. 7), and answers on the extent's minimum and maximum (cameras 8 and 9)"""
    r = 0.5
    E = _Edge(10)
    centre = np.array([1.5 * r, 0.0, 1.5 * r])
    ring = [(dx, dz) for dx in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dz) != (0, 0)]
    lo, lo2, hi, hi2, mid = E.pt([0, 0, 0]), E.pt([0, 0.5 * r, 0]), E.pt([3 * r, 0, 3 * r]), E.pt([3 * r, 0.5 * r, 3 * r]), E.pt(centre)
    for k, (dx, dz) in enumerate(ring):
        q = E.pt(_at(centre, 0.6 * r * dx, 0.0, 0.6 * r * dz))
        E.see(k, mid, q, (REASSIGNED, q))
    E.see(8, lo2, lo, (REASSIGNED, lo))
    E.see(9, hi2, hi, (REASSIGNED, hi))
    return E.done(radius=r)


def edge_one_camera():
    """one camera, min_fits = 0: a swap and an observation that fits"""
    cams = np.array([T._cam([0.3, -0.2, 10.0], f=1.1, k1=1e-2, k2=-2e-3)])
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.2]])
    row_ptr, pt_idx, uv = observe(cams, pts, [(0, 1, 0), (0, 0, 1), (0, 2, 2)])
    want = (np.array([REASSIGNED, REASSIGNED, FITS], dtype=np.uint8), np.array([0, 1, -1], dtype=np.int32))
    return dict(cams15=cams, pts=pts, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv, want=dict(min0=want), max_error=EDGE_MAX_ERROR, radius=0.0, bal=False)


# (problem, variant): the settings every edge run uses
EDGE_RUNS = [("swaps", "base"), ("neighbours", "base"), ("neighbours", "min0"), ("neighbours", "beyond"), ("cells", "base"), ("one_camera", "min0")]
EDGE_PROBLEMS = dict(swaps=edge_swaps, neighbours=edge_neighbours, cells=edge_cells, one_camera=edge_one_camera)


def edge_run(name, variant):
    """(problem, radius, max_error, min_fits, on_purpose) of an edge run"""
    P = EDGE_PROBLEMS[name]()
    radius = float(np.nextafter(P["radius"], 0.0)) if variant == "beyond" else P["radius"]
    return P, radius, P["max_error"], 0 if variant == "min0" else MIN_FITS, ("radius", "r2") if name == "neighbours" else ()
