"""numpy restatement of BAProblem.subset and BAProblem.window: what the device entries are held to (tests/test_gpu_subset.py,
tests/test_gpu_window.py) and what tests/test_subsetref.py holds to brute-force set arithmetic.  Indices and copies only."""
import numpy as np

CONST_ALL = 0x1ff


def subset_graph(row_ptr, pt_idx, n_pts, ci, pi):
    """(row_ptr', pt_idx', obs_of) of BAProblem::subset (src/baproblem.rs:394-423): cameras ci in the given order, a point
    named by its LAST slot in pi (HashMap::from_iter), observations of points outside pi dropped, row order kept.  obs_of =
    the parent observation behind every child observation.  This is the host routine BAProblem.subset ran before the device
    entry replaced it."""
    ci = np.asarray(ci, dtype=np.int64).reshape(-1)
    pi = np.asarray(pi, dtype=np.int64).reshape(-1)
    new_of = np.full(n_pts, -1, dtype=np.int64)
    new_of[pi] = np.arange(len(pi))                           # a repeated point keeps its last slot
    rows, cols, src = [0], [], []
    for c in ci:
        a, b = int(row_ptr[c]), int(row_ptr[c + 1])
        p_new = new_of[pt_idx[a:b].astype(np.int64)]
        k = p_new >= 0
        cols.append(p_new[k])
        src.append(np.arange(a, b, dtype=np.int64)[k])
        rows.append(rows[-1] + int(k.sum()))
    cols = np.concatenate(cols).astype(np.uint64) if cols else np.zeros(0, np.uint64)
    src = np.concatenate(src) if src else np.zeros(0, np.int64)
    return np.array(rows, dtype=np.uint64), cols, src


def subset(cams, pts, row_ptr, pt_idx, uv, ci, pi):
    """(cams', pts', row_ptr', pt_idx', uv') of subset on host arrays; cams is [n, 15] or [n, 9]"""
    ci = np.asarray(ci, dtype=np.int64).reshape(-1)
    pi = np.asarray(pi, dtype=np.int64).reshape(-1)
    rows, cols, src = subset_graph(row_ptr, pt_idx, len(pts), ci, pi)
    return cams[ci], pts[pi], rows, cols, np.asarray(uv).reshape(-1, 2)[src]


def as_seed(cameras, n_cam):
    a = np.asarray(cameras)
    if a.dtype == np.bool_:
        return a.copy()
    seed = np.zeros(n_cam, dtype=bool)
    seed[np.asarray(a, dtype=np.int64)] = True
    return seed


def window(row_ptr, pt_idx, n_pts, cameras, halo=True):
    """The window of the seed cameras (an index list or a bool mask).  S: the seeds; P: the points with an observation in a
    row of S; H (halo mode): the cameras outside S with an observation of a point of P; shared: the points of P with an
    observation outside S.  Child cameras S u H (halo) or S, ascending; child points P, ascending; a child row = the
    parent row's observations of P, in row order (a seed row is whole).  Returns dict(S, H, P, shared (indices, ascending),
    cam_of, pt_of, cam_role (1 halo), pt_role (1 shared, no-halo mode only), row_ptr, pt_idx, obs_of)."""
    n_cam = len(row_ptr) - 1
    seed = as_seed(cameras, n_cam)
    pt = np.asarray(pt_idx, dtype=np.int64)
    cam = np.repeat(np.arange(n_cam), np.diff(np.asarray(row_ptr, dtype=np.int64)))
    in_P = np.zeros(n_pts, dtype=bool)
    in_P[pt[seed[cam]]] = True
    rim = ~seed[cam] & in_P[pt]                               # observations of P from outside S
    is_halo = np.zeros(n_cam, dtype=bool)
    is_halo[cam[rim]] = True
    is_shared = np.zeros(n_pts, dtype=bool)
    is_shared[pt[rim]] = True
    cam_of = np.flatnonzero(seed | is_halo) if halo else np.flatnonzero(seed)
    pt_of = np.flatnonzero(in_P)
    rows, cols, obs_of = subset_graph(row_ptr, pt_idx, n_pts, cam_of, pt_of)
    return dict(S=np.flatnonzero(seed), H=np.flatnonzero(is_halo), P=pt_of, shared=np.flatnonzero(is_shared),
                cam_of=cam_of.astype(np.uint32), pt_of=pt_of.astype(np.uint32),
                cam_role=(~seed[cam_of]).astype(np.uint8),
                pt_role=np.zeros(len(pt_of), np.uint8) if halo else is_shared[pt_of].astype(np.uint8),
                row_ptr=rows, pt_idx=cols, obs_of=obs_of)


def window_masks(w, parent_cmask=None, parent_pmask=None):
    """(uint16 [n_cam'], uint8 [n_pts']) of the child: the parent's masks gathered, OR CONST_ALL on a halo camera, OR 1 on a
    shared point (no-halo mode)"""
    cm = np.zeros(len(w["cam_of"]), np.uint16) if parent_cmask is None else np.asarray(parent_cmask, np.uint16)[w["cam_of"]]
    pm = np.zeros(len(w["pt_of"]), np.uint8) if parent_pmask is None else np.asarray(parent_pmask, np.uint8)[w["pt_of"]]
    return cm | (w["cam_role"].astype(np.uint16) * CONST_ALL), pm | w["pt_role"]


def locality_grid():
    """The locality grid of the window tests: np_grid_layout(4, cpb=5, ppb=4, block_length=20.0), candidates within 10.0, the
    oracle's visibility predicate, nothing culled: 400 cameras, 960 points, 5 145 observations, rows of 0 .. 20 entries, 6 of
    them empty.  Returns (cams15, pts, row_ptr u64, pt_idx u64, uv)."""
    import oracle as O
    from _problems import np_candidate_pairs, np_grid_layout
    cams, pts = np_grid_layout(4, cpb=5, ppb=4, block_length=20.0)
    ci, pi = np_candidate_pairs(O.centers(cams), pts, 10.0)
    uv, keep = O.visibility_pairs(cams, pts, ci, pi, 10.0)
    ci, pi, uv = ci[keep == 1], pi[keep == 1], uv[keep == 1]
    counts = np.zeros(len(cams) + 1, dtype=np.int64)
    np.add.at(counts, ci.astype(np.int64) + 1, 1)
    return cams, pts, np.cumsum(counts).astype(np.uint64), pi.astype(np.uint64), np.ascontiguousarray(uv)


# window -> (seed cameras, halo cameras, points, shared points, child observations with halo, without); None: not stated
GRID_WINDOWS = {
    "37..100": (lambda n: np.arange(37, 101), (64, 76, 260, 179, 1470, 758)),
    "0..19": (lambda n: np.arange(0, 20), (20, 23, 78, 50, 412, 220)),
    "every 7th": (lambda n: np.arange(0, n, 7), (58, 283, 514, 514, None, None)),
    "all": (lambda n: np.arange(n), (400, 0, 960, 0, 5145, 5145)),
}
DOME_WINDOWS = {
    "0..9": (lambda n: np.arange(0, 10), (10, 70, 157, 149, None, None)),
    "77 alone": (lambda n: np.array([77]), (1, 0, 0, 0, 0, 0)),
}


def window_sizes(wh, wn):
    """the table's six numbers from the halo and the no-halo window of the same seeds"""
    return (len(wh["S"]), len(wh["H"]), len(wh["P"]), len(wh["shared"]), len(wh["pt_idx"]), len(wn["pt_idx"]))


def assert_sizes(got, want):
    for g, w in zip(got, want):
        assert w is None or g == w, (got, want)
