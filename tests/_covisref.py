"""Host reference of the camera covisibility graph and of the search over it (BAProblem.covisibility / neighbourhood),
in numpy.  shared(c, c'), c != c', = the number of distinct points with an observation in row c and one in row c'; the graph
at min_shared is the symmetric CSR (nbr_ptr u64, nbr u32 ascending inside a row, shared u32) of the pairs with shared >=
min_shared.  Integers only: the device is held to these arrays exactly."""
import numpy as np


def cam_of_rows(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))


def graph(row_ptr, pt_idx, min_shared=1):
    """(nbr_ptr [n_cam + 1] uint64, nbr [n_edges] uint32, shared [n_edges] uint32): unique (camera, point) pairs, per point every
    ordered pair of its distinct cameras, np.unique of the pairs with counts"""
    n_cam = len(row_ptr) - 1
    cam = cam_of_rows(row_ptr)
    pt = np.asarray(pt_idx, dtype=np.int64)
    out_a, out_b = [np.empty(0, dtype=np.int64)], [np.empty(0, dtype=np.int64)]
    if len(pt):
        pair = np.unique(pt * n_cam + cam)                   # sorted by point, then camera: duplicates of (camera, point) gone
        p, c = pair // n_cam, pair % n_cam
        start = np.flatnonzero(np.concatenate([[True], p[1:] != p[:-1]]))
        length = np.diff(np.concatenate([start, [len(p)]]))
        for n in np.unique(length):
            if n < 2:
                continue
            s = start[length == n]
            block = c[s[:, None] + np.arange(n)[None, :]]    # [tracks of this length, n]
            a = np.repeat(block, n, axis=1).reshape(-1)
            b = np.tile(block, (1, n)).reshape(-1)
            keep = a != b
            out_a.append(a[keep])
            out_b.append(b[keep])
    a, b = np.concatenate(out_a), np.concatenate(out_b)
    key, count = np.unique(a * max(n_cam, 1) + b, return_counts=True)
    key, count = key[count >= min_shared], count[count >= min_shared]
    row, col = key // max(n_cam, 1), key % max(n_cam, 1)
    nbr_ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n_cam))]).astype(np.uint64)
    return nbr_ptr, col.astype(np.uint32), count.astype(np.uint32)


def figures(nbr_ptr):
    """(undirected edges, maximum degree, isolated cameras) of a graph"""
    deg = np.diff(np.asarray(nbr_ptr, dtype=np.int64))
    return int(deg.sum()) // 2, int(deg.max()) if len(deg) else 0, int(np.sum(deg == 0))


def neighbourhood(g, seeds, hops=1, max_cameras=None, within=None):
    """level [n_cam] int32 (-1 = not reached) of the search over the graph g = (nbr_ptr, nbr, shared) from the seed cameras:
    level 0 = the seeds; level h + 1 = the cameras not reached yet, inside `within` (a bool mask, or None), with an edge to
    level h; at most `hops` levels beyond the seeds (None: until nothing new).  With max_cameras whole levels are taken while
    they fit; the first that does not fit is ranked by (score descending, index ascending), score = min(the sum of shared over
    the candidate's edges into the levels already taken, 2^32 - 1), its best fill the remainder and the search ends."""
    nbr_ptr, nbr, shared = (np.asarray(x, dtype=np.int64) for x in g)
    n_cam = len(nbr_ptr) - 1
    level = np.full(n_cam, -1, dtype=np.int32)
    seeds = np.unique(np.asarray(seeds, dtype=np.int64))
    level[seeds] = 0
    ok = np.ones(n_cam, dtype=bool) if within is None else np.asarray(within, dtype=bool)
    taken, front, h = len(seeds), seeds, 0
    while (hops is None or h < hops) and len(front) and not (max_cameras and taken == max_cameras):
        reach = np.unique(np.concatenate([nbr[nbr_ptr[c]:nbr_ptr[c + 1]] for c in front] + [np.empty(0, dtype=np.int64)]))
        new = reach[(level[reach] < 0) & ok[reach]]
        if not len(new):
            break
        if max_cameras and taken + len(new) > max_cameras:
            score = np.empty(len(new), dtype=np.int64)
            for i, c in enumerate(new):
                e = slice(nbr_ptr[c], nbr_ptr[c + 1])
                score[i] = min(int(shared[e][level[nbr[e]] >= 0].sum()), 2 ** 32 - 1)
            order = np.lexsort((new, -score))
            level[new[order[:max_cameras - taken]]] = h + 1
            break
        level[new] = h + 1
        taken += len(new)
        front, h = new, h + 1
    return level


def row_bounds(row_ptr, pt_idx, n_pts):
    """per camera the bound the device sorts cameras by: the sum over the row of (track length - 1)"""
    track = np.bincount(np.asarray(pt_idx, dtype=np.int64), minlength=n_pts)
    per_obs = track[np.asarray(pt_idx, dtype=np.int64)] - 1
    return np.add.reduceat(np.concatenate([per_obs, [0]]), np.minimum(np.asarray(row_ptr[:-1], dtype=np.int64), len(per_obs))) * (np.diff(np.asarray(row_ptr, dtype=np.int64)) > 0)


def _lists(rows):
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    pt_idx = np.concatenate([np.asarray(r, dtype=np.uint64) for r in rows] + [np.empty(0, dtype=np.uint64)])
    return row_ptr, pt_idx


def hub_list(degree, tight, seed=0):
    """(row_ptr u64, pt_idx u64, n_pts): camera 0 with `degree` neighbours, cameras 1 .. degree, met in a seeded shuffled order
    (its row is shuffled), never in ascending index.
    tight = False: camera 0 shares 1 .. 5 points of its own with each neighbour (neighbour k: 1 + k % 5), so shared runs over
    1 .. 5 in its row and its bound is the sum of them.
    tight = True: ONE point seen by camera 0 and every neighbour, so camera 0's bound equals its degree exactly -- a bound is at
    least the sum of the row's shared counts, so at bound == degree every count of the row is 1 --; shared still runs over 1 .. 5
    in the list: neighbours 2j + 1 and 2j + 2 share j % 5 further points of their own."""
    rng = np.random.default_rng(seed + degree)
    rows = [[] for _ in range(degree + 1)]
    p = 0
    if tight:
        for r in rows:
            r.append(0)
        p = 1
        for j in range(degree // 2):
            for _ in range(j % 5):
                rows[2 * j + 1].append(p)
                rows[2 * j + 2].append(p)
                p += 1
        for r in rows[1:]:
            rng.shuffle(r)
    else:
        for cam in rng.permutation(degree) + 1:
            for _ in range(1 + int(cam) % 5):
                rows[0].append(p)
                rows[int(cam)].append(p)
                p += 1
        rng.shuffle(rows[0])
    return _lists(rows) + (p,)


def collision_list(stride=1 << 16, degree=64):
    """camera stride * degree with the neighbours j * stride, j < degree, one point each (shared 1 .. 3: point j is listed by
    its pair only, 1 + j % 3 points a pair); every other row is empty: n_cam = stride * degree + 1.  Indices that agree in their
    low 16 bits: a table that hashes by the low bits puts them all in one slot."""
    n_cam = stride * degree + 1
    lengths = np.zeros(n_cam, dtype=np.int64)
    hub, pts_of = [], {}
    p = 0
    for j in range(degree):
        pts_of[j * stride] = list(range(p, p + 1 + j % 3))
        hub += pts_of[j * stride]
        p += 1 + j % 3
        lengths[j * stride] = 1 + j % 3
    lengths[n_cam - 1] = len(hub)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    pt_idx = np.concatenate([np.asarray(pts_of[j * stride]) for j in range(degree)] + [np.asarray(hub[::-1])]).astype(np.uint64)
    return row_ptr, pt_idx, p


def heavy_only_list(n_cam):
    """one point seen by every one of n_cam cameras: the complete graph, every shared 1, every camera's bound n_cam - 1"""
    return np.arange(n_cam + 1, dtype=np.uint64), np.zeros(n_cam, dtype=np.uint64), 1
