"""The index noise of DESIGN 4.18 restated in plain numpy: the four passes the device runs in place (csrc/index_noise_kernels.hpp),
defined by counter-based draws.  Nothing here is shaped like the kernels: selections are a lexsort on (a, index), the neighbours
are brute force over all pairs, the swaps are a Python loop.

The draws: Philox4x32-10 as normal_pair uses it (tests/_noiseref.py: philox4x32_10): counter = (entity lo, entity hi, slot, stream),
key = the seed's halves; a = o1 << 32 | o0, b = o3 << 32 | o2; u(x) = (x >> 11) * 2^-53."""
import numpy as np

from _noiseref import philox4x32_10

STREAM_DROP, STREAM_MISMATCH, STREAM_SPLIT, STREAM_JOIN = 6, 7, 8, 9
NEAREST = 11


def draws(seed, stream, entities, slot):
    """(a, b) uint64 of the block (seed; stream, entity, slot)"""
    ent = np.asarray(entities, dtype=np.uint64)
    o = philox4x32_10(ent, ent >> np.uint64(32), slot, stream, int(seed), int(seed) >> 32)
    return (o[1] << np.uint64(32)) | o[0], (o[3] << np.uint64(32)) | o[2]


def uniform(x):
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def smallest(keys, n):
    """bool mask of the n smallest (key, index)"""
    keys = np.asarray(keys, dtype=np.uint64)
    sel = np.zeros(len(keys), dtype=bool)
    n = max(0, min(int(n), len(keys)))
    sel[np.lexsort((np.arange(len(keys)), keys))[:n]] = True
    return sel


def fraction_count(fraction, count, cap):
    v = np.float64(fraction) * np.float64(count)
    if not v > 0.0:
        return 0
    return int(cap) if v >= cap else int(np.floor(v))


# ---- drop ---------------------------------------------------------------------------------------------------------------
def drop_keep(row_ptr, keep_fraction, seed):
    """bool keep [n_obs]: row of len entries keeps the floor(len * keep_fraction) (saturating) smallest (a, index)"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_obs = int(row_ptr[-1])
    a, _ = draws(seed, STREAM_DROP, np.arange(n_obs), 0)
    keep = np.zeros(n_obs, dtype=bool)
    for c in range(len(row_ptr) - 1):
        b, e = int(row_ptr[c]), int(row_ptr[c + 1])
        keep[b:e] = smallest(a[b:e], fraction_count(keep_fraction, e - b, e - b))
    return keep


def drop_features(row_ptr, pt_idx, uv, keep_fraction, seed):
    keep = drop_keep(row_ptr, keep_fraction, seed)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    cam_of = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    rows = np.concatenate([[0], np.cumsum(np.bincount(cam_of[keep], minlength=len(row_ptr) - 1))]).astype(np.uint64)
    return rows, np.asarray(pt_idx)[keep], np.asarray(uv).reshape(-1, 2)[keep]


# ---- mismatch -----------------------------------------------------------------------------------------------------------
def swap_weights(uv_row, i):
    """w_k = max_d - d_ik (w_i = max_d: the reference's zeroed-before-shift quirk, src/noise.rs:203-205)"""
    d = uv_row - uv_row[i]
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return dist.max() - dist


def mismatch_partner(row_ptr, uv, chance, seed, margin=1e-9):
    """(partner [n_obs] int32: row-relative j or -1, zero_rows: cameras counted, ambiguous: cameras in which a draw's
    u(b) * total lies within margin * total of a cumulative boundary)"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n_obs = int(row_ptr[-1])
    a, b = draws(seed, STREAM_MISMATCH, np.arange(n_obs), 0)
    ua, ub = uniform(a), uniform(b)
    partner = np.full(n_obs, -1, dtype=np.int32)
    zero_rows, ambiguous = set(), set()
    for c in range(len(row_ptr) - 1):
        lo, hi = int(row_ptr[c]), int(row_ptr[c + 1])
        if hi - lo <= 1:
            continue
        row = uv[lo:hi]
        for i in np.nonzero(ua[lo:hi] <= chance)[0]:
            w = swap_weights(row, i)
            cum = np.cumsum(w)
            total = cum[-1]
            if not total > 0.0:
                zero_rows.add(c)
                continue
            thr = ub[lo + i] * total
            over = np.nonzero(thr < cum)[0]
            partner[lo + i] = over[0] if len(over) else hi - lo - 1
            if np.any(np.abs(cum - thr) <= margin * total):
                ambiguous.add(c)
    return partner, sorted(zero_rows), sorted(ambiguous)


def mismatch_apply(row_ptr, pt_idx, partner):
    """the swaps of every camera in ascending i"""
    out = np.array(pt_idx, copy=True)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    for c in range(len(row_ptr) - 1):
        lo = int(row_ptr[c])
        for i in range(lo, int(row_ptr[c + 1])):
            j = int(partner[i])
            if j >= 0:
                out[i], out[lo + j] = out[lo + j], out[i]
    return out


# ---- split --------------------------------------------------------------------------------------------------------------
def split_landmarks(pts, pt_idx, split_fraction, seed):
    """(pts [n_pts + n, 3], pt_idx, n)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    pt_idx = np.asarray(pt_idx).astype(np.int64)
    n_pts = len(pts)
    n = fraction_count(split_fraction, n_pts, n_pts)
    a, _ = draws(seed, STREAM_SPLIT, np.arange(n_pts), 0)
    sel = smallest(a, n)
    copy_of = np.full(n_pts, -1, dtype=np.int64)
    copy_of[sel] = n_pts + np.arange(n)                      # the r-th selected point in ascending index
    ao, _ = draws(seed, STREAM_SPLIT, np.arange(len(pt_idx)), 1)
    move = sel[pt_idx] & ((ao & np.uint64(1)) == np.uint64(1)) if len(pt_idx) else np.zeros(0, dtype=bool)
    out = pt_idx.copy()
    out[move] = copy_of[pt_idx[move]]
    return np.concatenate([pts, pts[sel]]), out, n


# ---- nearest points and join ----------------------------------------------------------------------------------------------
def nearest_points(pts, query):
    """[n_query, 11] int32: ascending (d2, index), d2 = (dx * dx + dy * dy) + dz * dz, the point itself included; -1 padding"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.full((len(query), NEAREST), -1, dtype=np.int32)
    idx = np.arange(len(pts))
    for r, q in enumerate(np.asarray(query).astype(np.int64)):
        d = pts - pts[q]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((idx, d2))[:NEAREST]
        out[r, :len(order)] = order
    return out


def join_landmarks(pts, pt_idx, join_fraction, seed):
    """(pt_idx, n); raises ValueError("No neighbors?!") for n > 0 with fewer than two points"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    pt_idx = np.asarray(pt_idx).astype(np.int64)
    n_pts, n_obs = len(pts), len(pt_idx)
    n = fraction_count(join_fraction, n_pts, n_obs)
    if n == 0:
        return pt_idx.copy(), 0
    if n_pts < 2:
        raise ValueError("No neighbors?!")
    a, b = draws(seed, STREAM_JOIN, np.arange(n_obs), 0)
    sel = np.nonzero(smallest(a, n))[0]
    avail = min(NEAREST - 1, n_pts - 1)
    nn = nearest_points(pts, pt_idx[sel])
    e = np.minimum(np.floor(uniform(b[sel]) * avail).astype(np.int64), avail - 1)
    out = pt_idx.copy()
    out[sel] = nn[np.arange(len(sel)), 1 + e]
    return out, n
