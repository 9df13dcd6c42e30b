"""tests/_indexnoiseref.py -- the numpy restatement the GPU tests of the index noise compare with -- held to the reference's
DISTRIBUTIONAL contract (src/noise.rs:179-378) on small problems: the draw scheme is this project's, what it must produce is not.
No GPU."""
import numpy as np
import pytest

import _indexnoiseref as R


def _rows(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


LENGTHS = (0, 1, 2, 7, 63, 64, 65, 130)


def test_draws_are_counter_based_and_uniform():
    a, b = R.draws(5, R.STREAM_DROP, np.arange(20000), 0)
    a2, _ = R.draws(5, R.STREAM_DROP, np.arange(100, 200), 0)
    assert np.array_equal(a[100:200], a2)                    # an entity's draw does not depend on who else is drawn
    assert not np.array_equal(a, R.draws(6, R.STREAM_DROP, np.arange(20000), 0)[0])
    assert not np.array_equal(a, R.draws(5, R.STREAM_JOIN, np.arange(20000), 0)[0])
    for u in (R.uniform(a), R.uniform(b)):
        assert 0.0 <= u.min() and u.max() < 1.0
        assert abs(u.mean() - 0.5) < 4 / np.sqrt(12 * len(u))
    assert abs(float((a & np.uint64(1)).mean()) - 0.5) < 4 * 0.5 / np.sqrt(len(a))


@pytest.mark.parametrize("f", (0.0, 0.1, 0.5, 0.999, 1.0, 1.7, -1.0))
def test_drop_keeps_floor_len_f_per_row_in_order(f):
    row_ptr = _rows(LENGTHS)
    n = int(row_ptr[-1])
    pt = np.arange(n)
    uv = np.arange(2 * n, dtype=np.float64).reshape(-1, 2)
    rows, pt2, uv2 = R.drop_features(row_ptr, pt, uv, f, seed=11)
    want = [min(L, max(0, int(np.floor(L * f)))) for L in LENGTHS]
    assert list(np.diff(rows.astype(np.int64))) == want      # l = len * drop_percent, src/noise.rs:238
    assert np.all(np.diff(pt2) > 0)                          # survivors in their order (the reference leaves them shuffled)
    assert np.array_equal(uv2[:, 0], 2.0 * pt2)              # an observation keeps its pixel


def test_drop_selects_every_entry_equally_often():
    row_ptr = _rows((10,))
    hits = sum(R.drop_keep(row_ptr, 0.3, seed).astype(int) for seed in range(2000))
    assert hits.sum() == 2000 * 3
    assert np.all(np.abs(hits - 600) < 5 * np.sqrt(2000 * 0.3 * 0.7))


def test_swap_weights_put_most_mass_on_i_itself():
    rng = np.random.default_rng(0)
    row = rng.uniform(-1, 1, (40, 2))
    for i in (0, 17, 39):
        w = R.swap_weights(row, i)
        assert w[i] == w.max() and w.min() == 0.0 and np.all(w >= 0)         # weights[i] = 0 before the shift (:203-205)
    # and near observations are likelier partners than far ones
    i = 5
    w = R.swap_weights(row, i)
    d = np.hypot(*(row - row[i]).T)
    assert np.all(np.diff(w[np.argsort(d)]) <= 0)


def test_mismatch_partner_follows_the_weights():
    row = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0], [5.0, 5.0]])
    row_ptr = _rows((4,))
    counts = np.zeros((4, 4))
    swaps = 0
    for seed in range(4000):
        partner, zero, _ = R.mismatch_partner(row_ptr, row, 0.5, seed)
        assert not zero
        for i in np.nonzero(partner >= 0)[0]:
            counts[i, partner[i]] += 1
            swaps += 1
    assert abs(swaps - 4000 * 4 * 0.5) < 5 * np.sqrt(4000 * 4 * 0.25)
    for i in range(4):
        w = R.swap_weights(row, i)
        p = w / w.sum()
        n = counts[i].sum()
        assert np.all(np.abs(counts[i] - n * p) < 5 * np.sqrt(n * p * (1 - p)) + 1)
        assert counts[i, int(np.argmin(w))] == 0             # the farthest has weight 0
    # chance 0 swaps nothing, chance 1 every observation of a row with more than one
    assert np.all(R.mismatch_partner(_rows((1, 4)), np.vstack([row[:1], row]), 0.0, 3)[0] == -1)
    p1 = R.mismatch_partner(_rows((1, 4)), np.vstack([row[:1], row]), 1.0, 3)[0]
    assert p1[0] == -1 and np.all(p1[1:] >= 0)


def test_mismatch_counts_a_row_of_coinciding_positions_and_apply_is_sequential():
    uv = np.ones((3, 2))
    partner, zero, _ = R.mismatch_partner(_rows((3,)), uv, 1.0, 0)
    assert zero == [0] and np.all(partner == -1)
    # swaps in ascending i do not commute: 0<->1 then 1<->2
    out = R.mismatch_apply(_rows((3,)), np.array([10, 11, 12]), np.array([1, 2, -1]))
    assert list(out) == [11, 12, 10]


@pytest.mark.parametrize("f", (0.0, 0.1, 1.0, 1.5))
def test_split_copies_carry_the_same_bits(f):
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(50, 3))
    pt_idx = rng.integers(0, 50, 400)
    pts2, idx2, n = R.split_landmarks(pts, pt_idx, f, seed=9)
    assert n == min(50, int(np.floor(f * 50))) and len(pts2) == 50 + n
    assert np.array_equal(pts2[:50].view(np.uint64), pts.view(np.uint64))
    moved = idx2 != pt_idx
    assert np.all(idx2[moved] >= 50) and np.all(idx2[~moved] < 50)
    assert np.array_equal(pts2[idx2].view(np.uint64), pts[pt_idx].view(np.uint64))       # an observation still sees the same bits
    src = np.full(n, -1)
    src[idx2[moved] - 50] = pt_idx[moved]
    seen = src >= 0
    assert np.all(np.diff(src[seen]) > 0)                    # copies in ascending original index
    if n == 50:                                              # every point selected: about half of all observations move (:283-286)
        assert abs(moved.sum() - 200) < 5 * np.sqrt(400 * 0.25)


@pytest.mark.parametrize("n_pts", (2, 5, 11, 12, 200))
def test_every_joined_index_is_among_the_ten_nearest_others(n_pts):
    rng = np.random.default_rng(n_pts)
    pts = rng.normal(size=(n_pts, 3))
    pt_idx = rng.integers(0, n_pts, 30 * n_pts)
    out, n = R.join_landmarks(pts, pt_idx, 0.5, seed=4)
    assert n == n_pts // 2
    changed = np.nonzero(out != pt_idx)[0]
    assert len(changed) == n                                 # a neighbour is never the point itself (distinct positions)
    for o in changed:
        d = np.linalg.norm(pts - pts[pt_idx[o]], axis=1)
        d[pt_idx[o]] = np.inf
        assert out[o] in np.argsort(d)[:10]


def test_join_without_neighbours_and_caps():
    with pytest.raises(ValueError, match="No neighbors"):
        R.join_landmarks(np.zeros((1, 3)), np.zeros(5, dtype=int), 1.0, 0)
    assert R.join_landmarks(np.zeros((1, 3)), np.zeros(5, dtype=int), 0.5, 0)[1] == 0
    pts = np.random.default_rng(0).normal(size=(40, 3))
    assert R.join_landmarks(pts, np.arange(8), 1.0, 0)[1] == 8               # capped at the observation count


def test_nearest_orders_exact_duplicates_by_index():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float64)
    nn = R.nearest_points(pts, [2, 4])
    assert list(nn[0][:5]) == [0, 2, 1, 3, 4] and np.all(nn[0][5:] == -1)
    assert list(nn[1][:5]) == [4, 1, 3, 0, 2]
