"""tests/_covisref.py on the CPU: the covisibility graph against a brute-force dense incidence product B B^T, the search against a
plain breadth-first search with an explicit ranking, and the figures of the dome fixture the GPU tests lean on, pinned so that
the fixture cannot drift unnoticed."""
import numpy as np
import pytest

import _covisref as CR
from _problems import dome_problem, random_problem


def _dense(row_ptr, pt_idx, n_pts):
    """shared [n_cam, n_cam] by the incidence product: B[c, p] = 1 when row c lists p at least once; the diagonal zeroed"""
    n_cam = len(row_ptr) - 1
    B = np.zeros((n_cam, n_pts), dtype=np.int64)
    B[CR.cam_of_rows(row_ptr), np.asarray(pt_idx, dtype=np.int64)] = 1
    S = B @ B.T
    np.fill_diagonal(S, 0)
    return S


def _problems():
    P = dome_problem(seed=0)
    Q = random_problem(300, 2100, 12, seed=5)
    return (("dome", P["row_ptr"], P["pt_idx"], len(P["pts"])), ("random", Q["row_ptr"], Q["pt_idx"], len(Q["pts"])))


@pytest.mark.parametrize("min_shared", (1, 2, 5, 20))
def test_graph_is_the_dense_incidence_product(min_shared):
    for name, row_ptr, pt_idx, n_pts in _problems():
        S = _dense(row_ptr, pt_idx, n_pts)
        nbr_ptr, nbr, shared = CR.graph(row_ptr, pt_idx, min_shared)
        assert nbr_ptr.dtype == np.uint64 and nbr.dtype == np.uint32 and shared.dtype == np.uint32
        n_cam = len(row_ptr) - 1
        assert len(nbr_ptr) == n_cam + 1 and nbr_ptr[0] == 0 and nbr_ptr[-1] == len(nbr) == len(shared)
        for c in range(n_cam):
            want = np.flatnonzero(S[c] >= min_shared)
            e = slice(int(nbr_ptr[c]), int(nbr_ptr[c + 1]))
            assert np.array_equal(nbr[e], want), (name, c)
            assert np.array_equal(shared[e], S[c, want]), (name, c)


def test_dome_figures_are_pinned():
    P = dome_problem(seed=0)
    want = {1: (3160, 79, 1), 2: (1611, 72, 7), 5: (453, 62, 18), 20: (38, 29, 51)}
    for min_shared, fig in want.items():
        assert CR.figures(CR.graph(P["row_ptr"], P["pt_idx"], min_shared)[0]) == fig, min_shared
    # at min_shared = 1 the 80 non-empty cameras form the complete graph (the crowded point), the empty one is isolated
    assert 3160 == 80 * 79 // 2
    level = CR.neighbourhood(CR.graph(P["row_ptr"], P["pt_idx"], 5), [21], hops=None)
    assert np.bincount(level[level >= 0]).tolist() == [1, 1, 61]


def _bfs(S, min_shared, seeds, hops, cap, within):
    """plain breadth-first search over the dense matrix with python sets and an explicit sort of the level that does not fit"""
    n = len(S)
    level = {int(s): 0 for s in seeds}
    front, h = sorted(level), 0
    while (hops is None or h < hops) and front and not (cap and len(level) == cap):
        new = sorted({q for c in front for q in range(n) if S[c, q] >= min_shared and q not in level and (within is None or within[q])})
        if not new:
            break
        if cap and len(level) + len(new) > cap:
            score = {q: min(sum(int(S[q, t]) for t in level if S[q, t] >= min_shared), 2 ** 32 - 1) for q in new}
            for q in sorted(new, key=lambda q: (-score[q], q))[:cap - len(level)]:
                level[q] = h + 1
            break
        for q in new:
            level[q] = h + 1
        front, h = new, h + 1
    out = np.full(n, -1, dtype=np.int32)
    for q, l in level.items():
        out[q] = l
    return out


@pytest.mark.parametrize("min_shared", (1, 2, 5))
def test_neighbourhood_is_the_plain_search(min_shared):
    for name, row_ptr, pt_idx, n_pts in _problems():
        S = _dense(row_ptr, pt_idx, n_pts)
        g = CR.graph(row_ptr, pt_idx, min_shared)
        n_cam = len(S)
        rng = np.random.default_rng(min_shared)
        within = rng.random(n_cam) < 0.7
        for seeds in ([21], [3, 40, 41], list(np.flatnonzero(within)[:2])):
            for hops in (0, 1, 2, None):
                for cap in (None, len(seeds), len(seeds) + 1, 7, 30, 70):
                    for w in (None, within):
                        if w is not None and not all(w[s] for s in seeds):
                            continue
                        got = CR.neighbourhood(g, seeds, hops=hops, max_cameras=cap, within=w)
                        assert np.array_equal(got, _bfs(S, min_shared, seeds, hops, cap, w)), (name, seeds, hops, cap, w is not None)
                        if cap:
                            assert np.sum(got >= 0) <= cap


def test_the_ranking_breaks_ties_by_index():
    # camera 0 shares two points with 1, 2, 3 and 4 each; a cap of 3 takes the two lowest of them
    rows = [[0, 1, 2, 3, 4, 5, 6, 7], [0, 1], [2, 3], [4, 5], [6, 7]]
    row_ptr, pt_idx = CR._lists(rows)
    g = CR.graph(row_ptr, pt_idx, 1)
    assert np.array_equal(CR.neighbourhood(g, [0], hops=1, max_cameras=3), [0, 1, 1, -1, -1])
    # a duplicated (camera, point) entry counts once
    row_ptr, pt_idx = CR._lists([[0, 0], [0, 0]])
    assert [x.tolist() for x in CR.graph(row_ptr, pt_idx, 1)] == [[0, 1, 2], [1, 0], [1, 1]]


def test_the_fixture_lists_are_what_they_claim():
    for d in (63, 64, 65):
        row_ptr, pt_idx, n_pts = CR.hub_list(d, tight=False)
        nbr_ptr, nbr, shared = CR.graph(row_ptr, pt_idx, 1)
        assert nbr_ptr[1] == d and set(shared[:d].tolist()) == {1, 2, 3, 4, 5}
        first = [int(p) for p in pt_idx[:int(row_ptr[1])]]
        assert first != sorted(first)                        # the neighbours are not met in ascending order
    for d in (127, 128, 129):
        row_ptr, pt_idx, n_pts = CR.hub_list(d, tight=True)
        assert CR.row_bounds(row_ptr, pt_idx, n_pts)[0] == d
        nbr_ptr, nbr, shared = CR.graph(row_ptr, pt_idx, 1)
        assert nbr_ptr[1] == d and set(shared.tolist()) == {1, 2, 3, 4, 5}
    row_ptr, pt_idx, n_pts = CR.collision_list(stride=16, degree=8)
    nbr_ptr, nbr, shared = CR.graph(row_ptr, pt_idx, 1)
    assert len(row_ptr) - 1 == 129 and nbr[int(nbr_ptr[128]):].tolist() == [16 * j for j in range(8)]
    assert shared[int(nbr_ptr[128]):].tolist() == [1 + j % 3 for j in range(8)]
    row_ptr, pt_idx, n_pts = CR.heavy_only_list(9)
    assert CR.figures(CR.graph(row_ptr, pt_idx, 1)[0]) == (36, 8, 0) and CR.row_bounds(row_ptr, pt_idx, n_pts).tolist() == [8] * 9
