"""tests/_subsetref.py on the CPU: subset and window against brute-force set arithmetic on small random graphs, the
completeness property that makes a window solve exact block-coordinate descent, and the sizes of the windows the GPU tests
use (tests/test_gpu_window.py asserts the same numbers of the device first)."""
import numpy as np
import pytest

import _subsetref as SR
from _problems import dome_problem


def _random_graph(seed, n_cam=13, n_pts=17):
    """rows of 0 .. 9 entries with repeats of a (camera, point) pair allowed; some points unobserved"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 10, n_cam)
    lengths[rng.integers(0, n_cam)] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    pt_idx = rng.integers(0, n_pts - 2, int(lengths.sum())).astype(np.uint64)
    return row_ptr, pt_idx, n_pts, rng


def _obs(row_ptr, pt_idx):
    """[(camera, point, position)] of every observation"""
    return [(c, int(pt_idx[o]), o) for c in range(len(row_ptr) - 1) for o in range(int(row_ptr[c]), int(row_ptr[c + 1]))]


@pytest.mark.parametrize("seed", range(6))
def test_subset_is_the_brute_force_selection(seed):
    row_ptr, pt_idx, n_pts, rng = _random_graph(seed)
    n_cam = len(row_ptr) - 1
    ci = rng.integers(0, n_cam, 9)                            # repeats and an arbitrary order
    pi = rng.integers(0, n_pts, 12)
    rows, cols, src = SR.subset_graph(row_ptr, pt_idx, n_pts, ci, pi)
    last = {int(p): k for k, p in enumerate(pi)}              # the last slot wins
    want_cols, want_src, want_rows = [], [], [0]
    for c in ci:
        for o in range(int(row_ptr[c]), int(row_ptr[c + 1])):
            if int(pt_idx[o]) in last:
                want_cols.append(last[int(pt_idx[o])])
                want_src.append(o)
        want_rows.append(len(want_cols))
    assert rows.tolist() == want_rows and cols.tolist() == want_cols and src.tolist() == want_src
    # empty lists
    rows, cols, src = SR.subset_graph(row_ptr, pt_idx, n_pts, [], pi)
    assert rows.tolist() == [0] and len(cols) == 0
    rows, cols, src = SR.subset_graph(row_ptr, pt_idx, n_pts, ci, [])
    assert rows.tolist() == [0] * (len(ci) + 1) and len(cols) == 0


@pytest.mark.parametrize("halo", (True, False))
@pytest.mark.parametrize("seed", range(6))
def test_window_is_the_brute_force_sets_and_is_complete(seed, halo):
    row_ptr, pt_idx, n_pts, rng = _random_graph(100 + seed)
    n_cam = len(row_ptr) - 1
    S = set(int(c) for c in rng.choice(n_cam, size=int(rng.integers(1, 6)), replace=False))
    obs = _obs(row_ptr, pt_idx)
    P = {p for c, p, _ in obs if c in S}
    H = {c for c, p, _ in obs if c not in S and p in P}
    shared = {p for c, p, _ in obs if c not in S and p in P}
    w = SR.window(row_ptr, pt_idx, n_pts, sorted(S), halo=halo)
    assert set(w["S"].tolist()) == S and set(w["H"].tolist()) == H and set(w["P"].tolist()) == P and set(w["shared"].tolist()) == shared
    child_cams = sorted(S | H) if halo else sorted(S)
    assert w["cam_of"].tolist() == child_cams and w["pt_of"].tolist() == sorted(P)
    assert w["cam_role"].tolist() == [0 if c in S else 1 for c in child_cams]
    assert w["pt_role"].tolist() == [1 if (not halo and p in shared) else 0 for p in sorted(P)]
    # the child observations: those of P in the child's rows, in row order, renumbered
    want = [o for c in child_cams for cc, p, o in obs if cc == c and p in P]
    assert w["obs_of"].tolist() == want
    slot = {p: k for k, p in enumerate(sorted(P))}
    assert w["pt_idx"].tolist() == [slot[int(pt_idx[o])] for o in want]
    assert w["row_ptr"].tolist() == np.concatenate([[0], np.cumsum([sum(1 for cc, p, _ in obs if cc == c and p in P) for c in child_cams])]).tolist()
    # a seed row is whole
    for k, c in enumerate(child_cams):
        if c in S:
            assert int(w["row_ptr"][k + 1] - w["row_ptr"][k]) == int(row_ptr[c + 1] - row_ptr[c])
    # completeness: every parent observation that names a free child camera or a free child point is in the child
    free_cams = S
    free_pts = P if halo else P - shared
    in_child = set(w["obs_of"].tolist())
    for c, p, o in obs:
        if c in free_cams or p in free_pts:
            assert o in in_child, (c, p, o)


def test_window_masks_are_the_parents_or_the_role():
    row_ptr, pt_idx, n_pts, rng = _random_graph(7)
    n_cam = len(row_ptr) - 1
    cm = rng.integers(0, 0x200, n_cam).astype(np.uint16)
    pm = rng.integers(0, 2, n_pts).astype(np.uint8)
    for halo in (True, False):
        w = SR.window(row_ptr, pt_idx, n_pts, [1, 4, 5], halo=halo)
        c, p = SR.window_masks(w, cm, pm)
        for k, (co, role) in enumerate(zip(w["cam_of"], w["cam_role"])):
            assert c[k] == (0x1ff if role else cm[co])
        for k, (po, role) in enumerate(zip(w["pt_of"], w["pt_role"])):
            assert p[k] == (1 if role else pm[po])
        c0, p0 = SR.window_masks(w)
        assert c0.tolist() == (w["cam_role"].astype(int) * 0x1ff).tolist() and p0.tolist() == w["pt_role"].tolist()


@pytest.fixture(scope="module")
def grid():
    import __graft_entry__ as entry
    entry.build()                                                # the oracle's library
    return SR.locality_grid()


def test_locality_grid_and_its_windows_have_the_stated_sizes(grid):
    cams, pts, row_ptr, pt_idx, uv = grid
    lengths = np.diff(row_ptr.astype(np.int64))
    assert (len(cams), len(pts), len(pt_idx)) == (400, 960, 5145)
    assert lengths.min() == 0 and lengths.max() == 20 and int((lengths == 0).sum()) == 6
    for name, (pick, want) in SR.GRID_WINDOWS.items():
        seeds = pick(len(cams))
        wh = SR.window(row_ptr, pt_idx, len(pts), seeds, halo=True)
        wn = SR.window(row_ptr, pt_idx, len(pts), seeds, halo=False)
        SR.assert_sizes(SR.window_sizes(wh, wn), want)
    # every 7th camera: every point of the window is shared; all cameras: the child is the parent
    w = SR.window(row_ptr, pt_idx, len(pts), SR.GRID_WINDOWS["every 7th"][0](400), halo=False)
    assert w["pt_role"].all()
    w = SR.window(row_ptr, pt_idx, len(pts), np.arange(400), halo=True)
    assert w["cam_of"].tolist() == list(range(400)) and w["pt_of"].tolist() == list(range(960))
    assert np.array_equal(w["row_ptr"], row_ptr) and np.array_equal(w["pt_idx"], pt_idx)


@pytest.mark.parametrize("state", (False, True))
def test_dome_windows_have_the_stated_sizes(state):
    P = dome_problem(dup=True, state=state)
    n_cam, n_pts = len(P["bal9"]), len(P["pts"])
    assert sorted(set(P["lengths"].tolist()) & {0, 1, 63, 64, 65, 127, 130, 257}) == [0, 1, 63, 64, 65, 127, 130, 257]
    assert P["lengths"][77] == 0
    for name, (pick, want) in SR.DOME_WINDOWS.items():
        seeds = pick(n_cam)
        wh = SR.window(P["row_ptr"], P["pt_idx"], n_pts, seeds, halo=True)
        wn = SR.window(P["row_ptr"], P["pt_idx"], n_pts, seeds, halo=False)
        SR.assert_sizes(SR.window_sizes(wh, wn), want)
    w = SR.window(P["row_ptr"], P["pt_idx"], n_pts, [77], halo=True)
    assert (len(w["cam_of"]), len(w["pt_of"]), len(w["pt_idx"])) == (1, 0, 0)
