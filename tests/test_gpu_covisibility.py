"""The camera covisibility graph on the device (BAProblem.covisibility / c2b_covisibility_*_rows) against
tests/_covisref.py.  Integers only: every comparison is exact equality.  The dome has rows of 0, 1, 63, 64, 65, 127, 130 and 257
entries, duplicated (camera, point) pairs, the crowded point and unobserved points; the hub lists put one camera's degree at a
wave's chunk (63, 64, 65), at the table's size S = COVIS_WAVE_SLOTS (S - 1, S, S + 1: its bound crosses the table there) and
far beyond it (3 S); the collision list's neighbours agree in their low 16 bits; the heavy-only list sends every camera down
the heavy path.  The Level-0 cases need index arrays only, no geometry."""
import numpy as np
import pytest

import _covisref as CR
from _problems import dome_problem

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def c2b():
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd
    assert city2ba_amd.device_count() > 0
    return city2ba_amd


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dome(mode):
    if mode not in _cache:
        _cache[mode] = dome_problem(dup=True, state=mode == "state")
    return _cache[mode]


def _load(c2b, P):
    if P.get("bal", True):
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    return c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


def _properties(g, n_cam):
    """symmetry, ascending rows, no self edge, a consistent row pointer"""
    nbr_ptr, nbr, shared = g
    assert nbr_ptr.dtype == np.uint64 and nbr.dtype == np.uint32 and shared.dtype == np.uint32
    assert len(nbr_ptr) == n_cam + 1 and nbr_ptr[0] == 0 and int(nbr_ptr[-1]) == len(nbr) == len(shared)
    ptr = nbr_ptr.astype(np.int64)
    assert (np.diff(ptr) >= 0).all()
    row = np.repeat(np.arange(n_cam, dtype=np.int64), np.diff(ptr))
    col = nbr.astype(np.int64)
    assert (row != col).all() and (col < n_cam).all() and (shared >= 1).all()
    inner = np.ones(len(col), dtype=bool)
    inner[ptr[:-1][np.diff(ptr) > 0]] = False                 # the first entry of every non-empty row
    assert (np.diff(col)[inner[1:]] > 0).all()                # strictly ascending inside a row
    fwd = np.argsort(row * n_cam + col, kind="stable")
    back = np.argsort(col * n_cam + row, kind="stable")
    assert np.array_equal(row[fwd], col[back]) and np.array_equal(col[fwd], row[back]) and np.array_equal(shared[fwd], shared[back])


def _level0(row_ptr, pt_idx, n_pts, min_shared=1):
    """(graph as numpy arrays, (n_edges, n_heavy)) through device.covisibility_rows, twice: the same bytes"""
    import torch
    from city2ba_amd import device as D
    dev = torch.device("cuda:0")
    rp = torch.from_numpy(np.ascontiguousarray(row_ptr).astype(np.int64)).to(dev)
    pi = torch.from_numpy(np.ascontiguousarray(pt_idx).astype(np.uint32).view(np.int32)).to(dev)
    import types
    rows = types.SimpleNamespace(row_ptr=rp, n_cam=len(row_ptr) - 1, n_obs=len(pt_idx))      # (no tile records: the passes take the row pointer alone)
    prows = D.PointRows(rows, pi, n_pts)
    out = []
    for _ in range(2):
        nbr_ptr, nbr, shared, counts = D.covisibility_rows(rows, pi, prows, min_shared, return_counts=True)
        out.append((nbr_ptr.cpu().numpy().view(np.uint64), nbr.cpu().numpy().view(np.uint32), shared.cpu().numpy().view(np.uint32),
                    tuple(int(v) for v in counts.cpu().numpy())))
    assert all(_bits(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]
    return out[0][:3], out[0][3]


def _check_level0(row_ptr, pt_idx, n_pts, min_shared=1):
    want = CR.graph(row_ptr, pt_idx, min_shared)
    got, (n_edges, n_heavy) = _level0(row_ptr, pt_idx, n_pts, min_shared)
    for name, g, w in zip(("nbr_ptr", "nbr", "shared"), got, want):
        assert _bits(g, w), name
    assert n_edges == len(want[1])
    _properties(got, len(row_ptr) - 1)
    slots = _slots()
    assert n_heavy == int(np.sum(CR.row_bounds(row_ptr, pt_idx, n_pts) > slots))
    return got, n_heavy


def _slots():
    from city2ba_amd import device as D
    return D.COVIS_WAVE_SLOTS


@pytest.mark.parametrize("min_shared", (1, 2, 5, 20))
@pytest.mark.parametrize("mode", ("bal", "state"))
def test_dome_graph_is_the_references(c2b, mode, min_shared):
    P = _dome(mode)
    assert {0, 1, 63, 64, 65, 127, 130, 257} <= set(np.diff(P["row_ptr"].astype(np.int64)).tolist())
    ba = _load(c2b, P)
    want = CR.graph(P["row_ptr"], P["pt_idx"], min_shared)
    got = ba.covisibility(min_shared)
    again = ba.covisibility(min_shared)                      # the cached graph: the same bytes
    for name, g, w, a in zip(("nbr_ptr", "nbr", "shared"), got, want, again):
        assert _bits(g, w) and _bits(a, w), name
    _properties(got, ba.num_cameras())
    assert CR.figures(got[0]) == {1: (3160, 79, 1), 2: (1611, 72, 7), 5: (453, 62, 18), 20: (38, 29, 51)}[min_shared]
    assert ba.covisibility_heavy_cameras() == 0
    ba.close()
    _check_level0(P["row_ptr"], P["pt_idx"], len(P["pts"]), min_shared)


def test_empty_and_tiny_lists(c2b):
    e64 = np.zeros(0, dtype=np.uint64)
    got, _ = _check_level0(np.zeros(1, dtype=np.uint64), e64, 0)              # no camera
    assert got[0].tolist() == [0]
    got, _ = _check_level0(np.zeros(6, dtype=np.uint64), e64, 7)              # cameras and points, no observation
    assert got[0].tolist() == [0] * 6 and len(got[1]) == 0
    got, _ = _check_level0(np.array([0, 3], dtype=np.uint64), np.array([2, 0, 2], dtype=np.uint64), 3)       # one camera
    assert got[0].tolist() == [0, 0]
    # two cameras sharing one point listed twice in both rows: shared is 1
    got, _ = _check_level0(np.array([0, 2, 4], dtype=np.uint64), np.array([0, 0, 0, 0], dtype=np.uint64), 1)
    assert [x.tolist() for x in got] == [[0, 1, 2], [1, 0], [1, 1]]
    # ... and nothing at min_shared = 2
    got, _ = _check_level0(np.array([0, 2, 4], dtype=np.uint64), np.array([0, 0, 0, 0], dtype=np.uint64), 1, min_shared=2)
    assert got[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("which", ("63", "64", "65", "S-1", "S", "S+1", "3S"))
def test_hub_lists_cross_a_chunk_and_the_table(c2b, which):
    S = _slots()
    degree = {"63": 63, "64": 64, "65": 65, "S-1": S - 1, "S": S, "S+1": S + 1, "3S": 3 * S}[which]
    tight = which in ("S-1", "S", "S+1")
    row_ptr, pt_idx, n_pts = CR.hub_list(degree, tight=tight)
    bound = CR.row_bounds(row_ptr, pt_idx, n_pts)
    if tight:
        assert bound[0] == degree                            # the hub's bound crosses the table exactly at S
    got, n_heavy = _check_level0(row_ptr, pt_idx, n_pts)
    assert int(got[0][1]) == degree and _bits(got[1][:degree], np.arange(1, degree + 1, dtype=np.uint32))
    assert set(got[2].tolist()) == {1, 2, 3, 4, 5}
    assert (n_heavy > 0) == bool((bound > S).any()) and (bound[0] > S) == (which in ("S+1", "3S"))
    for min_shared in (3, 5):
        _check_level0(row_ptr, pt_idx, n_pts, min_shared)


def test_collision_list_of_indices_that_agree_in_their_low_bits(c2b):
    row_ptr, pt_idx, n_pts = CR.collision_list()
    n_cam = len(row_ptr) - 1
    assert n_cam == 64 * 2 ** 16 + 1
    got, n_heavy = _check_level0(row_ptr, pt_idx, n_pts)
    assert n_heavy == 0 and got[1][-64:].tolist() == [j << 16 for j in range(64)] and got[2][-64:].tolist() == [1 + j % 3 for j in range(64)]
    _check_level0(row_ptr, pt_idx, n_pts, min_shared=2)


def test_heavy_only_list(c2b):
    S = _slots()
    n = 2 * S
    row_ptr, pt_idx, n_pts = CR.heavy_only_list(n)
    want = CR.graph(row_ptr, pt_idx, 1)
    got, counts = _level0(row_ptr, pt_idx, n_pts)            # (twice: the same bytes)
    for name, g, w in zip(("nbr_ptr", "nbr", "shared"), got, want):
        assert _bits(g, w), name
    assert counts == (n * (n - 1), n)                        # every camera took the heavy path
    # the complete graph in closed form: row c is every camera but c, every shared 1 (symmetric, ascending, no self edge)
    assert _bits(got[0], np.arange(n + 1, dtype=np.uint64) * np.uint64(n - 1))
    every = np.tile(np.arange(n, dtype=np.uint32), (n, 1))
    assert _bits(got[1], every[~np.eye(n, dtype=bool)]) and (got[2] == 1).all()


def test_grid_built_on_the_device(c2b):
    from city2ba_amd import synthetic as SY
    ba = SY.synthetic_grid(10, 10, 4, 20.0, 1.0, 1.0, 1.0, 10.0, False, cull=True)
    n_cam = ba.num_cameras()
    for min_shared in (1, 3):
        want = CR.graph(ba.row_ptr, ba.pt_idx, min_shared)   # the reference fed from the downloaded list
        got = ba.covisibility(min_shared)
        for name, g, w in zip(("nbr_ptr", "nbr", "shared"), got, want):
            assert _bits(g, w), name
        _properties(got, n_cam)
    assert len(got[1]) > 0
    ba.close()


def test_the_graph_goes_with_the_list_and_stays_with_the_entities(c2b):
    import ctypes as C
    from city2ba_amd import _lib as L, noise as N
    lib = L.lib()
    P = _dome("bal")

    def held(ba):
        ms = C.c_int(-1)
        return ms.value if lib.c2b_problem_get_covisibility(ba._h, None, None, None, C.byref(ms), None) == 0 else None

    ba = _load(c2b, P)
    assert held(ba) is None
    ba.covisibility(2)
    assert held(ba) == 2
    ba.covisibility(5)                                       # another threshold rebuilds
    assert held(ba) == 5
    # kept: the entities move, the list does not
    ba.apply_step(None, None)
    assert held(ba) == 5
    N.add_noise(ba, 1e-4, 1e-4, 1e-4, 1e-4, seed=1)
    assert held(ba) == 5
    ba.refine_points(rounds=1)
    ba.refine_cameras(rounds=1)
    assert held(ba) == 5
    assert ba.merge_points(1e-9, 1e-9)["merged"] == 0 and held(ba) == 5          # a merge that merges nothing
    assert ba.filter_observations(np.inf) == 0 and held(ba) == 5                 # a filter that removes nothing
    g5 = ba.covisibility(5)
    # dropped: the list changes
    assert ba.filter_observations(2e-3) > 0 and held(ba) is None
    want = CR.graph(ba.row_ptr, ba.pt_idx, 5)
    got = ba.covisibility(5)
    assert all(_bits(g, w) for g, w in zip(got, want)) and len(got[1]) < len(g5[1])
    ba.drop_features(0.9, seed=3)
    assert held(ba) is None
    assert all(_bits(g, w) for g, w in zip(ba.covisibility(1), CR.graph(ba.row_ptr, ba.pt_idx, 1)))
    ba.cull()
    assert held(ba) is None
    assert all(_bits(g, w) for g, w in zip(ba.covisibility(1), CR.graph(ba.row_ptr, ba.pt_idx, 1)))
    ba.close()
    # a merge that merges: the dome's points split, then merged back
    ba = _load(c2b, dict(P, bal9=P["true_bal9"], pts=P["true_pts"]))
    ba.split_landmarks(0.2, seed=5)
    ba.covisibility(1)
    assert held(ba) == 1
    assert ba.merge_points(1e-6, 1.0)["merged"] > 0 and held(ba) is None
    assert all(_bits(g, w) for g, w in zip(ba.covisibility(1), CR.graph(ba.row_ptr, ba.pt_idx, 1)))
    # a shard is refused
    shard = _load(c2b, P)
    L.check(lib.c2b_problem_set_shard(shard._h, 0, 2 * shard.num_cameras(), 0))
    n = C.c_int64(-7)
    assert lib.c2b_problem_covisibility(shard._h, 1, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"shard" in lib.c2b_last_error() and n.value == -7
    assert lib.c2b_problem_covisibility(ba._h, 0, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"min_shared" in lib.c2b_last_error() and n.value == -7
    for x in (ba, shard):
        x.close()


def test_fifty_builds_leave_the_free_memory_where_it_was(c2b):
    """in the manner of tests/test_gpu_subset.py: a warm-up pair, then 50 build / drop pairs (another threshold drops the graph
    the handle holds and builds the next)"""
    import torch
    ba = _load(c2b, _dome("bal"))

    def pair():
        ba.covisibility(1)
        ba.covisibility(2)
    pair()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        pair()
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info(0)[0]
    print("free device memory dropped by %d bytes over 50 covisibility build / drop pairs" % drop)
    assert drop <= 0
    ba.close()
