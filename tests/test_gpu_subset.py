"""BAProblem.subset on the device (c2b_problem_subset) against tests/_subsetref.py, bit for bit: cameras, points,
row pointer, indices, uv.  The dome's rows of 63 / 64 / 65 / 127 / 130 / 257 entries put the stable fill across its chunks
of 64, its duplicated pairs and the crowded point 0 are kept as the reference keeps them; random_problem(300, 2100, ...)
crosses a scan tile of 1 024 points and a workgroup of 256 cameras; a camera list of 1 500 entries takes the tiled row scan."""
import numpy as np
import pytest

import _subsetref as SR
from _problems import dome_problem, random_problem

pytestmark = pytest.mark.gpu
MODES = ["bal", "state"]
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


def _arrays(ba):
    return ba.cameras(), ba.points(), ba.row_ptr, ba.pt_idx, ba.observations()


def _check(ba, ci, pi, carry=False):
    """the child of (ci, pi) against the reference over the parent's own arrays; returns the child's arrays"""
    want = SR.subset(*_arrays(ba), ci, pi)
    child = ba.subset(ci, pi, carry=carry)
    got = _arrays(child)
    assert child._sizes() == (len(want[0]), len(want[1]), len(want[3]))
    for name, g, w in zip(("cameras", "points", "row_ptr", "pt_idx", "uv"), got, want):
        assert _bits(g, w.reshape(g.shape)), name
    # the child is in the parent's camera mode and holds its bits there too
    assert _bits(child.cameras_bal(), ba.cameras_bal()[np.asarray(ci, dtype=np.int64)])
    child.close()
    return got


@pytest.mark.parametrize("mode", MODES)
def test_dome_selections_are_the_references_bit_for_bit(c2b, mode):
    P = _dome(mode)
    ba = _load(c2b, P)
    n_cam, n_pts = len(P["bal9"]), len(P["pts"])
    lengths = np.diff(P["row_ptr"].astype(np.int64))
    assert {0, 1, 63, 64, 65, 127, 130, 257} <= set(lengths.tolist())
    ci = np.concatenate([np.arange(n_cam)[::-1], [3]])        # reversed, camera 3 twice, the empty row included
    assert lengths[ci].min() == 0
    full = _check(ba, ci, np.arange(n_pts))
    assert len(full[3]) == int(lengths[ci].sum())             # every point selected: nothing disappears, duplicated pairs stay
    half = _check(ba, ci, np.arange(0, n_pts, 2))             # compaction across the chunk edges of the long rows
    assert 0 < len(half[3]) < len(full[3])
    # point 0 twice: the last slot wins, and the same bits come out of a second run
    pi = np.concatenate([[0], np.arange(5, 40), [0], np.arange(40, 50)])
    a = _check(ba, ci, pi)
    b = _check(ba, ci, pi)
    assert all(_bits(x, y) for x, y in zip(a, b))
    assert (a[3] == 36).any() and not (a[3] == 0).any()       # the crowded point's observations name slot 36, never slot 0
    # a camera list long enough for the tiled row scan
    _check(ba, np.arange(1500) % n_cam, np.arange(1, n_pts, 3))
    ba.close()


def test_random_problem_crosses_a_scan_tile_and_a_workgroup(c2b):
    P = random_problem(300, 2100, 12, seed=5, empty_every=7)
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    got = _check(ba, np.arange(299), np.arange(0, 2100, 3))
    assert len(got[0]) == 299 and len(got[1]) == 700 and len(got[3]) > 0
    ba.close()


@pytest.mark.parametrize("mode", MODES)
def test_empty_lists_and_a_selection_without_observations(c2b, mode):
    P = _dome(mode)
    ba = _load(c2b, P)
    n_cam, n_pts = len(P["bal9"]), len(P["pts"])
    for ci, pi in (([], np.arange(n_pts)), (np.arange(n_cam), []), ([], [])):
        got = _check(ba, ci, pi)
        assert len(got[3]) == 0 and got[2].tolist() == [0] * (len(ci) + 1)
    unobserved = np.setdiff1d(np.arange(n_pts), P["pt_idx"].astype(np.int64))
    assert len(unobserved) == 20
    got = _check(ba, np.arange(n_cam), unobserved)            # cameras and points, no observation kept
    assert len(got[0]) == n_cam and len(got[1]) == 20 and len(got[3]) == 0
    ba.close()


def test_refusals_leave_dst_as_it_was(c2b):
    import ctypes as C
    from city2ba_amd import _lib as L
    P, Q = _dome("bal"), random_problem(20, 60, 5, seed=3)
    ba = _load(c2b, P)
    other = c2b.BAProblem.from_bal(Q["bal9"], Q["pts"], Q["row_ptr"], Q["pt_idx"], Q["uv"], device=0)
    other.set_constant(points=np.arange(60) % 2 == 0)
    before = _arrays(other) + (other.cameras_bal(),) + other.constant()
    n_cam, n_pts = len(P["bal9"]), len(P["pts"])
    ok = np.array([0, 1], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = L.lib()
    for args, code in (((ba._h, p(np.array([0, n_cam], np.uint32)), 2, p(ok), 2, 0, other._h), L.ERR_INDEX_OUT_OF_RANGE),
                       ((ba._h, p(ok), 2, p(np.array([n_pts, 0], np.uint32)), 2, 0, other._h), L.ERR_INDEX_OUT_OF_RANGE),
                       ((other._h, p(ok), 2, p(ok), 2, 0, other._h), L.ERR_INVALID_ARGUMENT),            # dst == src
                       ((ba._h, None, 2, p(ok), 2, 0, other._h), L.ERR_INVALID_ARGUMENT),                 # a NULL list, a count
                       ((ba._h, p(ok), 2, None, 2, 0, other._h), L.ERR_INVALID_ARGUMENT),
                       ((ba._h, p(ok), 2, p(ok), 2, 2, other._h), L.ERR_INVALID_ARGUMENT)):               # an unknown flag
        assert lib.c2b_problem_subset(*args) == code, lib.c2b_last_error()
    # a shard is refused
    shard = _load(c2b, P)
    L.check(lib.c2b_problem_set_shard(shard._h, 0, 2 * n_cam, 0))
    assert lib.c2b_problem_subset(shard._h, p(ok), 2, p(ok), 2, 0, other._h) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_problem_window(shard._h, p(np.ones(n_cam, np.uint8)), 1, other._h) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_problem_window(ba._h, p(np.zeros(n_cam, np.uint8)), 1, other._h) == L.ERR_INVALID_ARGUMENT      # no seed
    after = _arrays(other) + (other.cameras_bal(),) + other.constant()
    assert all(_bits(x, y) for x, y in zip(before, after))
    with pytest.raises(L.City2baError) as err:
        ba.subset([0, n_cam], [0])
    assert err.value.status == L.ERR_INDEX_OUT_OF_RANGE
    with pytest.raises(L.City2baError):
        ba.subset([0], [-1])
    for x in (ba, other, shard):
        x.close()


def _with_state(c2b, P):
    """the dome with every kind of handle state set"""
    ba = _load(c2b, P)
    n_cam, n_pts = ba.num_cameras(), ba.num_points()
    rng = np.random.default_rng(2)
    ba.set_constant(cameras=rng.integers(0, 0x200, n_cam).astype(np.uint16), points=rng.integers(0, 2, n_pts).astype(bool))
    ba.set_priors(camera_centers=rng.normal(size=(n_cam, 3)), camera_center_weights=rng.uniform(0.1, 1.0, (n_cam, 3)),
                  points=rng.normal(size=(n_pts, 3)), point_weights=rng.uniform(0.1, 1.0, (n_pts, 3)))       # no intrinsics prior
    ba.set_loss("huber", 0.25)
    ba.set_preconditioner("schur_jacobi")
    ba.set_inner_iterations(2)
    ba.set_options(rank_sort_max_row=7)
    return ba


@pytest.mark.parametrize("mode", MODES)
def test_carry_takes_the_handle_state_gathered_and_records_an_origin_for_repeat_free_lists(c2b, mode):
    ba = _with_state(c2b, _dome(mode))
    n_cam, n_pts = ba.num_cameras(), ba.num_points()
    ci, pi = np.arange(n_cam)[::-3], np.arange(2, n_pts, 2)
    child = ba.subset(ci, pi, carry=True)
    cm, pm = ba.constant()
    assert _bits(child.constant()[0], cm[ci]) and _bits(child.constant()[1], pm[pi])
    pp, pc = ba.priors, child.priors
    for k in ("camera_centers", "camera_center_weights", "intrinsics", "intrinsics_weights"):
        assert _bits(pc[k], pp[k][ci]), k
    for k in ("points", "point_weights"):
        assert _bits(pc[k], pp[k][pi]), k
    assert pc["active"] == (len(ci), 0, len(pi)) and not pc["intrinsics_weights"].any()       # a kind the parent lacks is not held
    assert child.loss == ("huber", 0.25) and child.preconditioner == "schur_jacobi" and child.inner_iterations() == 2
    assert child.options() == ba.options() and child.options()["rank_sort_max_row"] == 7
    o = child.origin()
    assert o["cam_of"].tolist() == ci.tolist() and o["pt_of"].tolist() == pi.tolist() and not o["cam_role"].any() and not o["pt_role"].any()
    child.close()
    for rep_c, rep_p in ((np.array([1, 2, 1]), pi), (ci, np.array([4, 4]))):          # a repeat in either list: no origin
        child = ba.subset(rep_c, rep_p, carry=True)
        assert child.origin() is None and child.loss == ("huber", 0.25)
        assert _bits(child.constant()[0], cm[rep_c]) and _bits(child.constant()[1], pm[rep_p])
        child.close()
    # without carry none of it is carried
    child = ba.subset(ci, pi)
    assert not child.constant()[0].any() and not child.constant()[1].any() and child.priors["active"] == (0, 0, 0)
    assert child.loss == (None, 1.0) and child.preconditioner == "block_jacobi" and child.inner_iterations() == 0
    assert child.options()["rank_sort_max_row"] == 0 and child.origin() is None
    child.close()
    ba.close()


def test_fifty_extractions_leave_the_free_memory_where_it_was(c2b):
    """in the manner of tests/test_gpu_leak.py: one warm-up pair, then 50 extract / close pairs of each kind; the bound is that
    test's (twice the parent's drop on its path, 0 bytes)"""
    import torch
    ba = _with_state(c2b, _dome("bal"))
    n_cam, n_pts = ba.num_cameras(), ba.num_points()

    def pair():
        ba.subset(np.arange(n_cam)[::-1], np.arange(0, n_pts, 2), carry=True).close()
        ba.window(np.arange(10), halo=True).close()
    pair()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        pair()
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info(0)[0]
    print("free device memory dropped by %d bytes over 50 subset / window pairs" % drop)
    assert drop <= 0
    ba.close()
