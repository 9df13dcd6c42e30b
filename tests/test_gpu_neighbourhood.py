"""The search over the covisibility graph on the device (BAProblem.neighbourhood / c2b_problem_neighbourhood) and
the windows grown by it (solve.solve_neighbourhood, solve.solve_windows(by="covisibility")) against tests/_covisref.py: members
and levels are integers and are held exactly, ranking and ties included; the solves are held bit for bit to the manual
composition of the calls they are made of."""
import numpy as np
import pytest

import _covisref as CR
from _problems import dome_problem

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
LM = dict(iterations=3, lam=1e-4, max_iters=50, rel_tol=1e-8)
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


def _grid_arrays(c2b):
    """the --blocks 4 grid built on the device, culled, its start moved by noise: the arrays every test loads it from"""
    if "grid" not in _cache:
        from city2ba_amd import noise as N, synthetic as SY
        ba = SY.synthetic_grid(10, 10, 4, 20.0, 1.0, 1.0, 1.0, 10.0, False, cull=True)
        N.add_noise(ba, 0.0, 0.0, 1e-2, 1e-3, seed=3)
        _cache["grid"] = (ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
        ba.close()
    return _cache["grid"]


def _load(c2b, name):
    if name == "grid":
        return c2b.BAProblem.from_bal(*_grid_arrays(c2b), device=0), 1
    if "dome" not in _cache:
        _cache["dome"] = dome_problem(dup=True)
    P = _cache["dome"]
    return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0), 5


def _cost(ba):
    return ba.total_reprojection_error(2.0) ** 2


def _check(ba, g, seeds, min_shared, **kw):
    within = kw.get("within")
    if within is not None and np.asarray(within).dtype != np.bool_:                       # an index list: the reference takes the mask
        mask = np.zeros(len(g[0]) - 1, dtype=bool)
        mask[np.asarray(within, dtype=np.int64)] = True
        within = mask
    want = CR.neighbourhood(g, seeds, hops=kw.get("hops", 1), max_cameras=kw.get("max_cameras"), within=within)
    idx, lev = ba.neighbourhood(seeds, min_shared=min_shared, return_levels=True, **kw)
    assert idx.tolist() == np.flatnonzero(want >= 0).tolist(), (seeds, kw)
    assert lev.dtype == np.int32 and lev.tolist() == want[want >= 0].tolist(), (seeds, kw)
    assert _bits(ba.neighbourhood(seeds, min_shared=min_shared, **kw), idx)               # without the levels: the same members
    return want


@pytest.mark.parametrize("name", ("dome", "grid"))
def test_members_and_levels_are_the_references(c2b, name):
    ba, ms = _load(c2b, name)
    n_cam = ba.num_cameras()
    g = CR.graph(ba.row_ptr, ba.pt_idx, ms)
    deg = np.diff(g[0].astype(np.int64))
    hub = int(np.argmax(deg))
    first = 21 if name == "dome" else 0
    rng = np.random.default_rng(7)
    within = rng.random(n_cam) < 0.6
    within[[first, hub]] = True
    for seeds in ([first], [hub], [first, hub, n_cam - 1]):
        for hops in (0, 1, 2, None):
            want = _check(ba, g, seeds, ms, hops=hops)
            if hops == 0:
                assert np.flatnonzero(want >= 0).tolist() == sorted(seeds)
            _check(ba, g, seeds[:2], ms, hops=hops, within=within)
            _check(ba, g, seeds[:2], ms, hops=hops, within=np.flatnonzero(within))         # an index list for the mask
    if name == "dome":
        level = CR.neighbourhood(g, [21], hops=None)
        assert np.bincount(level[level >= 0]).tolist() == [1, 1, 61]
    # a cap inside level 1, inside level 2, equal to the seed count, one more than it, and beyond everything reachable
    full = CR.neighbourhood(g, [first], hops=None)
    sizes = np.bincount(full[full >= 0])
    assert len(sizes) >= 3 and deg[hub] >= 8
    for seeds, cap in (([hub], 1 + deg[hub] // 2), ([hub], 2), ([first], sizes[0] + sizes[1] + max(1, sizes[2] // 3)), ([first], 1),
                       ([first, hub], 2), ([first], n_cam + 5)):
        for hops in (None, 1, 3):
            want = _check(ba, g, seeds, ms, hops=hops, max_cameras=int(cap))
            assert np.sum(want >= 0) <= cap
        _check(ba, g, seeds, ms, hops=None, max_cameras=int(cap), within=within)
    # the ranking met ties somewhere: equal scores cut by index
    lvl = _check(ba, g, [hub], ms, hops=1, max_cameras=int(1 + deg[hub] // 2))
    e = slice(int(g[0][hub]), int(g[0][hub + 1]))
    taken = lvl[g[1][e].astype(np.int64)] >= 0
    assert taken.any() and not taken.all()
    assert g[2][e][taken].min() >= g[2][e][~taken].max()     # with a single seed the score is the shared count with it
    ba.close()


def test_refusals(c2b):
    import ctypes as C
    from city2ba_amd import _lib as L
    lib = L.lib()
    ba, ms = _load(c2b, "dome")
    n_cam = ba.num_cameras()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    seed = np.zeros(n_cam, np.uint8)
    seed[[3, 4, 5]] = 1
    within = np.ones(n_cam, np.uint8)
    within[4] = 0
    member, level, n = np.full(n_cam, 9, np.uint8), np.full(n_cam, 9, np.int32), C.c_int64(-7)
    for args, word in (((ba._h, p(np.zeros(n_cam, np.uint8)), 1, ms, 0, None), b"no seed"),
                       ((ba._h, p(seed), 1, ms, 2, None), b"max_cameras"),
                       ((ba._h, p(seed), 1, ms, 0, p(within)), b"within"),
                       ((ba._h, p(seed), 1, 0, 0, None), b"min_shared"),
                       ((ba._h, None, 1, ms, 0, None), b"NULL")):
        assert lib.c2b_problem_neighbourhood(*args, p(member), p(level), C.byref(n)) == L.ERR_INVALID_ARGUMENT, word
        assert word in lib.c2b_last_error(), lib.c2b_last_error()
    shard, _ = _load(c2b, "dome")
    L.check(lib.c2b_problem_set_shard(shard._h, 0, 2 * n_cam, 0))
    assert lib.c2b_problem_neighbourhood(shard._h, p(seed), 1, ms, 0, None, p(member), p(level), C.byref(n)) == L.ERR_INVALID_ARGUMENT
    assert b"shard" in lib.c2b_last_error()
    assert (member == 9).all() and (level == 9).all() and n.value == -7               # nothing written
    with pytest.raises(L.City2baError):
        ba.neighbourhood([])
    with pytest.raises(L.City2baError):
        ba.neighbourhood([n_cam])
    with pytest.raises(L.City2baError):
        ba.neighbourhood([3, 4, 5], max_cameras=2)
    with pytest.raises(ValueError):
        ba.neighbourhood(np.zeros(n_cam + 1, bool))
    assert ba.neighbourhood([3, 4, 5], hops=0, max_cameras=3).tolist() == [3, 4, 5]      # a cap equal to the seed count
    for x in (ba, shard):
        x.close()


@pytest.mark.parametrize("name", ("dome", "grid"))
def test_solve_neighbourhood_is_solve_window_on_the_neighbourhood(c2b, name):
    from city2ba_amd import solve as S
    ba, ms = _load(c2b, name)
    twin, _ = _load(c2b, name)
    seeds = [21] if name == "dome" else [150]
    kw = dict(hops=2, min_shared=ms, max_cameras=40)
    got = S.solve_neighbourhood(ba, seeds, halo=True, **kw, **LM)
    idx, lev = twin.neighbourhood(seeds, return_levels=True, **kw)
    want = S.solve_window(twin, idx, halo=True, **LM)
    assert 1 < len(idx) <= 40 and _bits(got["seeds"], idx) and _bits(got["levels"], lev)
    assert got["final_cost"] < got["initial_cost"]
    for k in want:
        assert repr(got[k]) == repr(want[k]), k              # the summary, iteration by iteration (repr: a NaN equals itself)
    assert set(got) == set(want) | {"seeds", "levels"}
    assert _bits(ba.cameras_bal(), twin.cameras_bal()) and _bits(ba.points(), twin.points())
    for x in (ba, twin):
        x.close()


@pytest.mark.parametrize("name", ("dome", "grid"))
def test_covisibility_windows_partition_the_cameras_and_never_raise_the_cost(c2b, name):
    from city2ba_amd import solve as S
    ba, ms = _load(c2b, name)
    twin, _ = _load(c2b, name)
    n_cam, _, n_obs = ba._sizes()
    size = 24 if name == "dome" else 64
    F0 = F = _cost(ba)
    mine = []
    for sweep in range(2):                                    # solve_windows' loop, with the parent's cost read between windows
        todo = np.ones(n_cam, bool)
        while todo.any():
            first = int(np.flatnonzero(todo)[0])
            idx, lev = ba.neighbourhood([first], hops=None, min_shared=ms, max_cameras=size, within=todo, return_levels=True)
            assert todo[idx].all() and first in idx and len(idx) <= size
            s = S.solve_window(ba, idx, halo=True, **LM)
            Fn = _cost(ba)
            bound = U53 * ((2 * n_obs + 4) * (F + Fn) + (2 * s["observations"] + 4) * (s["initial_cost"] + s["final_cost"]))
            assert s["final_cost"] <= s["initial_cost"] and Fn <= F + bound, (sweep, first, F, Fn, bound)
            F = Fn
            todo[idx] = False
            s.update(seed=first, seeds=idx, levels=lev, sweep=sweep)
            mine.append(s)
    assert F < F0
    theirs = S.solve_windows(twin, size, sweeps=2, halo=True, by="covisibility", min_shared=ms, **LM)
    assert len(theirs) == len(mine)
    for a, b in zip(mine, theirs):
        assert a["seed"] == b["seed"] and a["sweep"] == b["sweep"] and _bits(a["seeds"], b["seeds"]) and _bits(a["levels"], b["levels"])
        assert a["final_cost"] == b["final_cost"] and a["cameras"] == b["cameras"] and repr(a["history"]) == repr(b["history"])
    assert _bits(ba.cameras_bal(), twin.cameras_bal()) and _bits(ba.points(), twin.points())       # two runs, the same bits
    for sweep in range(2):                                    # a sweep's windows partition the cameras
        sets = [s["seeds"] for s in theirs if s["sweep"] == sweep]
        allc = np.concatenate(sets)
        assert len(allc) == n_cam and len(np.unique(allc)) == n_cam
    print("COVIS sweeps %s: cost %.17g -> %.17g over %d windows of up to %d cameras" % (name, F0, F, len(mine), size))
    with pytest.raises(ValueError):
        S.solve_windows(twin, size, stride=8, by="covisibility")
    with pytest.raises(ValueError):
        S.solve_windows(twin, size, by="distance")
    for x in (ba, twin):
        x.close()


def test_index_windows_are_unchanged(c2b):
    """by="index" is the default and is the loop it was: the manual solve_window loop over consecutive indices, bit for bit"""
    from city2ba_amd import solve as S
    a, _ = _load(c2b, "grid")
    b, _ = _load(c2b, "grid")
    m, _ = _load(c2b, "grid")
    n_cam = a.num_cameras()
    one = S.solve_windows(a, 64, stride=48, sweeps=1, halo=True, **LM)
    two = S.solve_windows(b, 64, stride=48, sweeps=1, halo=True, by="index", **LM)
    manual = []
    for lo in range(0, n_cam, 48):
        hi = min(lo + 64, n_cam)
        s = S.solve_window(m, range(lo, hi), halo=True, **LM)
        s.update(lo=lo, hi=hi, sweep=0)
        manual.append(s)
        if hi == n_cam:
            break
    assert repr(one) == repr(two) == repr(manual) and len(one) >= 2
    assert _bits(a.cameras_bal(), b.cameras_bal()) and _bits(a.cameras_bal(), m.cameras_bal()) and _bits(a.points(), m.points())
    for x in (a, b, m):
        x.close()
