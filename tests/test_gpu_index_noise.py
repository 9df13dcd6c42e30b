"""The index noise on the device (csrc/index_noise_kernels.hpp) against its numpy restatement
(tests/_indexnoiseref.py), index for index: the Level-0 row passes on torch tensors and the BAProblem methods in place.
Sizes follow what the kernels branch on: rows below, at and above a wave (64) and two (128), one row of 3 000, list and
camera counts around kScanBlock = 256 and kScanTile = 1024 of scan_kernels.hpp."""
import hashlib

import numpy as np
import pytest

import _indexnoiseref as R
import oracle as O

pytestmark = pytest.mark.gpu

CHUNK, TILE = 256, 1024                                      # kScanBlock, kScanTile
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 129, 3000)


@pytest.fixture(scope="module")
def c2b():
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd
    assert city2ba_amd.device_count() > 0
    return city2ba_amd


_CASES = {}


def _case(lengths, n_pts=300, seed=0):
    """cameras looking down -z from the origin, random points, rows of the given lengths naming random points, random pixels:
    the passes read the indices and the pixels, never a projection"""
    key = (tuple(lengths), n_pts, seed)
    if key not in _CASES:
        rng = np.random.default_rng(1234 + seed)
        bal9 = np.zeros((len(lengths), 9))
        bal9[:, 6] = 1.0
        row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        n = int(row_ptr[-1])
        _CASES[key] = dict(cams=O.camera_from_bal(bal9), pts=rng.normal(size=(n_pts, 3)), row_ptr=row_ptr,
                           pt_idx=rng.integers(0, n_pts, n).astype(np.uint64), uv=rng.uniform(-1, 1, (n, 2)))
    return _CASES[key]


def _problem(c2b, P):
    return c2b.BAProblem.from_visibility(P["cams"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


# ---- drop -----------------------------------------------------------------------------------------------------------------
def _check_drop(c2b, P, f, seed):
    want_rows, want_pt, want_uv = R.drop_features(P["row_ptr"], P["pt_idx"], P["uv"], f, seed)
    ba = _problem(c2b, P)
    mask = np.arange(len(P["pts"])) % 3 == 0
    ba.set_constant(points=mask)
    ba.set_loss("huber", 0.5)
    removed = ba.drop_features(f, seed=seed)
    assert removed == len(P["pt_idx"]) - len(want_pt)
    assert np.array_equal(ba.row_ptr, want_rows)
    assert np.array_equal(ba.pt_idx, want_pt.astype(np.uint64))              # the kept set and its order
    assert np.array_equal(_bits(ba.observations().reshape(-1, 2)), _bits(want_uv))
    assert np.array_equal(ba.constant()[1], mask) and ba.loss == ("huber", 0.5)
    assert ba.num_points() == len(P["pts"]) and np.array_equal(_bits(ba.points()), _bits(P["pts"]))
    ba.close()


@pytest.mark.parametrize("f", (0.0, 0.1, 0.5, 0.999, 1.0, 1.7, -1.0))
def test_drop_rows_of_every_length(c2b, f):
    _check_drop(c2b, _case(LENGTHS), f, seed=21)


@pytest.mark.parametrize("n_obs", (TILE - 1, TILE, TILE + 1))
def test_drop_list_lengths_at_the_scan_tile(c2b, n_obs):
    _check_drop(c2b, _case((5, 0, 300, n_obs - 305 - 64, 64), seed=n_obs), 0.5, seed=n_obs)


@pytest.mark.parametrize("n_cam", (CHUNK - 1, CHUNK, CHUNK + 1, TILE + 1))
def test_drop_camera_counts_at_the_scan_chunk(c2b, n_cam):
    lengths = np.random.default_rng(n_cam).integers(0, 6, n_cam)
    _check_drop(c2b, _case(tuple(int(x) for x in lengths), seed=n_cam), 0.6, seed=7)


def test_drop_keep_rows_level0_does_not_depend_on_the_other_rows(c2b):
    """the keep bits of a row are those of the same observation indices in any list: counter-based draws"""
    from city2ba_amd import device as D
    import torch
    P = _case(LENGTHS)
    row_ptr = P["row_ptr"].astype(np.int64)
    keep = torch.zeros(int(row_ptr[-1]), dtype=torch.uint8, device="cuda:0")
    D.drop_keep_rows(_dev(row_ptr), int(row_ptr[-1]), 0.5, 99, keep)
    torch.cuda.synchronize()
    assert np.array_equal(keep.cpu().numpy().astype(bool), R.drop_keep(row_ptr, 0.5, 99))


# ---- mismatch -------------------------------------------------------------------------------------------------------------
MISMATCH_SEED = 5


@pytest.mark.parametrize("chance", (0.0, 0.3, 1.0))
def test_mismatch_partner_and_apply(c2b, chance):
    from city2ba_amd import device as D
    import torch
    P = _case(LENGTHS)
    row_ptr = P["row_ptr"].astype(np.int64)
    n = int(row_ptr[-1])
    want, zero, ambiguous = R.mismatch_partner(row_ptr, P["uv"], chance, MISMATCH_SEED)
    assert not zero
    assert ambiguous == [], "the seed was picked so that the restatement sets no camera aside"
    partner = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    n_zero = torch.ones(1, dtype=torch.int64, device="cuda:0")
    D.mismatch_partner_rows(_dev(row_ptr), _dev(P["uv"]), chance, MISMATCH_SEED, partner, n_zero)
    torch.cuda.synchronize()
    got = partner.cpu().numpy()
    cam_of = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    aside = sorted(set(cam_of[got != want]) & set(ambiguous))
    assert len(aside) <= 1                                   # (none can be: the restatement found no ambiguous draw)
    ok = ~np.isin(cam_of, aside)
    assert np.array_equal(got[ok], want[ok])
    assert int(n_zero.item()) == 0
    if chance == 0.0:
        assert np.all(got == -1)
    if chance == 1.0:
        assert np.all(got[cam_of != 1] >= 0) and got[row_ptr[1]] == -1       # the row of one observation never swaps
    ba = _problem(c2b, P)
    swaps = ba.add_incorrect_correspondences(chance, seed=MISMATCH_SEED)
    assert swaps == int((want >= 0).sum())
    assert np.array_equal(ba.pt_idx[ok], R.mismatch_apply(row_ptr, P["pt_idx"], want)[ok])
    assert np.array_equal(ba.row_ptr, P["row_ptr"])
    assert np.array_equal(_bits(ba.observations().reshape(-1, 2)), _bits(P["uv"]))
    ba.close()


def test_mismatch_row_of_coinciding_positions_is_an_error_and_nothing_changes(c2b):
    P = dict(_case((4, 6, 3), seed=77))
    uv = P["uv"].copy()
    uv[4:10] = uv[4]                                         # camera 1: every pixel the same
    P["uv"] = uv
    _, zero, _ = R.mismatch_partner(P["row_ptr"], uv, 1.0, 1)
    assert zero == [1]
    ba = _problem(c2b, P)
    with pytest.raises(c2b.City2baError, match="all swap weights are zero"):
        ba.add_incorrect_correspondences(1.0, seed=1)
    assert np.array_equal(ba.pt_idx, P["pt_idx"])
    ba._refresh_graph()
    assert np.array_equal(ba.pt_idx, P["pt_idx"]) and np.array_equal(_bits(ba.observations().reshape(-1, 2)), _bits(uv))
    ba.close()


# ---- select ---------------------------------------------------------------------------------------------------------------
def _select(keys, n, n_sel, seed=0, stream=0, slot=0):
    from city2ba_amd import device as D
    import torch
    sel = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    D.select_smallest_keys_rows(n, n_sel, sel, seed=seed, stream=stream, slot=slot, keys=None if keys is None else _dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    return sel.cpu().numpy()


@pytest.mark.parametrize("N", (TILE - 1, TILE, TILE + 1, 2 * TILE + 77))
def test_select_smallest_keys_with_ties_and_shared_digits(c2b, N):
    rng = np.random.default_rng(N)
    # a pool of few values: full ties resolved by index; the pool shares its top five bytes, so the first five radix passes
    # cannot separate anything and the boundary falls inside a digit of the last three
    pool = (np.uint64(0xC3A5F00D12 << 24) | rng.integers(0, 1 << 24, 37).astype(np.uint64))
    pool[:4] = pool[4] + np.arange(1, 5, dtype=np.uint64)    # neighbours in the last digit
    tied = pool[rng.integers(0, len(pool), N)]
    spread = rng.integers(0, 1 << 63, N).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, N).astype(np.uint64)
    for keys in (tied, spread):
        for n_sel in (0, 1, N // 3, N - 1, N, N + 5):
            assert np.array_equal(_select(keys, N, n_sel).astype(bool), R.smallest(keys, n_sel)), n_sel
    for n_sel in (1, N // 2, N - 1):                         # the draws themselves: stream 8, slot 0, as split_landmarks selects
        a, _ = R.draws(31, R.STREAM_SPLIT, np.arange(N), 0)
        assert np.array_equal(_select(None, N, n_sel, seed=31, stream=R.STREAM_SPLIT).astype(bool), R.smallest(a, n_sel))


# ---- split ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", (0.0, 0.1, 1.0, 1.5))
def test_split_points_indices_and_state(c2b, f):
    P = _case((5, 0, 300, 64, 1100), n_pts=TILE + 3, seed=3)
    want_pts, want_idx, n = R.split_landmarks(P["pts"], P["pt_idx"], f, seed=13)
    ba = _problem(c2b, P)
    mask = np.arange(len(P["pts"])) % 2 == 0
    ba.set_constant(points=mask)
    ba.set_loss("cauchy", 2.0)
    assert ba.split_landmarks(f, seed=13) == n
    assert ba.num_points() == len(P["pts"]) + n
    assert np.array_equal(_bits(ba.points()), _bits(want_pts))
    assert np.array_equal(ba.pt_idx, want_idx.astype(np.uint64))
    assert np.array_equal(ba.row_ptr, P["row_ptr"])
    assert np.array_equal(_bits(ba.observations().reshape(-1, 2)), _bits(P["uv"]))
    assert ba.loss == ("cauchy", 2.0)                        # the handle's, as across cull
    if n:                                                    # the count changed: cull's policy, the masks are gone
        assert not ba.constant()[1].any() and len(ba.constant()[1]) == len(P["pts"]) + n
    else:
        assert np.array_equal(ba.constant()[1], mask)
    ba.close()


# ---- nearest points and join ------------------------------------------------------------------------------------------------
def _lattice():
    g = np.arange(6) * 0.25                                  # dyadic: every d2 is exact, ties are exact
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.concatenate([pts, pts[[0, 7, 100, 215, 100]]])            # exact duplicates, one point three times


def _slab():
    rng = np.random.default_rng(8)
    pts = np.column_stack([rng.uniform(0, 40, 2000), rng.uniform(0, 2, 2000), rng.uniform(0, 25, 2000)])
    return np.concatenate([pts, [[4000.0, 1.0, -3000.0]]])  # the shell walk crosses empty cells and still ends


def _small(n):
    return np.random.default_rng(n).normal(size=(n, 3))


def _flat(kind):
    rng = np.random.default_rng(2)
    t = rng.uniform(-3, 3, (150, 3))
    if kind == "plane_y":
        t[:, 1] = 0.5
    elif kind == "plane_x":
        t[:, 0] = -2.0
    elif kind == "line_x":
        t[:, 1:] = (1.0, 2.0)
    elif kind == "line_y":
        t[:, 0], t[:, 2] = 1.0, 2.0
    else:
        t[:] = (1.0, 2.0, 3.0)                               # every point the same
    return t


NEAREST_CASES = {"lattice": _lattice, "slab": _slab, "plane_y": lambda: _flat("plane_y"), "plane_x": lambda: _flat("plane_x"),
                 "line_x": lambda: _flat("line_x"), "line_y": lambda: _flat("line_y"), "one_spot": lambda: _flat("spot")}
NEAREST_CASES.update({"n%d" % n: (lambda n=n: _small(n)) for n in (1, 2, 5, 11, 12)})


@pytest.mark.parametrize("name", sorted(NEAREST_CASES))
def test_nearest_points_against_brute_force(c2b, name):
    from city2ba_amd import device as D
    import torch
    pts = NEAREST_CASES[name]()
    n = len(pts)
    query = np.arange(n) if n <= 300 else np.concatenate([np.arange(0, n, 7), [n - 1]])
    pts4 = np.zeros((n, 4))
    pts4[:, :3] = pts
    out = torch.full((len(query), R.NEAREST), -5, dtype=torch.int32, device="cuda:0")
    D.nearest_points_rows(_dev(pts4), _dev(query.astype(np.int32)), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.nearest_points(pts, query))


@pytest.mark.parametrize("name", ("lattice", "slab", "n2", "n5", "n12", "one_spot"))
def test_join_against_brute_force(c2b, name):
    pts = NEAREST_CASES[name]()
    rng = np.random.default_rng(len(pts))
    lengths = (3, 0, 70, 200, 1000)
    P = dict(_case(lengths, seed=5))
    P["pts"] = pts
    P["pt_idx"] = rng.integers(0, len(pts), int(P["row_ptr"][-1])).astype(np.uint64)
    f = 0.3 if len(pts) > 100 else 40.0                      # few points: as many as there are (and a cap at n_obs below)
    want, n = R.join_landmarks(pts, P["pt_idx"], f, seed=17)
    ba = _problem(c2b, P)
    mask = np.arange(len(pts)) % 2 == 1
    ba.set_constant(points=mask)
    assert ba.join_landmarks(f, seed=17) == n and n > 0
    assert np.array_equal(ba.pt_idx, want.astype(np.uint64))
    assert np.array_equal(ba.row_ptr, P["row_ptr"]) and np.array_equal(_bits(ba.points()), _bits(pts))
    assert np.array_equal(ba.constant()[1], mask)
    ba.close()


def test_join_caps_at_the_observations_and_needs_a_neighbour(c2b):
    P = dict(_case((2, 3), seed=9))
    P["pts"] = _small(12)
    P["pt_idx"] = np.array([0, 3, 5, 11, 7], dtype=np.uint64)
    ba = _problem(c2b, P)
    assert ba.join_landmarks(1.0, seed=2) == 5               # floor(1.0 * 12) = 12 > 5 observations
    assert np.array_equal(ba.pt_idx, R.join_landmarks(P["pts"], P["pt_idx"], 1.0, 2)[0].astype(np.uint64))
    ba.close()
    P["pts"] = _small(1)
    P["pt_idx"] = np.zeros(5, dtype=np.uint64)
    ba = _problem(c2b, P)
    assert ba.join_landmarks(0.5, seed=2) == 0               # floor(0.5 * 1) = 0: nothing to do
    with pytest.raises(c2b.City2baError, match="No neighbors"):
        ba.join_landmarks(1.0, seed=2)
    ba.close()


# ---- the chain ------------------------------------------------------------------------------------------------------------
def test_chain_drop_join_split_mismatch_with_culls(c2b):
    from _problems import grid_problem
    from city2ba_amd.baproblem import cull_arrays
    P = grid_problem()
    s = 40
    cams, pts = P["cams15"], P["pts"]
    row_ptr, pt_idx, uv = P["row_ptr"], P["pt_idx"], np.asarray(P["uv"]).reshape(-1, 2)
    ba = c2b.BAProblem.from_visibility(cams, pts, row_ptr, pt_idx, uv, device=0)

    def cull(cams, pts, row_ptr, pt_idx, uv):
        c, p, r, i, u = cull_arrays(cams, pts, np.asarray(row_ptr, dtype=np.uint64), np.asarray(pt_idx, dtype=np.uint64),
                                    np.ascontiguousarray(uv, dtype=np.float64))
        return c, p, r, i, np.asarray(u).reshape(-1, 2)

    row_ptr, pt_idx, uv = R.drop_features(row_ptr, pt_idx, uv, 0.8, s + 2)
    cams, pts, row_ptr, pt_idx, uv = cull(cams, pts, row_ptr, pt_idx, uv)
    pt_idx, n_join = R.join_landmarks(pts, pt_idx, 0.1, s + 3)
    cams, pts, row_ptr, pt_idx, uv = cull(cams, pts, row_ptr, pt_idx, uv)
    pts, pt_idx, n_split = R.split_landmarks(pts, pt_idx, 0.1, s + 4)
    cams, pts, row_ptr, pt_idx, uv = cull(cams, pts, row_ptr, pt_idx, uv)
    partner, zero, ambiguous = R.mismatch_partner(row_ptr, uv, 0.05, s + 5)
    assert not zero and not ambiguous
    pt_idx = R.mismatch_apply(row_ptr, pt_idx, partner)

    assert ba.drop_features(0.8, seed=s + 2) > 0
    ba.cull()
    assert ba.join_landmarks(0.1, seed=s + 3) == n_join > 0
    ba.cull()
    assert ba.split_landmarks(0.1, seed=s + 4) == n_split > 0
    ba.cull()
    assert ba.add_incorrect_correspondences(0.05, seed=s + 5) == int((partner >= 0).sum()) > 0

    assert np.array_equal(ba.row_ptr, np.asarray(row_ptr, dtype=np.uint64))
    assert np.array_equal(ba.pt_idx, np.asarray(pt_idx, dtype=np.uint64))
    assert np.array_equal(_bits(ba.observations().reshape(-1, 2)), _bits(uv))
    assert np.array_equal(_bits(ba.points()), _bits(pts))
    assert np.array_equal(_bits(ba.cameras()), _bits(cams))
    # a valid problem
    assert np.all(np.diff(ba.row_ptr.astype(np.int64)) >= 0) and int(ba.row_ptr[-1]) == len(ba.pt_idx) == ba.num_observations()
    assert len(ba.pt_idx) and int(ba.pt_idx.max()) < ba.num_points()
    ba.close()


# ---- the host route keeps its seeded outputs ----------------------------------------------------------------------------------
# sha256 over (points f64, row_ptr u64, pt_idx u64, uv f64) of the result on tests/_problems.grid_problem().  Recorded from a
# build of the parent commit by calling its four host entries (c2b_drop_features, c2b_add_incorrect_correspondences,
# c2b_split_landmarks, c2b_join_landmarks) with the arguments below on the same arrays; the Python wrappers add a download and an
# upload around them, which keep every bit.
HOST_ROUTE = {
    "drop_features": "99a3282f09be7559b0e5a56626c69a90db7cb7f5930f4d33bf8d46322c482a20",
    "add_incorrect_correspondences": "159a878a5964c091a7636b9a27020e987f6811cb5b68066c0959927ebfa54f07",
    "split_landmarks": "3737180773f4e3d996af74ec5d14e176b6341d526200f559404ad532eb9a83b9",
    "join_landmarks": "2c66657a1dca648662d720e98224a9f23ac7073b08d1f9e86f979071a432b451",
}


@pytest.mark.parametrize("name", sorted(HOST_ROUTE))
def test_host_route_is_unchanged(c2b, name):
    from _problems import grid_problem
    from city2ba_amd import noise
    P = grid_problem()
    ba = c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    out = getattr(noise, name)(ba, 0.1, seed=3)              # default arguments: the host route
    assert out is not ba
    h = hashlib.sha256()
    for a, dt in ((out.points(), np.float64), (out.row_ptr, np.uint64), (out.pt_idx, np.uint64), (out.observations(), np.float64)):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    assert h.hexdigest() == HOST_ROUTE[name]
    # and on_device=True is the other scheme, in place
    same = getattr(noise, name)(ba, 0.1, seed=3, on_device=True)
    assert same is ba
    out.close()
    ba.close()
