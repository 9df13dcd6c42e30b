"""The sizes at which a device scan can go wrong (csrc/scan_kernels.hpp), through public entries only, against numpy
(cumsum, argsort(kind="stable"), boolean masks), exactly.  Every scan of the library is the one workgroup primitive, the
one-workgroup chunk loop (k_scan_short) or the tiled path (k_scan_tiles, k_scan_short over the tile sums, k_scan_add):

  u32 -> u64, tiled, row-pointer form      the point-major transpose (D.PointRows)
  u64 -> u64, one workgroup                the row pointer of a compacted list (filter_observations), the dense count
  u32 -> u32, tiled, total to the host     cull's renumbering
  u32 -> u64, tiled, with a start offset   the tile bases of the text writer (offset = the header) and reader

The sizes below follow kScanBlock = 256 (the chunk of the one-workgroup loop) and kScanTile = 1024 (a tile of the tiled
path) of scan_kernels.hpp; if those constants change, these follow them."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

CHUNK, TILE = 256, 1024                                      # kScanBlock, kScanTile
TILE_EDGES = (0, 1, TILE - 1, TILE, TILE + 1)
CHUNK_EDGES = (CHUNK - 1, CHUNK, CHUNK + 1)
SUMS_EDGES = (CHUNK * TILE - 1, CHUNK * TILE + 1)            # the tile sums themselves span more than one chunk


@pytest.fixture(scope="module")
def c2b():
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd
    assert city2ba_amd.device_count() > 0
    return city2ba_amd


# ---- u32 -> u64: the transpose ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", TILE_EDGES + CHUNK_EDGES + SUMS_EDGES)
def test_transpose_at_the_scan_edges(c2b, n_pts):
    import torch
    from city2ba_amd import device as D
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 + n_pts)
    n_obs = n_pts + (3 if n_pts else 0)
    observed = max(1, n_pts - n_pts // 10 - 2)               # the last tenth of the points (and two more) is unobserved
    pt_idx = rng.integers(0, observed, n_obs).astype(np.int64)
    n_cam = 7
    cuts = np.sort(rng.integers(0, n_obs + 1, n_cam - 1))
    row_ptr = np.concatenate([[0], cuts, [n_obs]]).astype(np.int64)
    rows = D.Rows(torch.from_numpy(row_ptr).to(dev), n_obs)
    pr = D.PointRows(rows, torch.from_numpy(pt_idx.astype(np.int32)).to(dev), n_pts)
    torch.cuda.synchronize()
    want = np.argsort(pt_idx, kind="stable")
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt_idx, minlength=n_pts))]).astype(np.int64)
    cam_of = np.repeat(np.arange(n_cam), np.diff(row_ptr))
    assert np.array_equal(pr.pt_row_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(pr.obs_of.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(pr.cam_of.cpu().numpy().astype(np.int64), cam_of[want])


# ---- u64 -> u64: the row pointer of a compacted list --------------------------------------------------------------------
def _flat_cameras(centres):
    """cameras with R = 1, f = 1 and no distortion at these centres, looking down -z"""
    bal9 = np.zeros((len(centres), 9))
    bal9[:, 3:6] = -np.asarray(centres, dtype=np.float64)    # t = -R c
    bal9[:, 6] = 1.0
    return O.camera_from_bal(bal9)


_FILTER = {}


def _filter_case(n_cam):
    """n_cam cameras at the origin, two or three observations each of 16 points in front of them; the observation is
    the oracle's projection, moved by 1 in u where the mask says `remove`: a residual of 0 (to rounding) or of 1 against
    a threshold of 0.5, so the kept set is the mask and no rounding decides anything"""
    if n_cam not in _FILTER:
        rng = np.random.default_rng(2000 + n_cam)
        cams = _flat_cameras(np.zeros((n_cam, 3)))
        pts = np.column_stack([rng.uniform(-1, 1, 16), rng.uniform(-1, 1, 16), rng.uniform(-6, -3, 16)])
        counts = rng.integers(2, 4, n_cam)
        row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        n = int(row_ptr[-1])
        pt_idx = rng.integers(0, 16, n).astype(np.uint64)
        keep = rng.random(n) < 0.5
        if n_cam >= 2:                                       # one camera loses its whole row
            c = n_cam // 2
            keep[int(row_ptr[c]):int(row_ptr[c + 1])] = False
        uv = O.project_observations(cams, pts, row_ptr, pt_idx).reshape(-1, 2).copy()
        uv[~keep, 0] += 1.0
        _FILTER[n_cam] = dict(cams=cams, pts=pts, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv, keep=keep)
    return _FILTER[n_cam]


@pytest.mark.parametrize("n_cam", TILE_EDGES[1:] + CHUNK_EDGES)
def test_filter_row_pointer_at_the_scan_edges(c2b, n_cam):
    P = _filter_case(n_cam)
    keep, row_ptr = P["keep"], P["row_ptr"].astype(np.int64)
    cam_of = np.repeat(np.arange(n_cam), np.diff(row_ptr))
    want_rows = np.concatenate([[0], np.cumsum(np.bincount(cam_of[keep], minlength=n_cam))]).astype(np.uint64)
    ba = c2b.BAProblem.from_visibility(P["cams"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    assert ba.filter_observations(10.0) == 0                 # removes nothing: the lists stay as they are
    assert np.array_equal(ba.row_ptr, P["row_ptr"]) and np.array_equal(ba.pt_idx, P["pt_idx"])
    assert np.array_equal(ba.observations().reshape(-1, 2).view(np.uint64), P["uv"].view(np.uint64))
    assert ba.filter_observations(0.5) == int((~keep).sum())
    assert np.array_equal(ba.row_ptr, want_rows)
    assert np.array_equal(ba.pt_idx, P["pt_idx"][keep])
    assert np.array_equal(ba.observations().reshape(-1, 2).view(np.uint64), P["uv"][keep].view(np.uint64))
    if n_cam >= 2:
        assert want_rows[n_cam // 2] == want_rows[n_cam // 2 + 1]
    ba.close()


def test_dense_count_over_more_cameras_than_a_tile(c2b):
    """c2b_visibility_dense_count at n_cam = 1025: cameras of three kinds -- at the origin (see both groups of points), far
    away (see none), at z = -4 (the first group is behind them) -- and eight points, every decision far from its boundary"""
    n_cam = TILE + 1
    kind = np.arange(n_cam) % 3
    centres = np.zeros((n_cam, 3))
    centres[kind == 1, 0] = 1000.0
    centres[kind == 2, 2] = -4.0
    x = np.array([-0.4, -0.1, 0.2, 0.5])
    pts = np.concatenate([np.column_stack([x, 0.5 * x, np.full(4, -2.0)]), np.column_stack([x, -0.5 * x, np.full(4, -6.0)])])
    sees = {0: np.arange(8), 1: np.zeros(0, dtype=np.int64), 2: np.arange(4, 8)}
    want_rows = np.concatenate([[0], np.cumsum([len(sees[k]) for k in kind])]).astype(np.uint64)
    want_pts = np.concatenate([sees[k] for k in kind]).astype(np.uint64)
    ba = c2b.BAProblem.from_visibility(_flat_cameras(centres), pts, np.zeros(n_cam + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64),
                                       np.zeros((0, 2)), device=0)
    row_ptr, pt_idx, uv = ba.visibility_graph(10.0, dense=True)
    assert np.array_equal(row_ptr, want_rows) and np.array_equal(pt_idx, want_pts)
    ba.close()


# ---- u32 -> u32 with the total on the host: cull ------------------------------------------------------------------------
def test_cull_over_more_observations_than_a_chunk_of_tiles(c2b):
    """1100 cameras x 240 observations = 264 000 > 256 * 1024 + 1: the scan of the observations' keep flags has more tile
    sums than one chunk.  Every camera sees 240 points of a window of 400 around its place; one observation of every
    seventh camera is of a point nobody else sees (a singleton: removed, and the camera's count with it)."""
    from city2ba_amd.baproblem import cull_arrays
    rng = np.random.default_rng(3)
    n_cam, per, n_shared = 1100, 240, 30000
    assert n_cam * per > SUMS_EDGES[1]
    cols = []
    for c in range(n_cam):
        start = int(c * (n_shared - 400) / (n_cam - 1))
        cols.append(np.sort(rng.choice(np.arange(start, start + 400), size=per, replace=False)))
    lonely = np.arange(0, n_cam, 7)
    for k, c in enumerate(lonely):
        cols[c][-1] = n_shared + k                           # still ascending: the singletons' indices follow the shared points'
    pt_idx = np.concatenate(cols).astype(np.uint64)
    row_ptr = (np.arange(n_cam + 1) * per).astype(np.uint64)
    n_pts = n_shared + len(lonely)
    cams = rng.uniform(-1, 1, (n_cam, 15))
    cams[:, :9] = np.eye(3).reshape(9)
    pts = rng.uniform(-5, 5, (n_pts, 3))
    uv = rng.uniform(-1, 1, (len(pt_idx), 2))
    want = cull_arrays(cams, pts, row_ptr, pt_idx, uv, False)
    ba = c2b.BAProblem.from_visibility(cams, pts, row_ptr, pt_idx, uv, device=0)
    ba.cull(False)
    assert 0 < len(want[3]) < len(pt_idx) and len(want[1]) < n_pts
    assert (ba.num_cameras(), ba.num_points(), ba.num_observations()) == (len(want[0]), len(want[1]), len(want[3]))
    assert np.array_equal(ba.row_ptr, want[2]) and np.array_equal(ba.pt_idx, want[3])
    assert np.array_equal(ba.cameras(), want[0]) and np.array_equal(ba.points(), want[1])
    assert np.array_equal(ba.observations(), want[4])
    ba.close()


# ---- u32 -> u64 with a start offset: the text form ----------------------------------------------------------------------
def test_text_write_and_read_over_more_units_than_a_tile_of_tiles(c2b, tmp_path):
    """The writer scans one byte count per tile of 256 units (an observation line, or one value of a camera / point line),
    starting at the header's length; the reader one token count per 4096 bytes.  9 n_cam + 3 n_pts + n_obs is a little
    above 256 * 1024 units, so the writer's scan crosses one tile of tiles; the reader's crosses two."""
    from city2ba_amd.baproblem import write_bal
    rng = np.random.default_rng(4)
    n_cam, n_pts, per = 100, 20000, 2020
    n_obs = n_cam * per
    tiles = -(-n_obs // CHUNK) + -(-9 * n_cam // CHUNK) + -(-3 * n_pts // CHUNK)
    assert TILE < tiles < TILE + 16
    bal9 = np.column_stack([rng.uniform(-1, 1, (n_cam, 3)), rng.uniform(-50, 50, (n_cam, 3)), rng.uniform(0.8, 1.2, n_cam),
                            rng.uniform(-1e-2, 1e-2, (n_cam, 2))])
    pts = rng.uniform(-100, 100, (n_pts, 3))
    row_ptr = (np.arange(n_cam + 1) * per).astype(np.uint64)
    pt_idx = rng.integers(0, n_pts, n_obs).astype(np.uint64)
    uv = rng.uniform(-1, 1, (n_obs, 2))
    ba = c2b.BAProblem.from_bal(bal9, pts, row_ptr, pt_idx, uv, device=0)
    a, b = str(tmp_path / "dev.bal"), str(tmp_path / "host.bal")
    ba.write(a)
    write_bal(b, ba.cameras_bal(), ba.points(), ba.row_ptr, ba.pt_idx, ba.observations(), None)
    text = open(a, "rb").read()
    assert text == open(b, "rb").read()
    assert len(text) > 2 * TILE * 4096
    c2b.set_default_options(text_device_min_bytes=0, text_device_strict=True)        # the device parses it, or the read fails
    back = c2b.BAProblem.from_file(a)
    c2b.set_default_options(text_device_strict=False)
    assert np.array_equal(back.row_ptr, ba.row_ptr) and np.array_equal(back.pt_idx, ba.pt_idx)
    for x, y in ((back.cameras_bal(), ba.cameras_bal()), (back.points(), ba.points()), (back.observations(), ba.observations())):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    back.close()
    ba.close()
