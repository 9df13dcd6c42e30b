"""The step kernel's 512-thread x 2-tile launches cut the tile list 11 : 9 between even and odd XCDs (csrc/xcd_cuts.hpp)
instead of in equal eighths; what they compute must not have moved.

Reference: the 1 024-thread x 1-tile shape of the same library, whose map (xcd_tile32) and code this change does not touch
and which wrote the same r / Jc / Jp bits as the 512 x 2 shape before it (tests/test_gpu_k2_mix.py).  Compared bit for
bit, into buffers filled with NaN first, so a tile no workgroup took -- or took twice with another tile's data -- shows.
The folded sum (its root, the L2 norm) is held to the CPU oracle at 1e-12 (its last bits move with the grid, as between any two launch shapes).

The shape takes lists of 6 M observations and more only, so the sizes are just above that (synthetic --blocks 72: 6 132 074
observations, 95 814 tiles of 64 -- not a multiple of 16, the last workgroup tile is part filled, the last tile too): the
whole list; a launch that starts inside it (obs_base != 0: other cuts over other rows); shorter launches whose tile
counts leave 0 ... 7 tiles over after the shares.  Cuts fall every 1 024 observations where a camera's row has a few tens: the
test asserts that rows do straddle them.  Empty XCD ranges and the equal-cuts identity cannot be reached through a launch
of this size: tests/test_xcd_cuts.py walks the map itself for those."""
import argparse
import math

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import bench
    import city2ba_amd
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0
    dev = torch.device("cuda", 0)
    sh = bench.build_shard(argparse.Namespace(blocks=72), 0, 1, dev)
    n = sh["n_obs"]
    assert n == 6_132_074 and ((n + 63) // 64) % 16 != 0
    ws = D.workspace(n, dev)
    # the reference, once: 1 024 threads x 1 tile (a set between the store classes), equal eighths
    outs = D.JacobianOutputs(n, dev, max_attempts=1)
    outs.set_store_rate(6500.0)
    assert D.jacobian_launch_shape(n, 6500.0) == (16, 1) and D.jacobian_launch_shape(n, 0.0) == (8, 2)
    e = torch.zeros(1, dtype=torch.float64, device=dev)
    outs.r.fill_(float("nan")); outs.Jc.fill_(float("nan")); outs.Jp.fill_(float("nan"))
    D.residual_jacobian_rows_placed(sh["camblk"], sh["pts4"], sh["rows"], sh["pt_idx"], sh["uv"], outs, 2.0, ws, e)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs.r).all()) and bool(torch.isfinite(outs.Jc).all()) and bool(torch.isfinite(outs.Jp).all())
    got = tuple(torch.full((n, k), float("nan"), dtype=torch.float64, device=dev) for k in (2, 18, 6))
    return dict(torch=torch, D=D, dev=dev, sh=sh, n=n, ws=ws, ref=(outs.r, outs.Jc, outs.Jp), keep=outs, e_ref=e.item(), got=got)


def _host(sh):
    row_ptr = sh["rows"].row_ptr.cpu().numpy().astype(np.uint64)
    return (sh["cam15"].cpu().numpy(), np.ascontiguousarray(sh["pts4"][:, :3].cpu().numpy()), row_ptr,
            sh["pt_idx"].cpu().numpy().astype(np.uint64), sh["uv"].cpu().numpy())


def _cut_observations(n_obs):
    """first observations of the XCD ranges of a launch of n_obs observations (xcd_cuts.hpp, restated: 11 : 9)"""
    bt = ((n_obs + 63) // 64 + 15) // 16
    lens = [bt * (9 if x & 1 else 11) // 80 for x in range(8)]
    left = bt - sum(lens)
    lens = [v + (1 if x < left else 0) for x, v in enumerate(lens)]
    return [1024 * int(c) for c in np.cumsum(lens)[:-1]]


def _launch(big, obs_base, m, with_sum=True):
    torch, D, sh = big["torch"], big["D"], big["sh"]
    r, Jc, Jp = (t[:m] for t in big["got"])
    r.fill_(float("nan")); Jc.fill_(float("nan")); Jp.fill_(float("nan"))
    e = torch.full((1,), -1.0, dtype=torch.float64, device=big["dev"])
    assert D.jacobian_launch_shape(m, 0.0) == (8, 2)
    D.residual_jacobian_rows(sh["camblk"], sh["pts4"], sh["rows"], sh["pt_idx"][obs_base:obs_base + m], sh["uv"][obs_base:obs_base + m],
                             r, Jc, Jp, 2.0, big["ws"] if with_sum else None, e if with_sum else None, obs_base=obs_base, n_obs=m)
    torch.cuda.synchronize()
    for got, ref in zip((r, Jc, Jp), big["ref"]):
        assert torch.equal(got.view(torch.int64), ref[obs_base:obs_base + m].view(torch.int64)), (obs_base, m)
    return e.item()


def test_whole_list_bits_and_sum(big):
    n = big["n"]
    e1 = _launch(big, 0, n)
    assert _launch(big, 0, n) == e1                                    # same grid, same bits
    cams15, pts, row_ptr, pt_idx, uv = _host(big["sh"])
    want = O.total_reprojection_error(cams15, pts, row_ptr, pt_idx, uv, 2.0)      # the L2 norm: the root of the folded sum
    print("sum: 512 x 2 cut map %.17g, 1 024 x 1 %.17g, oracle's norm squared %.17g" % (e1, big["e_ref"], want * want))
    assert abs(math.sqrt(e1) - want) <= 1e-12 * want and abs(math.sqrt(big["e_ref"]) - want) <= 1e-12 * want
    starts = set(int(v) for v in row_ptr)
    cuts = _cut_observations(n)
    assert len(cuts) == 7 and sum(c not in starts for c in cuts) >= 5, "camera rows straddle the cuts"


def test_launch_from_inside_the_list(big):
    """obs_base != 0: the tile records, the row search of flagged tiles and the cuts all move"""
    base = 64 * 1501
    m = big["n"] - base
    assert m >= 6_000_000
    e = _launch(big, base, m)
    r = big["ref"][0][base:].cpu().numpy()                            # the sum of this slice, from residuals already held to the oracle's bits
    want = float(np.sum(r.astype(np.longdouble) ** 2))
    assert abs(e - want) <= 1e-12 * want


@pytest.mark.parametrize("drop_tiles", [1, 16 * 3 + 5, 16 * 8 * 2 + 16 * 7])
def test_shorter_launches_move_every_cut(big, drop_tiles):
    """tile counts with other remainders after the shares (the leftover workgroup tiles go to the first ranges), a last tile
    that is full / part filled, without the sum (the no-sum launch takes another shape: still the reference's bits)"""
    m = big["n"] - 64 * drop_tiles + (0 if drop_tiles == 1 else 7)
    m = min(m, big["n"])
    assert m >= 6_000_000
    _launch(big, 0, m)
    _launch(big, 0, m, with_sum=False)


def test_camera_index_form_takes_the_same_map(big):
    """one camera index per observation instead of the row structure: the same shape, the same cuts, the same bits and sum"""
    torch, D, sh, n = big["torch"], big["D"], big["sh"], big["n"]
    e_rows = _launch(big, 0, n)
    r, Jc, Jp = big["got"]
    r.fill_(float("nan")); Jc.fill_(float("nan")); Jp.fill_(float("nan"))
    e = torch.full((1,), -1.0, dtype=torch.float64, device=big["dev"])
    D.residual_jacobian_sum(sh["camblk"], sh["pts4"], sh["cam_idx"], sh["pt_idx"], sh["uv"], r, Jc, Jp, 2.0, big["ws"], e)
    torch.cuda.synchronize()
    for got, ref in zip((r, Jc, Jp), big["ref"]):
        assert torch.equal(got.view(torch.int64), ref.view(torch.int64))
    assert e.item() == e_rows
