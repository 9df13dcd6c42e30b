"""The step kernel's workgroup -> tile map for its 512-thread x 2-tile shape (city2ba_amd/csrc/xcd_cuts.hpp), on the host.

The header is plain C++: it is compiled here on its own with a small C wrapper, and the map -- the very functions the
launcher and the kernel call -- is walked workgroup by workgroup.  Whatever the cuts, every workgroup tile must be taken by
exactly one workgroup of the grid and every other workgroup must get -1 (it then only folds); with equal shares the map
must be the equal eighths of xcd_tile32, which the other two launch shapes keep.  The GPU half:
tests/test_gpu_xcd_cuts.py."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "city2ba_amd", "csrc", "xcd_cuts.hpp")

WRAPPER = r"""
#include "%s"
extern "C" int cuts_make(int n_tiles, int even_share, int odd_share, int *cut9) {
    c2b::XcdCuts m;
    const int grid = c2b::xcd_cuts_make(n_tiles, even_share, odd_share, m);
    for (int x = 0; x < 9; ++x) cut9[x] = m.cut[x];
    return grid;
}
// tile_of[b] for every workgroup of the grid
extern "C" void cuts_walk(const int *cut9, int grid, int *tile_of) {
    c2b::XcdCuts m;
    for (int x = 0; x < 9; ++x) m.cut[x] = cut9[x];
    for (int b = 0; b < grid; ++b) tile_of[b] = c2b::xcd_cut_tile(b, m);
}
extern "C" int shipped_even() { return c2b::kXcdEvenShare; }
extern "C" int shipped_odd() { return c2b::kXcdOddShare; }
"""


@pytest.fixture(scope="module")
def cuts(tmp_path_factory):
    d = tmp_path_factory.mktemp("xcd_cuts")
    src, so = str(d / "wrap.cpp"), str(d / "libwrap.so")
    with open(src, "w") as fh:
        fh.write(WRAPPER % HEADER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.cuts_make.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.cuts_walk.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    return lib


def _make(lib, n, even, odd):
    cut = (C.c_int * 9)()
    grid = lib.cuts_make(n, even, odd, cut)
    return list(cut), grid


def _walk(lib, cut, grid):
    out = (C.c_int * max(grid, 1))()
    lib.cuts_walk((C.c_int * 9)(*cut), grid, out)
    return list(out)[:grid]


def xcd_tile32(bid, n_tiles):                      # kernels.hpp, restated
    q, r = n_tiles >> 3, n_tiles & 7
    xcd, k = bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + k


SIZES = list(range(0, 70)) + [127, 128, 129, 1000, 5861, 5989, 18850, 18851]


def test_equal_shares_are_the_equal_eighths_of_xcd_tile32(cuts):
    for n in SIZES:
        cut, grid = _make(cuts, n, 1, 1)
        assert grid == 8 * ((n + 7) // 8)
        tiles = _walk(cuts, cut, grid)
        for b in range(grid):
            if b < n:
                assert tiles[b] == xcd_tile32(b, n), (n, b)
            else:                                  # the workgroups a one-shot grid of n never had
                assert tiles[b] == -1, (n, b)


@pytest.mark.parametrize("even,odd", [(None, None), (1, 1), (3, 1), (1, 3), (1, 0), (0, 1), (1000, 1)])
def test_every_tile_is_taken_once_whatever_the_cuts(cuts, even, odd):
    """the shipped shares, lopsided ones, and shares that leave four XCD ranges empty; tile counts below eight leave ranges
    empty under any shares"""
    if even is None:
        even, odd = cuts.shipped_even(), cuts.shipped_odd()
    for n in SIZES:
        cut, grid = _make(cuts, n, even, odd)
        assert cut[0] == 0 and cut[8] == n and all(cut[x] <= cut[x + 1] for x in range(8)), (n, cut)
        assert grid == 8 * max(cut[x + 1] - cut[x] for x in range(8))
        tiles = _walk(cuts, cut, grid)
        taken = sorted(t for t in tiles if t >= 0)
        assert taken == list(range(n)), (n, even, odd)
        assert all(t >= -1 for t in tiles)
        for b, t in enumerate(tiles):              # XCD b % 8 streams its own range in order
            if t >= 0:
                assert cut[b & 7] <= t < cut[(b & 7) + 1] and t - cut[b & 7] == b >> 3


def test_shipped_shares_and_the_grid_they_need(cuts):
    """11 : 9 between even and odd XCDs; the grid stays within the one partial per four tiles of 64
    observations that the workspace holds (a workgroup tile of this shape is sixteen of them)"""
    even, odd = cuts.shipped_even(), cuts.shipped_odd()
    assert (even, odd) == (11, 9)
    for n in SIZES:
        cut, grid = _make(cuts, n, even, odd)
        assert grid <= 1.1 * n + 8
        assert grid <= max(4 * n, 4096) + 8        # capi.hip: block_part_slots, in workgroup tiles of this shape
        lens = [cut[x + 1] - cut[x] for x in range(8)]
        for x in range(8):
            want = n * (even if x % 2 == 0 else odd) / (4.0 * (even + odd))
            assert abs(lens[x] - want) <= 1.0, (n, x, lens)
    cut, grid = _make(cuts, 18851, even, odd)      # the headline launch: 19 302 494 observations
    assert [cut[x + 1] - cut[x] for x in range(8)] == [2593, 2121, 2593, 2120, 2592, 2120, 2592, 2120] and grid == 20744
