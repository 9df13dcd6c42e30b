"""The resident problem gives back the device memory it takes ("Who owns it").  A handle's arrays, and the temporaries of
every call on it, are DevBuf objects; a member that a free function forgets, or a buffer moved into the handle without
its old array being freed, computes the right thing and fails nowhere -- it only leaks.  So one handle is taken
through every way its members are allocated, replaced and dropped, again and again, and the device's free memory is read
before and after."""
import os

import numpy as np
import pytest

from _problems import grid_cameras_points, grid_candidate_pairs

pytestmark = pytest.mark.gpu

MAX_DIST = 10.0
CYCLES = 10
# The grids (blocks, cameras per block, points per block; block length 5).  "smallest": the smallest grid of
# tests/_problems.py -- 8 cameras, 24 points, 46 observations within MAX_DIST -- whose cull still removes something (to 4
# cameras, 11 points, 31 observations) and that has cameras and points to hold constant.  The runtime serves allocations
# that small out of blocks it keeps, so this size sees a leak only once it has filled a block: a library built with
# drop_rows forgetting the solver's buffers lost 0 bytes here.  "mid" (480 cameras, 2 880 points, 197 158 observations;
# culls to 472, 2 877, 196 968) is the grid of the other GPU tests; its observation arrays and solver buffers are
# megabytes, and that same library lost 20 971 520 bytes.
GRIDS = {"smallest": (1, 1, 1), "mid": (3, 10, 20)}
# Bytes the device's free memory may drop over CYCLES cycles after one warm-up cycle.  The parent of the change that
# introduced DevBuf frees by hand and does not leak on this path, so what it loses is the noise of the runtime's own
# pools: PARENT_DROPS are three runs of this very measurement on its library (separate processes, one MI355X), and the
# bound is twice the largest -- set from them, never from the code under test.
PARENT_DROPS = {"smallest": (0, 0, 0), "mid": (0, 0, 0)}


def grid_problem(grid):
    import oracle as O
    blocks, cpb, ppb = GRIDS[grid]
    cams, pts = grid_cameras_points(blocks, cpb=cpb, ppb=ppb, L=5.0)
    ci, pi = grid_candidate_pairs(cams, pts, MAX_DIST)
    uv, keep = O.visibility_pairs(cams, pts, ci, pi, MAX_DIST)
    keep = keep.astype(bool)
    ci, pi, uv = ci[keep], pi[keep], uv[keep]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=len(cams)))]).astype(np.uint64)
    uv = uv + np.random.default_rng(5).normal(scale=1e-3, size=uv.shape)          # a step to solve for
    cmask = np.zeros(len(cams), np.uint16)
    cmask[0] = 0x1ff                                                              # the first camera whole, every third point
    return dict(cams=cams, pts=pts, row_ptr=row_ptr, pt_idx=pi.astype(np.uint64), uv=uv, cmask=cmask,
                pmask=(np.arange(len(pts)) % 3 == 0))


def cycle(c2b, P, tmp):
    """create, upload, set_constant, solve_step under Schur-Jacobi, project, dense visibility + adopt, cull, a .bbal written
    and read back, destroy"""
    ba = c2b.BAProblem.from_visibility(P["cams"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    ba.set_constant(cameras=P["cmask"], points=P["pmask"])
    ba.set_preconditioner("schur_jacobi")
    ba.solve_step(1e-3, max_iters=10)
    ba.project()
    ba.visibility_graph(MAX_DIST, fetch=False, dense=True)
    ba.adopt_visibility()
    before = (ba.num_cameras(), ba.num_points(), ba.num_observations())
    ba.cull()
    after = (ba.num_cameras(), ba.num_points(), ba.num_observations())
    assert 0 < after[0] < before[0] and 0 < after[1] < before[1], (before, after)
    path = os.path.join(tmp, "cycle.bbal")
    ba.write(path)
    back = c2b.BAProblem.from_file(path)
    assert (back.num_cameras(), back.num_points(), back.num_observations()) == after
    back.close()
    ba.close()


def free_memory_drop(c2b, tmp, grid):
    """bytes of free device memory lost over CYCLES cycles, after one cycle that warms the runtime's pools up"""
    import torch
    P = grid_problem(grid)
    cycle(c2b, P, tmp)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(CYCLES):
        cycle(c2b, P, tmp)
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("grid", sorted(GRIDS, reverse=True))
def test_ten_cycles_of_a_problem_leave_the_free_memory_where_it_was(tmp_path, grid):
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd as c2b
    assert c2b.device_count() > 0
    drop, bound = free_memory_drop(c2b, str(tmp_path), grid), 2 * max(PARENT_DROPS[grid])
    print("%s grid: free device memory dropped by %d bytes over %d cycles (bound %d; the parent's three runs: %s)"
          % (grid, drop, CYCLES, bound, ", ".join(map(str, PARENT_DROPS[grid]))))
    assert drop <= bound
