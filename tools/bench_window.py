#!/usr/bin/env python3
"""Time of sub-problem extraction and of a window sweep on tools/bench_lm.py's noisy synthetic grid.

1. BAProblem.window for 1 024 and 16 384 consecutive seed cameras from the middle of the problem, halo and no-halo, end to
   end: the call is synchronous (it sizes the child from counts it reads back), so its wall time is the device's time plus
   the host's; the median over `--repeats` calls after a warm-up, with the child's sizes and the bytes the call must move
   at least -- one read of cam_idx + pt_idx per marking pass, and the child's own arrays read and written -- over the HBM rate.
2. The comparator: the host subset this entry replaced (download cameras, points and observations, a Python loop over the
   selected cameras, upload), on the lists the halo window selects, by wall clock.
3. One solve_windows sweep (windows of `--size` cameras) against the full levenberg_marquardt_device with the same
   iterations per solve: wall time and the cost reached.
Prints one JSON line.

    python tools/bench_window.py [--blocks 128] [--repeats 7] [--out profiles/window_bench_blocks128.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_subset(c2b, np, ba, ci, pi):
    """BAProblem.subset as it was before the device entry: everything down, a loop over the cameras, a new problem up"""
    cams, pts, uv = ba.cameras(), ba.points(), ba.observations()
    new_of = np.full(len(pts), -1, dtype=np.int64)
    new_of[pi] = np.arange(len(pi))
    rows, cols, vals = [0], [], []
    for c in ci:
        a, b = int(ba.row_ptr[c]), int(ba.row_ptr[c + 1])
        p_new = new_of[ba.pt_idx[a:b].astype(np.int64)]
        k = p_new >= 0
        cols.append(p_new[k])
        vals.append(uv[a:b][k])
        rows.append(rows[-1] + int(k.sum()))
    cols = np.concatenate(cols).astype(np.uint64) if cols else np.zeros(0, np.uint64)
    vals = np.concatenate(vals) if vals else np.zeros((0, 2))
    return c2b.BAProblem.from_visibility(cams[ci], pts[pi], np.array(rows, dtype=np.uint64), cols, vals.reshape(-1, 2), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--sigma", type=float, default=1e-3, help="observation noise")
    ap.add_argument("--point-std", type=float, default=1e-2, help="noise on the points the solves start from")
    ap.add_argument("--repeats", type=int, default=7, help="timed calls; the median is reported")
    ap.add_argument("--size", type=int, default=16384, help="cameras per window of the sweep")
    ap.add_argument("--iterations", type=int, default=10, help="LM iterations per solve")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import numpy as np
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import noise as N, solve

    ba = B.bench_grid(a.blocks)
    N.add_noise(ba, 0.0, 0.0, a.point_std, a.sigma, seed=3)
    n_cam, n_pts, n_obs = ba._sizes()
    start = (ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())

    def wall(fn, repeats):
        out = []
        for _ in range(repeats):
            dt, child = B.wall_s(fn)
            out.append(dt)
            child.close()
        return B.median(out), B.spread([dt * 1e3 for dt in out], 3)

    extraction = {}
    for seeds in (1024, 16384):
        if seeds > n_cam:
            continue
        lo = (n_cam - seeds) // 2
        idx = np.arange(lo, lo + seeds)
        for halo in (True, False):
            child = ba.window(idx, halo=halo)                # warm-up, and the sizes
            nc, npt, no = child._sizes()
            origin = child.origin()
            child.close()
            t, spread = wall(lambda: ba.window(idx, halo=halo), a.repeats)
            # two marking passes read cam_idx + pt_idx; the fill reads the child's rows of the parent and writes the child
            # (12 + 4 + 16 bytes in, 4 + 4 + 16 out per observation); the entities are gathered (15 + 9 and 4 doubles, in and out)
            floor_bytes = 2 * 8 * n_obs + no * (32 + 24) + nc * 2 * 8 * 24 + npt * 2 * 8 * 4
            rec = dict(seed_cameras=seeds, halo=halo, cameras=nc, points=npt, observations=no, wall_ms=round(t * 1e3, 3), spread_ms=spread,
                       floor_bytes=floor_bytes, floor_ms_at_hbm_peak=round(floor_bytes / B.HBM_PEAK_BYTES_PER_S * 1e3, 4),
                       time_over_floor=round(t / (floor_bytes / B.HBM_PEAK_BYTES_PER_S), 1))
            if halo:
                th, spread_h = wall(lambda: host_subset(c2b, np, ba, origin["cam_of"].astype(np.int64), origin["pt_of"].astype(np.int64)), 3)
                rec["host_subset_wall_ms"] = round(th * 1e3, 1)
                rec["host_subset_spread_ms"] = spread_h
            extraction["%d_%s" % (seeds, "halo" if halo else "nohalo")] = rec
    ba.close()

    def fresh():
        return c2b.BAProblem.from_bal(*start, device=0)

    def cost(g):
        return g.total_reprojection_error(2.0) ** 2
    g = fresh()
    solve.solve_window(g, range(0, min(1024, n_cam)), iterations=1)          # the first solve of a process pays for the kernels' load
    g.close()
    g = fresh()
    c0 = cost(g)
    t_full, (_, s) = B.wall_s(lambda: solve.levenberg_marquardt_device(g, a.iterations))
    c_full = cost(g)
    g.close()
    g = fresh()
    t_sweep, sweep = B.wall_s(lambda: solve.solve_windows(g, a.size, sweeps=1, halo=True, iterations=a.iterations))
    c_sweep = cost(g)
    g.close()
    result = dict(bench="window", blocks=a.blocks, n_cam=n_cam, n_pts=n_pts, n_obs=n_obs, repeats=a.repeats, extraction=extraction,
                  lm_iterations=a.iterations, start_cost=c0,
                  full_lm=dict(wall_s=round(t_full, 4), cost=c_full, iterations=s["iterations"]),
                  window_sweep=dict(size=a.size, windows=len(sweep), wall_s=round(t_sweep, 4), cost=c_sweep,
                                    child_cameras=[w["cameras"] for w in sweep], child_observations=[w["observations"] for w in sweep]))
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
