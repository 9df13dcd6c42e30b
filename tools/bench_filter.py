#!/usr/bin/env python3
"""Wall time of BAProblem.filter_observations (mask, compaction and swap on the device) against the route it replaces --
download project() and observations(), filter in numpy, re-upload the whole problem through BAProblem.from_visibility -- on
the same noisy synthetic grid with wrong matches in the same process, each followed by the solve_step that rebuilds what
the new list needs.  Both routes must leave the same lists.  Prints one JSON line.

    python tools/bench_filter.py [--blocks 128] [--repeats 3] [--out profiles/filter_observations_bench_blocks128.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--sigma", type=float, default=1e-3, help="observation noise")
    ap.add_argument("--mismatch", type=float, default=0.05, help="chance of a wrong match per observation")
    ap.add_argument("--repeats", type=int, default=3, help="the median is reported")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import numpy as np
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import noise as N

    g = B.bench_grid(a.blocks)
    N.add_noise(g, 0.0, 0.0, 0.0, a.sigma, seed=3)
    bad = N.add_incorrect_correspondences(g, a.mismatch, seed=1)
    g.close()
    start = (bad.cameras(), bad.points(), bad.row_ptr.copy(), bad.pt_idx.copy(), bad.observations())
    sizes = bad._sizes()
    bad.close()
    max_error = 10.0 * a.sigma

    def fresh():
        ba = c2b.BAProblem.from_visibility(*start, device=0)
        ba.solve_step(1e-2)                                  # the caches a filter has to drop exist
        return ba

    def host_route(ba):
        proj, uv = ba.project().reshape(-1, 2), ba.observations().reshape(-1, 2)
        du, dv = proj[:, 0] - uv[:, 0], proj[:, 1] - uv[:, 1]
        keep = du * du + dv * dv <= max_error * max_error
        rows = ba.row_ptr.astype(np.int64)
        cam = np.repeat(np.arange(len(rows) - 1), np.diff(rows))
        new_rows = np.concatenate([[0], np.cumsum(np.bincount(cam[keep], minlength=len(rows) - 1))]).astype(np.uint64)
        return c2b.BAProblem.from_visibility(ba.cameras(), ba.points(), new_rows, ba.pt_idx[keep], uv[keep], device=0)

    warm = fresh()                                           # the first call of a process pays for the kernels' load
    warm.filter_observations(max_error)
    warm.close()
    t = dict(device=[], step_after_device=[], host=[], step_after_host=[])
    same, removed = True, 0
    for _ in range(a.repeats):
        ba = fresh()
        dt, removed = B.wall_s(lambda: ba.filter_observations(max_error))
        t["device"].append(dt)
        t["step_after_device"].append(B.wall_s(lambda: ba.solve_step(1e-2))[0])
        src = fresh()
        dt, twin = B.wall_s(lambda: host_route(src))
        t["host"].append(dt)
        t["step_after_host"].append(B.wall_s(lambda: twin.solve_step(1e-2))[0])
        same = same and ba.row_ptr.tobytes() == twin.row_ptr.tobytes() and ba.pt_idx.tobytes() == twin.pt_idx.tobytes() and \
            ba.observations().tobytes() == twin.observations().tobytes()
        for p in (ba, src, twin):
            p.close()
    med = {k: round(B.median(v) * 1e3, 3) for k, v in t.items()}
    result = dict(bench="filter_observations", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], removed=int(removed),
                  max_error=max_error, filter_ms=dict(device=med["device"], host_round_trip=med["host"]),
                  step_after_ms=dict(device=med["step_after_device"], host_round_trip=med["step_after_host"]), same_lists=bool(same))
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
