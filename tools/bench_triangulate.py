#!/usr/bin/env python3
"""Kernel time of triangulation's pass (c2b_triangulate_rows: k_triangulate_points) on a noisy synthetic grid against
k_normal_points through c2b_normal_points_rows on the same problem in the same process -- the same point-major walk over
the transpose with more arithmetic per observation, so it is the yardstick.  Both are timed with device events around
`--launches` back-to-back launches, alternating, after a warm-up; the median over `--repeats` windows is reported.  The
points are restored between windows, so every triangulation launch starts from the noisy points.  Prints one JSON line.

    python tools/bench_triangulate.py [--blocks 128] [--repeats 7] [--out profiles/triangulate_bench_blocks128.json]
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
    ap.add_argument("--point-std", type=float, default=0.5, help="noise on the points the pass starts from")
    ap.add_argument("--min-angle", type=float, default=1.0, help="degrees")
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="windows; the median is reported")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import numpy as np
    import torch
    import benchkit as B
    from city2ba_amd import _lib as L, device as D, noise as N

    dev = torch.device("cuda", 0)
    ba = B.bench_grid(a.blocks)
    N.add_noise(ba, 0.0, 0.0, a.point_std, a.sigma, seed=3)
    sizes = ba._sizes()
    lv = B.level0(ba, point_rows=True)
    camblk, prows, start, uv = lv.camblk, lv.prows, lv.pts4, lv.uv
    pts4 = start.clone()
    status = torch.zeros(sizes[1], dtype=torch.uint8, device=dev)
    counts = torch.zeros(5, dtype=torch.int64, device=dev)
    V = torch.empty((sizes[1], 3, 3), dtype=torch.float64, device=dev)
    gp = torch.empty((sizes[1], 3), dtype=torch.float64, device=dev)
    angle = float(np.deg2rad(a.min_angle))

    def window(fn):
        return B.window_us(fn, a.launches, before=lambda: pts4.copy_(start))

    # (the first launch of a window moves the points; the later ones walk the same rows from the triangulated points: the
    # pass reads no point, so its work does not depend on where the points are)
    tri = lambda: D.triangulate_rows(camblk, pts4, prows, uv, status, counts, angle)
    nrm = lambda: D.normal_points_rows(camblk, start, prows, uv, V, gp)
    for fn in (tri, nrm, tri, nrm):
        window(fn)
    t = dict(tri=[], nrm=[])
    for _ in range(a.repeats):
        t["tri"].append(window(tri))
        t["nrm"].append(window(nrm))
    got = dict(zip(L.TRI_STATUS, (int(v) for v in counts.cpu().numpy())))
    med = {k: B.median(v) for k, v in t.items()}
    result = dict(bench="triangulate_points", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], min_angle_deg=a.min_angle,
                  counts=got, launches_per_window=a.launches, windows=a.repeats,
                  kernel_us=dict(triangulate_rows=round(med["tri"], 2), normal_points_rows=round(med["nrm"], 2)),
                  spread_us=dict(triangulate_rows=B.spread(t["tri"], 2), normal_points_rows=B.spread(t["nrm"], 2)),
                  ratio_triangulate_over_normal_points=round(med["tri"] / med["nrm"], 4))
    ba.close()
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
