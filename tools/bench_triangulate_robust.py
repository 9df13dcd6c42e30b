#!/usr/bin/env python3
"""Kernel time of consensus triangulation's pass (c2b_triangulate_consensus_rows: k_triangulate_consensus) on a noisy
synthetic grid with wrong matches (noise.add_incorrect_correspondences on the host) against plain triangulation
(c2b_triangulate_rows: k_triangulate_points) on the same problem in the same process -- the pass it replaces where the list
holds wrong matches, so it is the yardstick.  Both are timed with device events around `--launches` back-to-back launches,
alternating, after a warm-up; the median over `--repeats` windows is reported.  The points are restored between windows.
Neither pass reads a point, so its work does not depend on where the points are.  Prints one JSON line.

    python tools/bench_triangulate_robust.py [--blocks 128] [--mismatch 0.05] [--repeats 7]
                                             [--out profiles/triangulate_robust_bench_blocks128.json]
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
    ap.add_argument("--point-std", type=float, default=0.5, help="noise on the points the passes start from")
    ap.add_argument("--mismatch", type=float, default=0.05, help="chance of a wrong match per observation")
    ap.add_argument("--min-angle", type=float, default=1.0, help="degrees")
    ap.add_argument("--max-error", type=float, default=1e-2)
    ap.add_argument("--min-inliers", type=int, default=3)
    ap.add_argument("--max-hypotheses", type=int, default=64)
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
    clean = ba
    ba = N.add_incorrect_correspondences(clean, a.mismatch, seed=4)     # a new problem: the list is rewritten on the host
    clean.close()
    sizes = ba._sizes()
    lv = B.level0(ba, point_rows=True)
    camblk, prows, start, uv = lv.camblk, lv.prows, lv.pts4, lv.uv
    pts4 = start.clone()
    status = torch.zeros(sizes[1], dtype=torch.uint8, device=dev)
    hyp = torch.zeros(sizes[1], dtype=torch.int32, device=dev)
    n_inl = torch.zeros(sizes[1], dtype=torch.int32, device=dev)
    inlier = torch.zeros(max(sizes[2], 1), dtype=torch.uint8, device=dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    counts_plain = torch.zeros(5, dtype=torch.int64, device=dev)
    angle = float(np.deg2rad(a.min_angle))

    def window(fn):
        return B.window_us(fn, a.launches, before=lambda: pts4.copy_(start))

    rob = lambda: D.triangulate_consensus_rows(camblk, pts4, prows, uv, status, counts, angle, a.max_error, a.min_inliers, a.max_hypotheses,
                                               hyp=hyp, n_inl=n_inl, inlier=inlier)
    tri = lambda: D.triangulate_rows(camblk, pts4, prows, uv, status, counts_plain, angle)
    for fn in (rob, tri, rob, tri):
        window(fn)
    t = dict(rob=[], tri=[])
    for _ in range(a.repeats):
        t["rob"].append(window(rob))
        t["tri"].append(window(tri))
    window(rob)                                              # the outputs below are the consensus pass's
    got = dict(zip(L.TRI_CONSENSUS_STATUS, (int(v) for v in counts.cpu().numpy())))
    got_plain = dict(zip(L.TRI_STATUS, (int(v) for v in counts_plain.cpu().numpy())))
    outliers = int((inlier[:sizes[2]] == 0).sum().item())
    med = {k: B.median(v) for k, v in t.items()}
    result = dict(bench="triangulate_points_robust", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2],
                  mean_row=round(sizes[2] / max(sizes[1], 1), 3), mismatch=a.mismatch, min_angle_deg=a.min_angle, max_error=a.max_error,
                  min_inliers=a.min_inliers, max_hypotheses=a.max_hypotheses, counts=got, outliers=outliers, counts_plain=got_plain,
                  launches_per_window=a.launches, windows=a.repeats,
                  kernel_us=dict(triangulate_consensus_rows=round(med["rob"], 2), triangulate_rows=round(med["tri"], 2)),
                  spread_us=dict(triangulate_consensus_rows=B.spread(t["rob"], 2), triangulate_rows=B.spread(t["tri"], 2)),
                  ratio_consensus_over_triangulate=round(med["rob"] / med["tri"], 4))
    ba.close()
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
