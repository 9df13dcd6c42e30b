#!/usr/bin/env python3
"""Time the Gauss-Newton diagonal blocks' Level-0 passes on `synthetic --blocks B` (default 128, the flagship size) with
HIP events and print one JSON line: the transpose (built once per observation list), the camera pass (U, gc and the
folded sum of squares), the point pass (V, gp), their algorithmic bytes and fraction of 8 TB/s, and the step launch
(residual + Jacobian into plain arrays) for scale.

    python tools/bench_normal.py [--blocks 128] [--reps 20] [--warmup 3]

Algorithmic bytes (each input read once, each output written once):
  camera pass: n_obs x (4 pt_idx + 16 uv) + n_pts x 32 + n_cam x (8 row_ptr + 192 camera record + 648 U + 72 gc)
  point pass:  n_obs x (4 obs_of + 4 cam_of + 16 uv) + n_pts x (8 pt_row_ptr + 32 point + 72 V + 24 gp) + n_cam x 192
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    import bench
    import benchkit as B
    from city2ba_amd import device as D
    dev = torch.device("cuda", 0)
    sh = bench.build_shard(argparse.Namespace(blocks=a.blocks), 0, 1, dev)
    n, rows, pts4, pi, uv, camblk = sh["n_obs"], sh["rows"], sh["pts4"], sh["pt_idx"], sh["uv"], sh["camblk"]
    n_cam, n_pts = rows.n_cam, pts4.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    U, gc = torch.empty((n_cam, 9, 9), **f64), torch.empty((n_cam, 9), **f64)
    V, gp = torch.empty((n_pts, 3, 3), **f64), torch.empty((n_pts, 3), **f64)
    ws = D.workspace(n, dev)
    s = torch.zeros(1, **f64)
    r, Jc, Jp = torch.empty((n, 2), **f64), torch.empty((n, 18), **f64), torch.empty((n, 6), **f64)
    pr = [None]

    def transpose():
        pr[0] = D.PointRows(rows, pi, n_pts)

    runs = {
        "transpose": transpose,
        "cameras": lambda: D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U, gc, ws, s),
        "points": lambda: D.normal_points_rows(camblk, pts4, pr[0], uv, V, gp),
        "step": lambda: D.residual_jacobian_rows(camblk, pts4, rows, pi, uv, r, Jc, Jp, 2.0, ws, s),
    }
    us = {name: B.us_record(B.each_us(fn, a.reps, a.warmup)) for name, fn in runs.items()}
    bytes_c = n * 20 + n_pts * 32 + n_cam * (8 + 192 + 648 + 72)
    bytes_p = n * 24 + n_pts * (8 + 32 + 72 + 24) + n_cam * 192
    both = us["cameras"]["median_us"] + us["points"]["median_us"]
    out = {
        "blocks": a.blocks, "n_obs": n, "n_cam": n_cam, "n_pts": n_pts,
        "transpose": us["transpose"],
        "cameras": dict(us["cameras"], algorithmic_bytes=bytes_c, frac_of_8TBs=round(B.frac_of_peak(bytes_c, us["cameras"]["median_us"]), 4)),
        "points": dict(us["points"], algorithmic_bytes=bytes_p, frac_of_8TBs=round(B.frac_of_peak(bytes_p, us["points"]["median_us"]), 4)),
        "both_passes_us": round(both, 1),
        "both_frac_of_8TBs": round(B.frac_of_peak(bytes_c + bytes_p, both), 4),
        "step_us": us["step"],
        "both_over_step": round(both / us["step"]["median_us"], 3),
    }
    B.emit(out)


if __name__ == "__main__":
    main()
