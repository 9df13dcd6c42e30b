#!/usr/bin/env python3
"""Kernel time of resection's pass (c2b_resect_rows: k_resect_cameras) on a noisy synthetic grid against k_normal_cameras
through c2b_normal_cameras_rows on the same problem in the same process -- the same camera-major walk over the same rows,
so it is the yardstick.  Both are timed with device events around `--launches` back-to-back launches, alternating, after a
warm-up; the median over `--repeats` windows is reported.  The cameras are restored between windows, so every window's
first resection starts from the noisy poses (the pass reads no pose, so its work does not depend on where they are).
Prints one JSON line.

    python tools/bench_resect.py [--blocks 128] [--repeats 7] [--out profiles/resect_bench_blocks128.json]
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
    ap.add_argument("--rotation-std", type=float, default=0.1, help="noise on the rotations the pass starts from")
    ap.add_argument("--translation-std", type=float, default=0.5, help="noise on the translations the pass starts from")
    ap.add_argument("--min-points", type=int, default=6)
    ap.add_argument("--min-gap", type=float, default=1e-4)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="windows; the median is reported")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    import benchkit as B
    from city2ba_amd import _lib as L, device as D, noise as N

    dev = torch.device("cuda", 0)
    ba = B.bench_grid(a.blocks)
    N.add_noise(ba, a.translation_std, a.rotation_std, 0.0, a.sigma, seed=3)
    sizes = ba._sizes()
    lv = B.level0(ba)
    camblk, rows, pts4, pt_idx, uv = lv.camblk, lv.rows, lv.pts4, lv.pt_idx, lv.uv
    start = torch.from_numpy(ba.cameras_bal()).to(dev)
    bal9 = start.clone()
    status = torch.zeros(sizes[0], dtype=torch.uint8, device=dev)
    counts = torch.zeros(5, dtype=torch.int64, device=dev)
    U = torch.empty((sizes[0], 9, 9), dtype=torch.float64, device=dev)
    gc = torch.empty((sizes[0], 9), dtype=torch.float64, device=dev)

    def window(fn):
        return B.window_us(fn, a.launches, before=lambda: bal9.copy_(start))

    res = lambda: D.resect_rows(bal9, pts4, rows, pt_idx, uv, status, counts, a.min_points, a.min_gap)
    nrm = lambda: D.normal_cameras_rows(camblk, pts4, rows, pt_idx, uv, U, gc)
    for fn in (res, nrm, res, nrm):
        window(fn)
    t = dict(res=[], nrm=[])
    for _ in range(a.repeats):
        t["res"].append(window(res))
        t["nrm"].append(window(nrm))
    got = dict(zip(L.RES_STATUS, (int(v) for v in counts.cpu().numpy())))
    med = {k: B.median(v) for k, v in t.items()}
    result = dict(bench="resect_cameras", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], min_points=a.min_points,
                  min_gap=a.min_gap, counts=got, launches_per_window=a.launches, windows=a.repeats,
                  kernel_us=dict(resect_rows=round(med["res"], 2), normal_cameras_rows=round(med["nrm"], 2)),
                  spread_us=dict(resect_rows=B.spread(t["res"], 2), normal_cameras_rows=B.spread(t["nrm"], 2)),
                  ratio_resect_over_normal_cameras=round(med["res"] / med["nrm"], 4))
    ba.close()
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
