#!/usr/bin/env python3
"""Wall time of BAProblem.align (on="both") and BAProblem.transform on the synthetic grid's entities against a second problem made
from it by drift + noise, and each device pass of the alignment alone (Level 0, device time between events) next to the statistics
pass (c2b_stats) timed in the same run on the same tables: bytes, fraction of 8 TB/s, ratio to the statistics pass.  Medians after
a warm-up, with the spread (min .. max).  Prints one JSON line.

    python tools/bench_align.py [--blocks 128] [--repeats 20] [--out profiles/align_bench_blocks128.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20, help="timed repeats after 5 warm-up calls; the median is reported")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import numpy as np
    import torch
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L, device as D, noise as N

    def grid():
        ba = c2b.BAProblem(0)
        L.check(L.lib().c2b_problem_synthetic_grid_layout(ba._h, 10, 10, a.blocks, 20.0, 1.0, 1.0, 1.0))
        return ba
    truth, est = grid(), grid()
    extent = 20.0 * a.blocks * 2.0 ** 0.5                      # add_drift moves by strength * distance^2 and turns by angle * distance^1.2:
    N.add_drift(est, 2.0 / extent ** 2, 0.02 / extent ** 1.2, 0.01, [1.0, 0.5, 0.0], seed=1)      # 2 units and 0.02 rad at the far corner
    N.add_noise(est, 1e-2, 1e-3, 1e-2, 0.0, seed=2)
    nc, np_, _ = truth._sizes()

    def spread(us):
        return dict(median_us=round(B.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2))

    def wall(fn):
        for _ in range(5):
            fn()
        return spread([B.wall_s(fn)[0] * 1e6 for _ in range(a.repeats)])
    c, s_ = np.cos(0.3), np.sin(0.3)
    Rb = np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])
    est.transform(1.5, Rb, [10.0, -5.0, 2.0])                  # another frame: what the alignment has to undo
    res = est.align(truth, on="both")
    t_align = wall(lambda: est.align(truth, on="both"))
    t_trim = wall(lambda: est.align(truth, on="both", max_dist=3.0 * res["points"]["rmse"], rounds=3))
    t_transform = wall(lambda: est.transform(1.0, Rb, [0.0, 0.0, 0.0]))

    # the passes alone, on tables of the same entities
    dev = "cuda:0"

    def rows4(x):
        t = torch.zeros((len(x), 4), dtype=torch.float64, device=dev)
        t[:, :3] = torch.from_numpy(x).to(dev)
        return t
    cx, cy = torch.from_numpy(est.cameras()).to(dev), torch.from_numpy(truth.cameras()).to(dev)
    xc, yc, xp, yp = rows4(est._camera_centers()), rows4(truth._camera_centers()), rows4(est.points()), rows4(truth.points())
    ws = D.workspace(0, dev)
    cen = D.centers_table(nc, dev)
    blk = D.cameras_prepare_state(cx, centers=cen)
    sim = L.similarity(res["scale"], res["rotation"], res["translation"])
    means = D.align_means_rows(ws, xc, yc, None, xp, yp, None)
    err_c, err_p = torch.empty(nc, dtype=torch.float64, device=dev), torch.empty(np_, dtype=torch.float64, device=dev)
    cam_w, pts_w = cx.clone(), xp.clone()
    row = 2 * 32
    passes = {
        "stats": (lambda: D.stats(blk, xp, ws, centers=cen), (nc + np_) * 32),
        "means": (lambda: D.align_means_rows(ws, xc, yc, None, xp, yp, None), (nc + np_) * row),
        "moments": (lambda: D.align_moments_rows(ws, means, xc, yc, None, xp, yp, None), (nc + np_) * row),
        "errors_cameras": (lambda: D.align_errors_rows(ws, xc, yc, sim, err=err_c), nc * (row + 8)),
        "errors_points": (lambda: D.align_errors_rows(ws, xp, yp, sim, err=err_p), np_ * (row + 8)),
        "rotation_errors": (lambda: D.align_rotation_errors_rows(ws, cx, cy, sim, err=err_c), nc * (2 * 120 + 8)),
        "apply": (lambda: D.similarity_apply(cam_w, pts_w, L.similarity(1.0, Rb, [0.0, 0.0, 0.0])), nc * 2 * 96 + np_ * 2 * 24),
    }
    timed = {}
    for name, (fn, nbytes) in passes.items():
        timed[name] = dict(spread(B.each_us(fn, a.repeats, 5)), bytes=int(nbytes))
        timed[name]["fraction_of_8TBs"] = round(B.frac_of_peak(nbytes, timed[name]["median_us"]), 3)
    for name in timed:
        timed[name]["ratio_to_stats"] = round(timed[name]["median_us"] / timed["stats"]["median_us"], 2)
    result = dict(bench="align", blocks=a.blocks, n_cam=nc, n_pts=np_, repeats=a.repeats, status=res["status"], scale=res["scale"],
                  camera_rmse=res["cameras"]["rmse"], point_rmse=res["points"]["rmse"], align_both_wall=t_align, align_both_trim3_wall=t_trim,
                  transform_wall=t_transform, passes=timed)
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
