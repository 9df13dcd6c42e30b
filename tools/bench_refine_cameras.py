#!/usr/bin/env python3
"""Kernel time of per-camera refinement (c2b_refine_cameras_rows: k_refine_cameras) on a noisy synthetic grid at rounds = 1, 5
and 10, against k_normal_cameras through c2b_normal_cameras_rows on the same problem in the same process: a launch of `rounds`
rounds walks every camera's row rounds + 1 times, each walk k_normal_cameras' walk plus the cost, and between the walks runs
the dense part (the record from bal9, the 9x9 factor and solve, the model) -- so (rounds + 1) camera passes plus the dense part
is the structural expectation, reported as a ratio to one k_normal_cameras launch; marginal_in_camera_passes holds the cost
of an added round (the slope from 1 to 10 rounds), the dense part of a round (that less its one walk) and the launch's fixed
part.  All are timed with device events around `--launches` back-to-back launches, alternating, after a warm-up; the median
over `--repeats` windows is reported.  bal9 is
restored before every refinement launch is queued (a device copy inside the window, timed alone and subtracted), so every
launch starts from the noisy cameras.  Prints one JSON line.

    python tools/bench_refine_cameras.py [--blocks 128] [--repeats 7] [--out profiles/refine_cameras_bench_blocks128.json]
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
    ap.add_argument("--translation-std", type=float, default=1e-2, help="noise on the camera translations the pass starts from")
    ap.add_argument("--rotation-std", type=float, default=1e-3, help="noise on the camera rotations the pass starts from")
    ap.add_argument("--lam", type=float, default=1e-4)
    ap.add_argument("--launches", type=int, default=10, help="launches per timed window")
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
    start = torch.from_numpy(ba.cameras_bal()).to(dev)
    lv = B.level0(ba)
    rows, pts4, pt_idx, uv = lv.rows, lv.pts4, lv.pt_idx, lv.uv
    camblk = D.cameras_prepare_bal(start)                    # the table of the cameras the refinement starts from, as it reads them
    bal9 = start.clone()
    status = torch.zeros(sizes[0], dtype=torch.uint8, device=dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    U = torch.empty((sizes[0], 9, 9), dtype=torch.float64, device=dev)
    gc = torch.empty((sizes[0], 9), dtype=torch.float64, device=dev)

    def window(fn):
        return B.window_us(fn, a.launches)

    def refine(rounds):
        def fn():
            bal9.copy_(start)
            D.refine_cameras_rows(bal9, pts4, rows, pt_idx, uv, status, counts, rounds=rounds, lam=a.lam)
        return fn
    fns = {"copy": lambda: bal9.copy_(start), "normal_cameras_rows": lambda: D.normal_cameras_rows(camblk, pts4, rows, pt_idx, uv, U, gc)}
    fns.update({"refine_rounds_%d" % r: refine(r) for r in (1, 5, 10)})
    for fn in list(fns.values()) * 2:
        window(fn)
    t = {k: [] for k in fns}
    got = {}
    for _ in range(a.repeats):
        for k, fn in fns.items():
            t[k].append(window(fn))
            if k.startswith("refine"):
                got[k] = dict(zip(L.REFINE_COUNTS, (int(v) for v in counts.cpu().numpy())))
    med = {k: B.median(v) for k, v in t.items()}
    kernel = {"normal_cameras_rows": round(med["normal_cameras_rows"], 2), "bal9_copy": round(med["copy"], 2)}
    passes = {}
    for r in (1, 5, 10):
        k = "refine_rounds_%d" % r
        kernel[k] = round(med[k] - med["copy"], 2)
        passes[k] = round((med[k] - med["copy"]) / med["normal_cameras_rows"], 3)
    ba.close()
    # in camera passes: what an added round costs (the slope from 1 to 10 rounds), the dense part of a round (that less its one
    # walk), and what a launch costs on top of rounds x that (its fixed part: walk 0 with its record among it)
    per_round = (passes["refine_rounds_10"] - passes["refine_rounds_1"]) / 9.0
    marginal = dict(added_round=round(per_round, 3), dense_part_of_a_round=round(per_round - 1.0, 3),
                    fixed_part_of_a_launch=round(passes["refine_rounds_1"] - per_round, 3))
    result = dict(bench="refine_cameras", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], lam=a.lam,
                  translation_std=a.translation_std, rotation_std=a.rotation_std, counts=got, launches_per_window=a.launches, windows=a.repeats,
                  kernel_us=kernel, spread_us={k: B.spread(v, 2) for k, v in t.items()}, camera_passes=passes,
                  expected_camera_passes={"refine_rounds_%d" % r: r + 1 for r in (1, 5, 10)}, marginal_in_camera_passes=marginal)
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
