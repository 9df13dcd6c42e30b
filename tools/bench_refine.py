#!/usr/bin/env python3
"""Kernel time of per-point refinement (c2b_refine_points_rows: k_refine_points) on a noisy synthetic grid at rounds = 1, 5 and
10, against k_normal_points through c2b_normal_points_rows on the same problem in the same process: a launch of `rounds`
rounds walks every point's list rounds + 1 times, each walk k_normal_points' walk plus the cost, so (rounds + 1) point
passes is the structural expectation.  All are timed with device events around `--launches` back-to-back launches,
alternating, after a warm-up; the median over `--repeats` windows is reported.  The points are restored before every
refinement launch is queued (a device copy inside the window, timed alone and subtracted), so every launch starts from the
noisy points.

Then the Levenberg-Marquardt loop on tools/bench_lm.py's noisy grid with inner_iterations = 0, 1 and 2: the cost after every
iteration, the wall time of `--iterations` iterations, and the wall time to the cost the plain loop reaches in
`--iterations` iterations (a fresh run of as many iterations as that takes; null when the cost is not reached).
Prints one JSON line.

    python tools/bench_refine.py [--blocks 128] [--repeats 7] [--out profiles/refine_bench_blocks128.json]
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
    ap.add_argument("--point-std", type=float, default=1e-2, help="noise on the points the pass starts from")
    ap.add_argument("--lam", type=float, default=1e-4)
    ap.add_argument("--launches", type=int, default=10, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="windows; the median is reported")
    ap.add_argument("--iterations", type=int, default=10, help="LM iterations of the inner-iteration runs")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L, device as D, noise as N, solve

    dev = torch.device("cuda", 0)
    ba = B.bench_grid(a.blocks)
    N.add_noise(ba, 0.0, 0.0, a.point_std, a.sigma, seed=3)
    sizes = ba._sizes()
    lm_start = (ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
    lv = B.level0(ba, point_rows=True)
    camblk, prows, start, uv = lv.camblk, lv.prows, lv.pts4, lv.uv
    pts4 = start.clone()
    status = torch.zeros(sizes[1], dtype=torch.uint8, device=dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    V = torch.empty((sizes[1], 3, 3), dtype=torch.float64, device=dev)
    gp = torch.empty((sizes[1], 3), dtype=torch.float64, device=dev)

    def window(fn):
        return B.window_us(fn, a.launches)

    def refine(rounds):
        def fn():
            pts4.copy_(start)
            D.refine_points_rows(camblk, pts4, prows, uv, status, counts, rounds=rounds, lam=a.lam)
        return fn
    fns = {"copy": lambda: pts4.copy_(start), "normal_points_rows": lambda: D.normal_points_rows(camblk, start, prows, uv, V, gp)}
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
    kernel = {"normal_points_rows": round(med["normal_points_rows"], 2), "points_copy": round(med["copy"], 2)}
    passes = {}
    for r in (1, 5, 10):
        k = "refine_rounds_%d" % r
        kernel[k] = round(med[k] - med["copy"], 2)
        passes[k] = round((med[k] - med["copy"]) / med["normal_points_rows"], 3)
    ba.close()

    # ---- the LM loop with inner iterations ----
    def fresh():
        return c2b.BAProblem.from_bal(*lm_start, device=0)

    def run(n_inner, iterations):
        g = fresh()
        dt, (h, s) = B.wall_s(lambda: solve.levenberg_marquardt_device(g, iterations, lam=a.lam, inner_iterations=n_inner))
        g.close()
        return dt, h, s
    run(2, 1)                                                # the first solve of a process pays for the kernels' load
    lm = {}
    target = None
    for n_inner in (0, 1, 2):
        dt, h, s = run(n_inner, a.iterations)
        after = [e["cost_trial"] if e["accepted"] else e["cost"] for e in h]
        if n_inner == 0:
            target = s["final_cost"]
        reach = next((k + 1 for k, c in enumerate(after) if c <= target), None)
        t_reach = None
        if reach is not None:
            t_reach = B.median([run(n_inner, reach)[0] for _ in range(3)])
        lm["inner_%d" % n_inner] = dict(wall_s=round(dt, 4), accepted="".join("A" if e["accepted"] else "R" for e in h), initial_cost=s["initial_cost"],
                                        cost_after_iteration=after, final_cost=s["final_cost"], iterations_to_plain_final_cost=reach,
                                        wall_s_to_plain_final_cost=None if t_reach is None else round(t_reach, 4),
                                        pcg_iterations=[e["pcg_iterations"] for e in h])
    result = dict(bench="refine_points", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], lam=a.lam, point_std=a.point_std,
                  counts=got, launches_per_window=a.launches, windows=a.repeats, kernel_us=kernel,
                  spread_us={k: B.spread(v, 2) for k, v in t.items()},
                  point_passes=passes, expected_point_passes={"refine_rounds_%d" % r: r + 1 for r in (1, 5, 10)},
                  lm_iterations=a.iterations, lm=lm)
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
