#!/usr/bin/env python3
"""Kernel time of consensus resection's pass (c2b_resect_consensus_rows: k_resect_consensus) on a noisy synthetic grid with
wrong matches (noise.add_incorrect_correspondences on the host) against plain resection (c2b_resect_rows: k_resect_cameras)
on the same problem in the same process -- the pass it replaces where the list holds wrong matches, so it is the
yardstick -- and against plain resection on the list filtered by the consensus pass's own inlier mask: the refit's work,
which is what splits the pass's time into hypotheses-and-scoring and refit.  Both are timed with device events around `--launches` back-to-back launches, alternating, after a warm-up; the
median over `--repeats` windows is reported.  The cameras are restored between windows.  Neither pass reads a pose, so its
work does not depend on where the cameras are.  Prints one JSON line.

    python tools/bench_resect_robust.py [--blocks 128] [--mismatch 0.05] [--repeats 7]
                                        [--out profiles/resect_robust_bench_blocks128.json]
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
    ap.add_argument("--rotation-std", type=float, default=0.1, help="noise on the rotations the passes start from")
    ap.add_argument("--translation-std", type=float, default=0.5, help="noise on the translations the passes start from")
    ap.add_argument("--mismatch", type=float, default=0.05, help="chance of a wrong match per observation")
    ap.add_argument("--max-error", type=float, default=1e-2)
    ap.add_argument("--min-inliers", type=int, default=6)
    ap.add_argument("--min-gap", type=float, default=1e-4)
    ap.add_argument("--max-hypotheses", type=int, default=64)
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
    clean = ba
    ba = N.add_incorrect_correspondences(clean, a.mismatch, seed=4)     # a new problem: the list is rewritten on the host
    clean.close()
    sizes = ba._sizes()
    lv = B.level0(ba)
    rows, pts4, pt_idx, uv = lv.rows, lv.pts4, lv.pt_idx, lv.uv
    start = torch.from_numpy(ba.cameras_bal()).to(dev)
    bal9 = start.clone()
    status = torch.zeros(sizes[0], dtype=torch.uint8, device=dev)
    hyp = torch.zeros(sizes[0], dtype=torch.int32, device=dev)
    n_inl = torch.zeros(sizes[0], dtype=torch.int32, device=dev)
    inlier = torch.zeros(max(sizes[2], 1), dtype=torch.uint8, device=dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    counts_plain = torch.zeros(5, dtype=torch.int64, device=dev)

    def window(fn):
        return B.window_us(fn, a.launches, before=lambda: bal9.copy_(start))

    rob = lambda: D.resect_consensus_rows(bal9, pts4, rows, pt_idx, uv, status, counts, a.max_error, a.min_inliers, a.min_gap, a.max_hypotheses,
                                          hyp=hyp, n_inl=n_inl, inlier=inlier)
    res = lambda: D.resect_rows(bal9, pts4, rows, pt_idx, uv, status, counts_plain, a.min_inliers, a.min_gap)
    for fn in (rob, res, rob, res):
        window(fn)
    t = dict(rob=[], res=[])
    for _ in range(a.repeats):
        t["rob"].append(window(rob))
        t["res"].append(window(res))
    window(rob)                                              # the outputs below are the consensus pass's
    # the refit alone: plain resection of the list the mask leaves (every camera's inliers, in row order)
    keep = inlier[:sizes[2]].bool()
    prefix = torch.zeros(sizes[2] + 1, dtype=torch.int64, device=dev)
    prefix[1:] = torch.cumsum(keep.to(torch.int64), 0)
    rows_f = D.Rows(prefix[rows.row_ptr].contiguous())
    pt_idx_f, uv_f = pt_idx[keep].contiguous(), uv.reshape(-1, 2)[keep].contiguous()
    counts_fit = torch.zeros(5, dtype=torch.int64, device=dev)
    fit = lambda: D.resect_rows(bal9, pts4, rows_f, pt_idx_f, uv_f, status, counts_fit, a.min_inliers, a.min_gap)
    window(fit)
    t["fit"] = [window(fit) for _ in range(a.repeats)]
    got_fit = dict(zip(L.RES_STATUS, (int(v) for v in counts_fit.cpu().numpy())))
    got = dict(zip(L.RES_CONSENSUS_STATUS, (int(v) for v in counts.cpu().numpy())))
    got_plain = dict(zip(L.RES_STATUS, (int(v) for v in counts_plain.cpu().numpy())))
    outliers = int((inlier[:sizes[2]] == 0).sum().item())
    med = {k: B.median(v) for k, v in t.items()}
    result = dict(bench="resect_cameras_robust", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2],
                  mean_row=round(sizes[2] / max(sizes[0], 1), 3), mismatch=a.mismatch, max_error=a.max_error, min_inliers=a.min_inliers,
                  min_gap=a.min_gap, max_hypotheses=a.max_hypotheses, counts=got, outliers=outliers, counts_plain=got_plain,
                  launches_per_window=a.launches, windows=a.repeats,
                  counts_filtered=got_fit, n_obs_filtered=rows_f.n_obs,
                  kernel_us=dict(resect_consensus_rows=round(med["rob"], 2), resect_rows=round(med["res"], 2),
                                 resect_rows_filtered=round(med["fit"], 2)),
                  spread_us=dict(resect_consensus_rows=B.spread(t["rob"], 2), resect_rows=B.spread(t["res"], 2),
                                 resect_rows_filtered=B.spread(t["fit"], 2)),
                  ratio_consensus_over_resect=round(med["rob"] / med["res"], 4),
                  refit_share_of_consensus=round(med["fit"] / med["rob"], 4))
    ba.close()
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
