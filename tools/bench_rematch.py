#!/usr/bin/env python3
"""Time of guided re-matching on a synthetic grid after the host join_landmarks and
add_incorrect_correspondences: the choose pass (c2b_rematch_rows: the extent, its cell list, k_rematch_choose and
k_rematch_resolve -- the entry synchronises, so it is timed by the wall clock around the call), one whole
BAProblem.rematch_observations call on a freshly loaded problem (the filter's mask, the transpose, the trusted points, the
choose pass, apply, compaction and installation), and as the yardstick c2b_merge_partner_rows on the same problem in the same
process.  --radius 0 takes the 90th percentile of the distance to the tenth nearest neighbour over a sample of 2 000 points
(join_landmarks hands out one of the ten nearest).  The median over `--repeats` is reported.  Prints one JSON line.

    python tools/bench_rematch.py [--blocks 128] [--join 0.05] [--mismatch 0.05] [--radius 0] [--max-error 1e-3] [--min-fits 2]
                                  [--repeats 5] [--out profiles/rematch_bench_blocks128.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--join", type=float, default=0.05, help="join_landmarks' fraction")
    ap.add_argument("--mismatch", type=float, default=0.05, help="add_incorrect_correspondences' chance")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.0)
    ap.add_argument("--max-error", type=float, default=1e-3)
    ap.add_argument("--min-fits", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import numpy as np
    import torch
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L, device as D, noise as N

    dev = torch.device("cuda", 0)
    whole = B.bench_grid(a.blocks)
    true_idx = whole.pt_idx.copy()
    joined = N.join_landmarks(whole, a.join, seed=a.seed)        # new problems: the list is rewritten on the host
    whole.close()
    ba = N.add_incorrect_correspondences(joined, a.mismatch, seed=a.seed + 1)
    joined.close()
    sizes = ba._sizes()
    wrong = ba.pt_idx != true_idx
    host = (ba.cameras(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations().reshape(-1, 2).copy())
    lv = B.level0(ba, point_rows=True)
    camblk, rows, prows, pts4, pt_idx, uv = lv.camblk, lv.rows, lv.prows, lv.pts4, lv.pt_idx, lv.uv
    radius = a.radius
    if radius <= 0.0:
        pick = torch.from_numpy(np.random.default_rng(a.seed).choice(sizes[1], size=min(2000, sizes[1]), replace=False)).to(dev)
        xyz = pts4[:, :3]
        tenth = torch.cat([torch.cdist(xyz[pick[k:k + 250]], xyz).kthvalue(min(11, sizes[1]), dim=1).values for k in range(0, len(pick), 250)])
        radius = float(torch.quantile(tenth, 0.9).item())       # (the nearest of all is the point itself)
    fits = torch.zeros(sizes[2], dtype=torch.uint8, device=dev)
    choice = torch.zeros(sizes[2], dtype=torch.int32, device=dev)
    status = torch.zeros(sizes[2], dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    partner = torch.zeros(sizes[1], dtype=torch.int32, device=dev)
    pstatus = torch.zeros(sizes[1], dtype=torch.uint8, device=dev)
    pcounts = torch.zeros(4, dtype=torch.int64, device=dev)
    D.residual_keep_rows(camblk, pts4, rows, pt_idx, uv, a.max_error, fits, in_front=True)
    # rule 2 with the pieces Level 0 exposes: the fitting observations per point
    nfit = torch.zeros(sizes[1], dtype=torch.int64, device=dev).index_add_(0, pt_idx.long(), fits.long())
    trusted = ((nfit >= a.min_fits) & torch.isfinite(pts4[:, :3]).all(dim=1)).to(torch.uint8)

    def choose_pass():
        return B.wall_s(lambda: D.rematch_rows(camblk, pts4, rows, pt_idx, uv, fits, choice, status, counts, radius, a.max_error,
                                               pt_trusted=trusted))[0] * 1e6

    def partner_pass():
        return B.wall_s(lambda: D.merge_partner_rows(camblk, pts4, prows, uv, partner, pstatus, pcounts, radius, a.max_error))[0] * 1e6

    def whole_call():
        fresh = c2b.BAProblem.from_visibility(*host, device=0)
        fresh.total_reprojection_error(2.0)                      # the cameras' records and the row structure exist, as in a pipeline
        dt, out = B.wall_s(lambda: fresh.rematch_observations(radius, a.max_error, min_fits=a.min_fits))
        fresh.close()
        return dt * 1e6, out

    choose_pass(), partner_pass()                                # warm-up
    t = dict(choose=[], partner=[], call=[])
    out = None
    for _ in range(a.repeats):
        t["choose"].append(choose_pass())
        t["partner"].append(partner_pass())
        dt, out = whole_call()
        t["call"].append(dt)
    got = dict(zip(L.REMATCH_STATUS, (int(v) for v in counts.cpu().numpy())))
    st, ch = status.cpu().numpy(), choice.cpu().numpy()
    back = int(((st == L.REMATCH_REASSIGNED) & (ch == true_idx.astype(np.int64))).sum())
    med = {k: B.median(v) for k, v in t.items()}
    names = (("rematch_rows", "choose"), ("rematch_observations_call", "call"), ("merge_partner_rows", "partner"))
    result = dict(bench="rematch_observations", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], join=a.join, mismatch=a.mismatch,
                  wrong_labels=int(wrong.sum()), radius=round(radius, 6), max_error=a.max_error, min_fits=a.min_fits, level0_status=got,
                  level1_status=out, reassigned_to_truth=back, right_observations_changed=int((~wrong & (st >= L.REMATCH_REASSIGNED)).sum()),
                  repeats=a.repeats, time_us={k: round(med[v], 1) for k, v in names},
                  spread_us={k: B.spread(t[v], 1) for k, v in names})
    ba.close()
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
