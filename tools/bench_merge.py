#!/usr/bin/env python3
"""Time of landmark merging on a synthetic grid after the host split_landmarks: the partner pass alone
(c2b_merge_partner_rows: the extent, its cell list and k_merge_partner -- the entry synchronises, so it is timed by the wall
clock around the call), one whole BAProblem.merge_points call on a freshly loaded problem (transpose, partner pass, apply,
remap, per round), and the rebuild of the point-major transpose alone (c2b_normal_transpose, device events), which every
round after a merge pays.  The median over `--repeats` is reported.  Prints one JSON line.

    python tools/bench_merge.py [--blocks 128] [--split 0.1] [--radius 0.5] [--max-error 1e-4] [--rounds 2] [--repeats 5]
                                [--out profiles/merge_bench_blocks128.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--split", type=float, default=0.1, help="fraction of the landmarks split on the host")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--max-error", type=float, default=1e-4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L, device as D, noise as N

    dev = torch.device("cuda", 0)
    whole = B.bench_grid(a.blocks)
    n_before = whole._sizes()[1]
    ba = N.split_landmarks(whole, a.split, seed=a.seed)          # a new problem: the list is rewritten on the host
    whole.close()
    sizes = ba._sizes()
    host = (ba.cameras(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations().reshape(-1, 2).copy())
    lv = B.level0(ba, point_rows=True)
    partner = torch.zeros(sizes[1], dtype=torch.int32, device=dev)
    status = torch.zeros(sizes[1], dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)

    def partner_pass():
        return B.wall_s(lambda: D.merge_partner_rows(lv.camblk, lv.pts4, lv.prows, lv.uv, partner, status, counts, a.radius, a.max_error))[0] * 1e6

    def transpose():
        return B.each_us(lambda: D.PointRows(lv.rows, lv.pt_idx, sizes[1]), 1, 0)[0]

    def whole_call():
        fresh = c2b.BAProblem.from_visibility(*host, device=0)
        fresh.total_reprojection_error(2.0)                      # the cameras' records and the row structure exist, as in a pipeline
        dt, out = B.wall_s(lambda: fresh.merge_points(a.radius, a.max_error, rounds=a.rounds))
        fresh.close()
        return dt * 1e6, out

    partner_pass(), transpose()                                  # warm-up
    t = dict(partner=[], transpose=[], call=[])
    out = None
    for _ in range(a.repeats):
        t["partner"].append(partner_pass())
        t["transpose"].append(transpose())
        dt, out = whole_call()
        t["call"].append(dt)
    got = dict(zip(L.MERGE_STATUS, (int(v) for v in counts.cpu().numpy())))
    med = {k: B.median(v) for k, v in t.items()}
    result = dict(bench="merge_points", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_pts_before_split=n_before, n_obs=sizes[2],
                  split=a.split, radius=a.radius, max_error=a.max_error, rounds=a.rounds, first_round_status=got, merged=out["merged"],
                  rounds_run=out["rounds"], repeats=a.repeats,
                  time_us=dict(merge_partner_rows=round(med["partner"], 1), merge_points_call=round(med["call"], 1),
                               normal_transpose=round(med["transpose"], 1)),
                  spread_us={k: B.spread(v, 1) for k, v in
                             (("merge_partner_rows", t["partner"]), ("merge_points_call", t["call"]), ("normal_transpose", t["transpose"]))})
    ba.close()
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
