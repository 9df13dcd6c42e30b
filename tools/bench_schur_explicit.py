#!/usr/bin/env python3
"""Time the damped Gauss-Newton step with the implicit or the explicit Schur complement on the synthetic grid and
print one JSON line.  tools/bench_schur.py's figures for the chosen setting -- solve_step with 0 iterations (under explicit: the
build of S is in it), with 25 iterations at rel_tol 0, one PCG iteration as the difference / 25, info_25 -- and, under
--schur explicit, what the option adds:
  * pattern_build_ms: the covisibility passes at Level 0 (host clock, once), n_edges, obs_per_edge, schur_bytes;
  * k_schur_y, k_schur_blocks (both kernels) and k_schur_spmv at Level 0 (HIP events) with their algorithmic bytes and
    fraction of 8 TB/s.
--to-tol adds the iterations and wall time of a solve to rel_tol 1e-2 and to 1e-4.  --points-per-block N builds the grid with N
points per block (synthetic_grid(10, N, ...)) in place of bench.py's 10, so that a list with many observations per edge can be
made.  tools/bench_schur.py itself is unchanged: its line for --blocks 128 is the yardstick of the implicit path.

    python tools/bench_schur_explicit.py [--blocks 128] [--points-per-block N] [--schur implicit|explicit]
                                         [--preconditioner block_jacobi|schur_jacobi] [--reps 5] [--warmup 1] [--to-tol]

Algorithmic bytes (each input read once, each output written once):
  Y pass:   n_obs x (4 cam_idx + 4 pt_idx + 16 uv + 216 Y) + n_pts x (32 point + 72 V) + n_cam x 192 record
  blocks:   n_obs x (4 pt_idx + 4 obs_of + 4 cam_of + 216 Y) + n_pts x 8 + n_cam x (16 + 2 x 648 S_diag) + n_edges x (4 + 648 S_off)
            (every Y read once: a lower bound, the walk re-reads the Y of a track's other observations through the caches)
  product:  (n_edges + n_cam) x 648 + n_edges x 4 + n_cam x (8 + 72 x + 72 y)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--points-per-block", type=int, default=10, help="points per block of the grid (default: bench.py's 10)")
    ap.add_argument("--schur", choices=["implicit", "explicit"], default="explicit")
    ap.add_argument("--preconditioner", choices=["block_jacobi", "schur_jacobi"], default="block_jacobi")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--to-tol", action="store_true", help="also time solves to rel_tol 1e-2 and 1e-4")
    ap.add_argument("--tol-max-iters", type=int, default=1000)
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    import benchkit as B
    from city2ba_amd import device as D
    from city2ba_amd import noise as N
    from city2ba_amd import synthetic as S
    dev = torch.device("cuda", 0)
    lam = 1e-4
    ba = S.synthetic_grid(10, a.points_per_block, a.blocks, 20.0, 1.0, 1.0, 1.0, 10.0, cull=False, mirror=False)
    N.add_noise(ba, 0.0, 0.0, 0.0, 1e-3, seed=20243)
    n_cam, n_pts, n = ba._sizes()
    f64 = dict(dtype=torch.float64, device=dev)
    frac = lambda b, us: round(B.frac_of_peak(b, us), 4)

    def events(fn):
        return B.us_record(B.each_us(fn, max(a.reps, 10), a.warmup + 2))

    def wall(fn):
        times = B.wall_ms(fn, a.reps, a.warmup)
        return {"median_ms": round(B.upper_median(times), 3), "min_ms": round(min(times), 3)}

    extra = {}
    if a.schur == "explicit":                                # the pattern and the three passes, alone, over the same state
        lv = B.level0(ba, point_rows=True)
        U, gc = torch.empty((n_cam, 9, 9), **f64), torch.empty((n_cam, 9), **f64)
        V, gp = torch.empty((n_pts, 3, 3), **f64), torch.empty((n_pts, 3), **f64)
        D.normal_cameras_rows(lv.camblk, lv.pts4, lv.rows, lv.pt_idx, lv.uv, U, gc)
        D.normal_points_rows(lv.camblk, lv.pts4, lv.prows, lv.uv, V, gp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g_ptr, g_nbr, _ = D.covisibility_rows(lv.rows, lv.pt_idx, lv.prows, 1)
        torch.cuda.synchronize()
        pattern_ms = (time.perf_counter() - t0) * 1e3
        n_edges = int(g_nbr.shape[0])
        cam_idx = D.expand_rows(lv.rows.row_ptr, n)
        Y, Sd, So = torch.empty((n, 3, 9), **f64), torch.empty((n_cam, 9, 9), **f64), torch.empty((max(n_edges, 1), 9, 9), **f64)
        x, y = torch.randn((n_cam, 9), **f64) * 1e-3, torch.empty((n_cam, 9), **f64)
        part = torch.empty(4 * ((n_cam + 3) // 4), **f64)
        D.schur_jacobi_blocks(lv.camblk, lv.pts4, lv.rows, lv.pt_idx, lv.uv, U, V, lam, Sd)
        us_y = events(lambda: D.schur_y_rows(lv.camblk, lv.pts4, cam_idx, lv.pt_idx, lv.uv, V, lam, Y))
        us_b = events(lambda: D.schur_blocks_rows(lv.rows, lv.pt_idx, lv.prows, g_ptr, g_nbr, Y, Sd, So))
        us_s = events(lambda: D.schur_spmv_rows(g_ptr, g_nbr, Sd, So, x, y, part))
        bytes_y = n * (4 + 4 + 16 + 216) + n_pts * (32 + 72) + n_cam * 192
        bytes_b = n * (4 + 4 + 4 + 216) + n_pts * 8 + n_cam * (16 + 2 * 648) + n_edges * (4 + 648)
        bytes_s = (n_edges + n_cam) * 648 + n_edges * 4 + n_cam * (8 + 72 + 72)
        extra = {"n_edges": n_edges, "obs_per_edge": round(n / max(n_edges, 1), 3), "pattern_build_ms": round(pattern_ms, 3),
                 "schur_y_pass": dict(us_y, algorithmic_bytes=bytes_y, frac_of_8TBs=frac(bytes_y, us_y["median_us"])),
                 "schur_blocks_pass": dict(us_b, algorithmic_bytes=bytes_b, frac_of_8TBs=frac(bytes_b, us_b["median_us"])),
                 "schur_spmv_pass": dict(us_s, algorithmic_bytes=bytes_s, frac_of_8TBs=frac(bytes_s, us_s["median_us"]))}
        del lv, U, gc, V, gp, g_ptr, g_nbr, cam_idx, Y, Sd, So, x, y, part
        torch.cuda.empty_cache()
        extra["schur_bytes"] = ba.schur_bytes()

    dc, dp = torch.empty((n_cam, 9), **f64), torch.empty((n_pts, 3), **f64)
    info = {}
    ba.set_preconditioner(a.preconditioner)
    ba.set_schur(a.schur)

    def solve(k):
        info[k] = ba.solve_step(lam, max_iters=k, rel_tol=0.0, out=(dc, dp))[2]

    s0 = wall(lambda: solve(0))
    s25 = wall(lambda: solve(25))
    to_tol = {}
    if a.to_tol:
        for tol in (1e-2, 1e-4):
            res = {}

            def solve_tol():
                res["info"] = ba.solve_step(lam, max_iters=a.tol_max_iters, rel_tol=tol, out=(dc, dp))[2]

            w = wall(solve_tol)
            to_tol["to_rel_tol_%g" % tol] = dict(w, iterations=res["info"]["iterations"], status=res["info"]["status"],
                                                 rel_residual=res["info"]["rel_residual"])
    out = {"blocks": a.blocks, "points_per_block": a.points_per_block, "schur": a.schur, "preconditioner": a.preconditioner,
           "n_obs": n, "n_cam": n_cam, "n_pts": n_pts, "lambda": lam, **extra,
           "solve_0_iterations": s0, "solve_25_iterations": s25,
           "pcg_iteration_ms": round((s25["median_ms"] - s0["median_ms"]) / 25.0, 3), **to_tol, "info_25": info[25]}
    ba.close()
    B.emit(out)


if __name__ == "__main__":
    main()
