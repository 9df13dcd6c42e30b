#!/usr/bin/env python3
"""Time the damped Gauss-Newton step on `synthetic --blocks B` (default 128, the flagship size; observation noise 1e-3)
and print one JSON line:
  * the two Schur passes at Level 0 (HIP events), with their algorithmic bytes and fraction of 8 TB/s;
  * solve_step with 0 iterations -- the set-up (the normal-equation passes, the 9x9 factorisations, b) plus the
    back-substitution and the model-decrease pass, i.e. everything but PCG;
  * solve_step with 25 iterations and rel_tol = 0 (a fixed-count solve), and one PCG iteration as the difference / 25;
  * apply_step, and under --loss robust_cost() (the LM loop's accept test: one projection per observation).
The Level-1 calls are synchronous and timed on the host clock; each figure is the median of --reps after --warmup.

    python tools/bench_schur.py [--blocks 128] [--reps 5] [--warmup 1] [--loss huber|cauchy|soft_l1 --loss-scale A]
                                [--preconditioner block_jacobi|schur_jacobi] [--to-tol]
                                [--constant none|intrinsics|gauge|points]

--preconditioner schur_jacobi (combinable with --loss) solves with the Schur-Jacobi blocks and also reports
the pass that forms them alone (k_schur_jacobi: us, algorithmic bytes, fraction of 8 TB/s).  --to-tol adds, for either
preconditioner, the iterations and wall time of a solve to rel_tol 1e-2 and to 1e-4 (max_iters --tol-max-iters; a
solve that ends with status 1 is reported as such).

--constant reports the same rows for a solve with constant parameters (BAProblem.set_constant): intrinsics
= f, k1, k2 of every camera; gauge = camera 0 wholly and t0 of camera 1; points = every point.  none, the default, sets
no mask: the run is the one it was before the option existed.  The Level-0 passes are timed without the mask.

--loss times the same figures under a robust loss (the weighted kernels); without it every launch is a
squared-loss kernel.

Algorithmic bytes (each input read once, each output written once):
  point pass:  n_obs x (4 obs_of + 4 cam_of + 16 uv) + n_pts x (8 pt_row_ptr + 32 point + 72 V + 24 t) + n_cam x (192 record + 72 x)
  camera pass: n_obs x (4 pt_idx + 16 uv) + n_pts x (32 point + 24 t) + n_cam x (8 row_ptr + 192 record + 648 U + 72 x + 72 y)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loss", choices=["huber", "cauchy", "soft_l1"], default=None, help="robust loss (default: squared)")
    ap.add_argument("--loss-scale", type=float, default=3e-3, help="its scale a, in the residuals' units (noise is 1e-3)")
    ap.add_argument("--preconditioner", choices=["block_jacobi", "schur_jacobi"], default="block_jacobi")
    ap.add_argument("--constant", choices=["none", "intrinsics", "gauge", "points"], default="none",
                    help="hold parameters constant in the solve (default: none)")
    ap.add_argument("--to-tol", action="store_true", help="also time solves to rel_tol 1e-2 and 1e-4")
    ap.add_argument("--tol-max-iters", type=int, default=1000)
    a = ap.parse_args()
    loss = (a.loss, a.loss_scale) if a.loss else None
    import __graft_entry__ as entry
    entry.build()
    import torch
    import benchkit as B
    from city2ba_amd import device as D
    from city2ba_amd import noise as N
    dev = torch.device("cuda", 0)
    lam = 1e-4

    ba = B.bench_grid(a.blocks, cull=False, mirror=False)    # bench.py's instance
    N.add_noise(ba, 0.0, 0.0, 0.0, 1e-3, seed=20243)

    # Level 0 over the same state
    lv = B.level0(ba, point_rows=True)
    n_cam, n_pts, n = lv.n_cam, lv.n_pts, lv.n_obs
    camblk, rows, prows, pts4, pi, uv = lv.camblk, lv.rows, lv.prows, lv.pts4, lv.pt_idx, lv.uv
    f64 = dict(dtype=torch.float64, device=dev)
    U, gc = torch.empty((n_cam, 9, 9), **f64), torch.empty((n_cam, 9), **f64)
    V, gp = torch.empty((n_pts, 3, 3), **f64), torch.empty((n_pts, 3), **f64)
    D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U, gc, loss=loss)
    D.normal_points_rows(camblk, pts4, prows, uv, V, gp, loss=loss)
    x = torch.randn((n_cam, 9), **f64) * 1e-3
    t, y = torch.empty((n_pts, 3), **f64), torch.empty((n_cam, 9), **f64)

    def events(fn):
        return B.us_record(B.each_us(fn, max(a.reps, 10), a.warmup + 2))

    def wall(fn):
        times = B.wall_ms(fn, a.reps, a.warmup)
        return {"median_ms": round(B.upper_median(times), 3), "min_ms": round(min(times), 3)}

    us_p = events(lambda: D.schur_points_rows(camblk, pts4, prows, uv, V, lam, x, None, t, loss=loss))
    us_c = events(lambda: D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, lam, x, t, y, loss=loss))
    bytes_p = n * 24 + n_pts * (8 + 32 + 72 + 24) + n_cam * (192 + 72)
    bytes_c = n * 20 + n_pts * (32 + 24) + n_cam * (8 + 192 + 648 + 72 + 72)
    frac = lambda b, us: round(B.frac_of_peak(b, us), 4)
    sj = a.preconditioner == "schur_jacobi"
    if sj:                                                   # the pass that forms M, alone
        M = torch.empty((n_cam, 9, 9), **f64)
        us_m = events(lambda: D.schur_jacobi_blocks(camblk, pts4, rows, pi, uv, U, V, lam, M, loss=loss))
        bytes_m = n * 20 + n_pts * (32 + 72) + n_cam * (8 + 192 + 72 + 648)      # + U's diagonal (its lines), M written once
        del M
    del U, gc, V, gp, t, y, x, prows, rows, camblk, lv
    torch.cuda.empty_cache()

    dc, dp = torch.empty((n_cam, 9), **f64), torch.empty((n_pts, 3), **f64)
    info = {}
    ba.set_preconditioner(a.preconditioner)
    if loss:
        ba.set_loss(*loss)
    if a.constant != "none":
        import numpy as np
        from city2ba_amd import solve as LM
        cm = np.zeros(n_cam, dtype=np.uint16)
        if a.constant == "intrinsics":
            cm[:] = LM.INTRINSICS
        elif a.constant == "gauge":
            cm[0], cm[1] = LM.ALL, 1 << 3
        ba.set_constant(cm, np.ones(n_pts, dtype=bool) if a.constant == "points" else None)

    def solve(k):
        info[k] = ba.solve_step(lam, max_iters=k, rel_tol=0.0, out=(dc, dp))[2]

    s0 = wall(lambda: solve(0))
    s25 = wall(lambda: solve(25))
    zc, zp = torch.zeros_like(dc), torch.zeros_like(dp)
    ap_ms = wall(lambda: ba.apply_step(zc, zp))
    rc_ms = wall(ba.robust_cost) if loss else None           # what an LM iteration under a loss pays for its accept test
    to_tol = {}
    if a.to_tol:
        for tol in (1e-2, 1e-4):
            res = {}

            def solve_tol():
                res["info"] = ba.solve_step(lam, max_iters=a.tol_max_iters, rel_tol=tol, out=(dc, dp))[2]

            w = wall(solve_tol)
            to_tol["to_rel_tol_%g" % tol] = dict(w, iterations=res["info"]["iterations"], status=res["info"]["status"],
                                                 rel_residual=res["info"]["rel_residual"])
    out = {
        "blocks": a.blocks, "preconditioner": a.preconditioner, "constant": a.constant, "loss": a.loss, "loss_scale": a.loss_scale if a.loss else None, "n_obs": n, "n_cam": n_cam, "n_pts": n_pts, "lambda": lam,
        "points_pass": dict(us_p, algorithmic_bytes=bytes_p, frac_of_8TBs=frac(bytes_p, us_p["median_us"])),
        "cameras_pass": dict(us_c, algorithmic_bytes=bytes_c, frac_of_8TBs=frac(bytes_c, us_c["median_us"])),
        "both_passes_us": round(us_p["median_us"] + us_c["median_us"], 1),
        "solve_0_iterations": s0,
        "solve_25_iterations": s25,
        "pcg_iteration_ms": round((s25["median_ms"] - s0["median_ms"]) / 25.0, 3),
        "apply_step": ap_ms,
        **({"robust_cost": rc_ms} if loss else {}),
        **({"schur_jacobi_pass": dict(us_m, algorithmic_bytes=bytes_m, frac_of_8TBs=frac(bytes_m, us_m["median_us"])),
            "fallbacks": ba.preconditioner_fallbacks()} if sj else {}),
        **to_tol,
        "info_25": info[25],
    }
    ba.close()
    B.emit(out)


if __name__ == "__main__":
    main()
