#!/usr/bin/env python3
"""Time the direct solve of the reduced camera system on a window of the synthetic grid and print one JSON line.

The problem: tools/bench_lm.py's noisy grid of --blocks blocks, and of it the window of --window consecutive cameras from the
middle (BAProblem.window, without the halo unless --halo: the child then has exactly that many cameras and S that order).
  * Level 0 (HIP events, on the window's own S at lambda 1e-4): c2b_dense_scatter_rows, c2b_dense_cholesky (microseconds and
    GFLOP/s at Np^3 / 3) and c2b_dense_cholesky_solve, with the launches each takes.
  * solve_step (wall clock): under linear_solver = cholesky, and under pcg with the implicit and the explicit Schur complement, at
    the LM default (max_iters 100, rel_tol 1e-6) and converged to rel_tol 1e-10 (max_iters 5000), with iterations, status and the
    relative residual each reaches.
  * levenberg_marquardt_device to termination (function_tol 1e-6, at most --iterations): cholesky, and pcg at the LM default, from
    the same start: wall time, iterations, PCG iterations and the cost reached.

    python tools/bench_dense_schur.py [--blocks 16] [--window 256] [--halo] [--reps 5] [--warmup 1] [--iterations 50] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--window", type=int, default=256, help="seed cameras of the window")
    ap.add_argument("--halo", action="store_true", help="keep the rim cameras (constant) in the child")
    ap.add_argument("--sigma", type=float, default=1e-3, help="observation noise")
    ap.add_argument("--point-std", type=float, default=1e-2, help="noise on the points the solves start from")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=50, help="most LM iterations of the loops")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import numpy as np
    import torch
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import device as D
    from city2ba_amd import noise as N, solve

    dev = torch.device("cuda", 0)
    lam = 1e-4
    grid = B.bench_grid(a.blocks)
    N.add_noise(grid, 0.0, 0.0, a.point_std, a.sigma, seed=3)
    n_cam_grid = grid._sizes()[0]
    seeds = min(a.window, n_cam_grid)
    lo = (n_cam_grid - seeds) // 2
    ba = grid.window(np.arange(lo, lo + seeds), halo=a.halo)
    grid.close()
    n_cam, n_pts, n_obs = ba._sizes()
    n, Np = 9 * n_cam, (9 * n_cam + 63) // 64 * 64
    T = Np // 64
    start = (ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
    masks = ba.constant()

    def wall(fn):
        times = B.wall_ms(fn, a.reps, a.warmup)
        return {"median_ms": round(B.upper_median(times), 3), "min_ms": round(min(times), 3)}

    # ---- Level 0 on the window's own S
    nbr_ptr, nbr, Sd, So, b = ba.schur_complement(lam)
    t = lambda v, dt=None: torch.from_numpy(np.ascontiguousarray(v if dt is None else v.view(dt))).to(dev)
    d_ptr, d_nbr = t(nbr_ptr, np.int64), t(nbr if len(nbr) else np.zeros(1, dtype=np.uint32), np.int32)
    d_Sd, d_So = t(Sd), t(So if len(So) else np.zeros((1, 9, 9)))
    A = torch.empty((Np, Np), dtype=torch.float64, device=dev)
    x = torch.zeros(Np, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    rhs = np.zeros(Np)
    rhs[:n] = b.reshape(-1)
    d_b = t(rhs)
    events = lambda fn: B.us_record(B.each_us(fn, max(a.reps, 10), a.warmup + 2))
    us_scatter = events(lambda: D.dense_scatter_rows(d_ptr, d_nbr, d_Sd, d_So, A))

    def factor():                                            # (the factorisation is in place: S is scattered again before each)
        D.dense_scatter_rows(d_ptr, d_nbr, d_Sd, d_So, A)
        D.dense_cholesky(A, n, info)
    us_both = events(factor)
    us_factor = {k: round(us_both[k] - us_scatter[k], 1) for k in us_both}
    factor()

    def substitute():
        x.copy_(d_b)
        D.dense_cholesky_solve(A, n, x)
    us_solve = events(substitute)
    torch.cuda.synchronize()
    flops = Np ** 3 / 3.0
    level0 = dict(scatter=us_scatter, factor=dict(us_factor, launches=3 * T - 2, gflops=round(flops / (us_factor["median_us"] * 1e-6) / 1e9, 1),
                                                  info=int(info.cpu()[0])),
                  solve=dict(us_solve, launches=4 * T - 2, note="with the copy of b"))
    del A, x, d_Sd, d_So, d_ptr, d_nbr, d_b
    torch.cuda.empty_cache()

    # ---- solve_step
    f64 = dict(dtype=torch.float64, device=dev)
    dc, dp = torch.empty((n_cam, 9), **f64), torch.empty((n_pts, 3), **f64)
    steps = {}
    for name, linear, schur, max_iters, tol in (("cholesky", "cholesky", "implicit", 100, 1e-6),
                                                ("pcg_implicit_default", "pcg", "implicit", 100, 1e-6), ("pcg_explicit_default", "pcg", "explicit", 100, 1e-6),
                                                ("pcg_implicit_1e-10", "pcg", "implicit", 5000, 1e-10), ("pcg_explicit_1e-10", "pcg", "explicit", 5000, 1e-10)):
        ba.set_linear_solver(linear)
        ba.set_schur(schur)
        res = {}

        def step():
            res["info"] = ba.solve_step(lam, max_iters=max_iters, rel_tol=tol, out=(dc, dp))[2]
        steps[name] = dict(wall(step), iterations=res["info"]["iterations"], status=res["info"]["status"], rel_residual=res["info"]["rel_residual"])
    bytes_dense = None
    ba.set_schur("implicit")
    ba.set_linear_solver("cholesky")
    bytes_dense = ba.linear_solver_bytes()
    ba.close()

    # ---- the LM loop to termination, from the same start
    loops = {}
    for name, linear in (("cholesky", "cholesky"), ("pcg_default", "pcg")):
        g = c2b.BAProblem.from_bal(*start, device=0)
        g.set_constant(*masks)
        solve.levenberg_marquardt_device(g, 1, linear_solver=linear)         # the first solve of a kind pays for the kernels' load
        g.close()
        g = c2b.BAProblem.from_bal(*start, device=0)
        g.set_constant(*masks)
        secs, (hist, s) = B.wall_s(lambda: solve.levenberg_marquardt_device(g, a.iterations, function_tol=1e-6, linear_solver=linear))
        loops[name] = dict(wall_s=round(secs, 4), iterations=s["iterations"], termination=s["reason"], initial_cost=s["initial_cost"],
                           final_cost=s["final_cost"], pcg_iterations=sum(h["pcg_iterations"] for h in hist),
                           accepted=sum(1 for h in hist if h["accepted"]), statuses=sorted(set(h["status"] for h in hist)))
        g.close()
    B.emit(dict(bench="dense_schur", blocks=a.blocks, window=seeds, halo=a.halo, n_cam=n_cam, n_pts=n_pts, n_obs=n_obs, n_edges=int(len(nbr)),
                order=n, padded_order=Np, linear_solver_bytes=bytes_dense, **{"lambda": lam}, level0=level0, solve_step=steps, lm=loops), a.out)


if __name__ == "__main__":
    main()
