#!/usr/bin/env python3
"""Time the priors of the device LM step on `synthetic --blocks B` (default 128; observation noise 1e-3) and
print one JSON line:
  * the three prior launches at Level 0 by HIP events (k_prior_cameras into U and gc, k_prior_points into V and gp,
    k_prior_model), with centre and intrinsics priors on every camera and a prior on every 100th point;
  * solve_step with 0 iterations (everything but PCG, host clock) interleaved over --rounds rounds, each round in the order
    none, zero weights, none, zero weights, in force: without priors, with priors whose weights are all 0 (stored as no
    priors: nothing is launched) and with the priors above in force; the spread of the no-prior figure over its 2 x rounds
    measurements is reported next to the differences of the medians;
  * on the same grid after noise.add_drift (--drift: the displacement and the rotation it reaches at the grid's far corner,
    from which strength = displacement / extent^2 and angle strength = rotation / extent^1.2), for both preconditioners, without and with centre priors at the
    clean centres (sigma --sigma): the PCG iterations of one step to rel_tol 1e-6 (at most --tol-max-iters), and a
    Levenberg-Marquardt run of --lm-iterations iterations -- its costs, the gradient maximum per iteration and the first
    iteration at which that fell to --gradient-drop of its first value (null: never).

    python tools/bench_priors.py [--blocks 128] [--reps 5] [--warmup 1] [--rounds 3] [--sigma 0.3] [--out FILE]
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.3)
    ap.add_argument("--drift", type=float, nargs=3, default=(1.0, 0.03, 0.01),
                    help="add_drift's displacement (units) and rotation (rad) at the grid's far corner, and its std")
    ap.add_argument("--tol-max-iters", type=int, default=1000)
    ap.add_argument("--lm-iterations", type=int, default=12)
    ap.add_argument("--gradient-drop", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import numpy as np
    import torch
    import benchkit as B
    from city2ba_amd import device as D
    from city2ba_amd import noise as N
    from city2ba_amd import solve as LM
    dev = torch.device("cuda", 0)
    lam = 1e-4
    f64 = dict(dtype=torch.float64, device=dev)

    def grid():
        ba = B.bench_grid(a.blocks, cull=False, mirror=False)    # bench.py's instance
        N.add_noise(ba, 0.0, 0.0, 0.0, 1e-3, seed=20243)
        return ba

    def events(fn):
        return B.us_record(B.each_us(fn, max(a.reps, 10), a.warmup + 2))

    ba = grid()
    n_cam, n_pts, n = ba._sizes()
    clean = ba._camera_centers()
    intr = ba.cameras_bal()[:, 6:9].copy()
    pts = ba.points()
    xw = np.zeros((n_pts, 3))
    xw[::100] = 1.0
    every = dict(camera_centers=clean + 1e-3, camera_center_weights=1.0 / a.sigma, intrinsics=intr, intrinsics_weights=[10.0, 100.0, 100.0],
                 points=pts + 1e-3, point_weights=xw)

    # ---- the three launches, Level 0 ----------------------------------------------------------------------------------
    lv = B.level0(ba)
    camblk, pts4 = lv.camblk, lv.pts4
    U, gc = torch.zeros((n_cam, 9, 9), **f64), torch.zeros((n_cam, 9), **f64)
    V, gp = torch.zeros((n_pts, 3, 3), **f64), torch.zeros((n_pts, 3), **f64)
    dc, dp = torch.randn((n_cam, 9), **f64) * 1e-3, torch.randn((n_pts, 3), **f64) * 1e-3
    c0, cw = torch.from_numpy(every["camera_centers"]).to(dev), torch.full((n_cam, 3), 1.0 / a.sigma, **f64)
    i0, iw = torch.from_numpy(intr).to(dev), torch.tensor([10.0, 100.0, 100.0], **f64).repeat(n_cam, 1).contiguous()
    x0, xwd = torch.from_numpy(every["points"]).to(dev), torch.from_numpy(xw).to(dev)
    sums = torch.zeros(2, **f64)
    us_c = events(lambda: D.prior_cameras_rows(camblk, c0, cw, i0, iw, U=U, gc=gc))
    us_p = events(lambda: D.prior_points_rows(pts4, x0, xwd, V=V, gp=gp))
    us_m = events(lambda: D.prior_model_rows(camblk, pts4, dc, dp, sums, c0, cw, i0, iw, x0, xwd))
    bytes_c = n_cam * (256 + 48 + 48 + 2 * 39 * 8 + 2 * 72)          # record, two pairs, 39 entries of U and gc read and written
    bytes_p = n_pts * 24 + (n_pts // 100 + 1) * (32 + 24 + 48 + 48)    # every point's weights; point, target, V's diagonal and gp of every 100th
    launches = {"prior_cameras": dict(us_c, algorithmic_bytes=bytes_c, frac_of_8TBs=round(B.frac_of_peak(bytes_c, us_c["median_us"]), 4)),
                "prior_points": dict(us_p, algorithmic_bytes=bytes_p), "prior_model": us_m,
                "three_launches_us": round(us_c["median_us"] + us_p["median_us"] + us_m["median_us"], 1)}
    del U, gc, V, gp, c0, cw, i0, iw, x0, xwd, camblk, lv, pts4
    torch.cuda.empty_cache()

    # ---- solve_step with 0 iterations, interleaved ------------------------------------------------------------------------
    out_c, out_p = torch.empty((n_cam, 9), **f64), torch.empty((n_pts, 3), **f64)
    rounds = {"none": [], "zero_weights": [], "in_force": []}
    for _ in range(a.rounds):
        for how in ("none", "zero_weights", "none", "zero_weights", "in_force"):
            if how == "none":
                ba.set_priors()
            elif how == "zero_weights":
                ba.set_priors(camera_center_weights=0.0, intrinsics_weights=0.0, point_weights=0.0)
            else:
                ba.set_priors(**every)
            times = B.wall_ms(lambda: ba.solve_step(lam, max_iters=0, rel_tol=0.0, out=(out_c, out_p)), a.reps, a.warmup)
            rounds[how].append(round(B.upper_median(times), 3))
    none = rounds["none"]
    solve0 = {k: {"per_round_ms": v, "median_ms": round(B.upper_median(v), 3)} for k, v in rounds.items()}
    solve0["no_prior_spread_ms"] = round(max(none) - min(none), 3)
    solve0["zero_weights_minus_none_ms"] = round(B.upper_median(rounds["zero_weights"]) - B.upper_median(none), 3)
    solve0["in_force_minus_none_ms"] = round(B.upper_median(rounds["in_force"]) - B.upper_median(none), 3)
    ba.close()
    del out_c, out_p, dc, dp
    torch.cuda.empty_cache()

    # ---- a drifted problem: PCG and LM iterations without and with centre priors ------------------------------------------------
    drifted = {}
    for kind in ("block_jacobi", "schur_jacobi"):
        for tied in (False, True):
            ba = grid()
            extent = 20.0 * a.blocks * 2.0 ** 0.5
            N.add_drift(ba, a.drift[0] / extent ** 2, a.drift[1] / extent ** 1.2, a.drift[2], [1.0, 0.5, 0.0], seed=7)
            dist = lambda: float(np.mean(np.linalg.norm(ba._camera_centers() - clean, axis=1)))
            start = dist()
            ba.set_preconditioner(kind)
            if tied:
                ba.set_priors(camera_centers=clean, camera_center_weights=1.0 / a.sigma)
            pcg_s, (_, _, info) = B.wall_s(lambda: ba.solve_step(lam, max_iters=a.tol_max_iters, rel_tol=1e-6))
            lm_s, (h, s) = B.wall_s(lambda: LM.levenberg_marquardt_device(ba, a.lm_iterations, lam=lam, max_iters=100, rel_tol=1e-6))
            pcg_ms, lm_ms = pcg_s * 1e3, lm_s * 1e3
            g = [e["gradient_max"] for e in h]
            reached = next((k for k, v in enumerate(g) if v <= a.gradient_drop * g[0]), None)
            drifted["%s %s" % (kind, "centre priors" if tied else "no priors")] = {
                "pcg_to_1e-6": dict(iterations=info["iterations"], status=info["status"], rel_residual=info["rel_residual"], ms=round(pcg_ms, 1)),
                "lm": dict(iterations=s["iterations"], termination=s["termination"], accepted="".join("A" if e["accepted"] else "R" for e in h),
                        pcg_iterations=[e["pcg_iterations"] for e in h], cost=[s["initial_cost"], s["final_cost"]],
                        gradient_max=[float("%.4g" % v) for v in g], first_iteration_at_gradient_drop=reached, ms=round(lm_ms, 1)),
                "mean_centre_distance": dict(start=round(start, 6), after_lm=round(dist(), 6))}
            ba.close()
    out = {"blocks": a.blocks, "n_obs": n, "n_cam": n_cam, "n_pts": n_pts, "lambda": lam, "sigma": a.sigma, "drift": list(a.drift),
           "gradient_drop": a.gradient_drop, "launches": launches, "solve_0_iterations": solve0, "drifted": drifted}
    B.emit(out, a.out)


if __name__ == "__main__":
    main()
