#!/usr/bin/env python3
"""Wall time of the Levenberg-Marquardt loop in Python (city2ba_amd.solve.levenberg_marquardt: a download per accepted
step, an upload per rejected one) against the loop inside the library (levenberg_marquardt_device: checkpoint and
rollback on the device), on the same noisy synthetic grid in the same process, and of one forced rejection: the upload
the Python loop restores with against rollback(), each with the solve_step that follows it (the upload drops the row
structure, the transpose and the solve buffers; the rollback keeps them).  Prints one JSON line.

    python tools/bench_lm.py [--blocks 128] [--iterations 10] [--out profiles/lm_loop_bench_blocks128.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--lam", type=float, default=1e-4)
    ap.add_argument("--repeats", type=int, default=3, help="repeats of the forced rejection (the median is reported)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import noise as N, solve

    g = B.bench_grid(a.blocks)
    N.add_noise(g, 0.0, 0.0, 1e-2, 1e-3, seed=3)
    start = (g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), g.observations())
    sizes = g._sizes()
    g.close()

    def fresh():
        return c2b.BAProblem.from_bal(*start, device=0)

    warm = fresh()                                           # the first solve of a process pays for the kernels' load
    solve.levenberg_marquardt_device(warm, 1, lam=a.lam)
    warm.close()
    ba = fresh()
    t_py, hp = B.wall_s(lambda: solve.levenberg_marquardt(ba, a.iterations, lam=a.lam))
    end_py = (ba.cameras_bal(), ba.points())
    ba.close()
    ba = fresh()
    t_dev, (hd, summary) = B.wall_s(lambda: solve.levenberg_marquardt_device(ba, a.iterations, lam=a.lam))
    same = end_py[0].tobytes() == ba.cameras_bal().tobytes() and end_py[1].tobytes() == ba.points().tobytes() and \
        [e["error"] for e in hp] == [e["error"] for e in hd]

    # one forced rejection, both ways, from the solved state
    bal9, pts = ba.cameras_bal(), ba.points()
    row_ptr, pt_idx, uv = ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations()
    lam = summary["lam_next"]
    dc, dp, _ = ba.solve_step(lam)
    rej = dict(upload=[], step_after_upload=[], rollback=[], step_after_rollback=[])
    for _ in range(a.repeats):
        ba.checkpoint()
        ba.apply_step(dc, dp)
        rej["rollback"].append(B.wall_s(ba.rollback)[0])
        rej["step_after_rollback"].append(B.wall_s(lambda: ba.solve_step(lam, out=(dc, dp)))[0])
        ba.apply_step(dc, dp)
        rej["upload"].append(B.wall_s(lambda: ba._upload(bal9, True, pts, row_ptr, pt_idx, uv))[0])
        rej["step_after_upload"].append(B.wall_s(lambda: ba.solve_step(lam, out=(dc, dp)))[0])
    ba.close()
    med = {k: B.median(v) * 1e3 for k, v in rej.items()}
    n = max(len(hd), 1)
    result = dict(bench="lm_loop", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], iterations=len(hd),
                  accepted=sum(e["accepted"] for e in hd), pcg_iterations=sum(e["pcg_iterations"] for e in hd),
                  python_loop_s=round(t_py, 4), device_loop_s=round(t_dev, 4),
                  python_ms_per_iteration=round(t_py / n * 1e3, 2), device_ms_per_iteration=round(t_dev / n * 1e3, 2),
                  difference_ms_per_iteration=round((t_py - t_dev) / n * 1e3, 2), same_result=bool(same),
                  rejection_ms=dict(upload=round(med["upload"], 3), rollback=round(med["rollback"], 3),
                                    step_after_upload=round(med["step_after_upload"], 2),
                                    step_after_rollback=round(med["step_after_rollback"], 2)),
                  cost=[summary["initial_cost"], summary["final_cost"]])
    B.emit(result, a.out)


if __name__ == "__main__":
    main()
