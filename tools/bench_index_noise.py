#!/usr/bin/env python3
"""Time of the index noise on a synthetic grid, device route against host route, in one build:

  passes   each of the four passes alone on a problem read from the file: the device entry (c2b_problem_drop_features, ...: they
           synchronise, so the wall clock around the call) and the host route of city2ba_amd.noise (download, the host pass of
           csrc/host_noise.hpp, a new problem uploaded).  drop runs first on the problem as read; join, split and mismatch follow on
           what the pass before left (no cull in between: the passes are timed, not the chain).
  cli      `city2ba noise IN OUT --drop-features 0.8 --split-landmarks 0.1 --join-landmarks 0.05 --mismatch-chance 0.05 --seed S`
           with `--index-noise device` and with `--index-noise host`, end to end (process start to exit), and the phase times
           C2B_TIMING=1 prints for each.

The median over `--repeats` is reported.  Prints one JSON line.

    python tools/bench_index_noise.py [--blocks 128] [--repeats 3] [--seed 5] [--dir /tmp] [--out profiles/index_noise_bench_blocks128.json]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAIN = ["--drop-features", "0.8", "--split-landmarks", "0.1", "--join-landmarks", "0.05", "--mismatch-chance", "0.05"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--dir", default="", help="where the input and output files go (default: a temporary directory)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    cli = entry.build_cli()
    import ctypes as C
    import benchkit as B
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L, noise as N

    tmp = tempfile.TemporaryDirectory(dir=a.dir or None)
    src, out = os.path.join(tmp.name, "grid.bbal"), os.path.join(tmp.name, "out.bbal")
    subprocess.run([cli, "synthetic", src, "--blocks", str(a.blocks)], check=True, capture_output=True, timeout=1200)

    # ---- the passes alone -------------------------------------------------------------------------------------------------------
    lib = L.lib()
    passes = (("drop_features", lib.c2b_problem_drop_features, 0.8), ("join_landmarks", lib.c2b_problem_join_landmarks, 0.1),
              ("split_landmarks", lib.c2b_problem_split_landmarks, 0.1), ("add_incorrect_correspondences", lib.c2b_problem_add_incorrect_correspondences, 0.05))
    t_dev = {name: [] for name, _, _ in passes}
    t_host = {name: [] for name, _, _ in passes}
    counts = {}
    sizes = None
    for rep in range(a.repeats):
        ba = c2b.BAProblem.from_file(src)
        sizes = sizes or ba._sizes()
        ba.total_reprojection_error(2.0)                         # the cameras' records and the row structure exist, as in a pipeline
        for k, (name, f, value) in enumerate(passes):
            n = C.c_int64()
            t_dev[name].append(B.wall_s(lambda: L.check(f(ba._h, value, a.seed + 2 + k, C.byref(n))))[0] * 1e3)
            counts[name] = int(n.value)
        ba.close()
        ba = c2b.BAProblem.from_file(src)
        ba.total_reprojection_error(2.0)
        for k, (name, _, value) in enumerate(passes):
            dt, nxt = B.wall_s(lambda: getattr(N, name)(ba, value, seed=a.seed + 2 + k))
            t_host[name].append(dt * 1e3)
            ba.close()
            ba = nxt
        ba.close()

    # ---- the command line, end to end -------------------------------------------------------------------------------------------
    def run(route):                                              # (a child process from start to exit: no device work of this one to wait for)
        t0 = time.perf_counter()
        r = subprocess.run([cli, "noise", src, out] + CHAIN + ["--seed", str(a.seed), "--index-noise", route], capture_output=True, text=True,
                           timeout=1200, env=dict(os.environ, C2B_TIMING="1"))
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit("noise --index-noise %s failed: %s" % (route, r.stderr))
        phases = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"(?m)^\[timing\] (.*?)\s+([0-9.]+) ms$", r.stderr)}
        report = [ln for ln in r.stdout.splitlines() if ln.startswith(("Initial error", "BA Problem", "Final error"))]
        return dt, phases, report

    t_cli = dict(device=[], host=[])
    phases, reports = {}, {}
    for rep in range(a.repeats):
        for route in ("device", "host"):
            dt, phases[route], reports[route] = run(route)
            t_cli[route].append(dt)

    med = B.median
    result = dict(bench="index_noise", blocks=a.blocks, n_cam=sizes[0], n_pts=sizes[1], n_obs=sizes[2], repeats=a.repeats, seed=a.seed,
                  file_bytes=os.path.getsize(src), counts=counts,
                  pass_ms=dict(device={k: round(med(v), 2) for k, v in t_dev.items()}, host_route={k: round(med(v), 2) for k, v in t_host.items()}),
                  cli_chain=" ".join(CHAIN),
                  cli_s=dict(device=round(med(t_cli["device"]), 3), host=round(med(t_cli["host"]), 3)),
                  cli_spread_s={k: B.spread(v, 3) for k, v in t_cli.items()},
                  cli_phases_ms=phases, cli_report=reports,
                  device_route_is_faster=bool(med(t_cli["device"]) < med(t_cli["host"])))
    B.emit(result, a.out)
    tmp.cleanup()


if __name__ == "__main__":
    main()
