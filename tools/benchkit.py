"""What the tools/bench_*.py scripts share: three ways to time a call, the statistics they report, the bench grid and its
Level-0 views, and the JSON line at the end.  Plain functions; torch, numpy and the package are imported inside the functions
that need them, so a script's --help works without a GPU.

Which timing fits which call:
  window_us   a Level-0 launch: it only enqueues, so `launches` of them go back to back between one pair of device events.
  each_us     a call that allocates or synchronises inside (PointRows, a pass with a read-back): one pair of events per call.
  wall_s/_ms  a whole Level-1 call (host work, transfers and launches): the host clock, between two device synchronises.
"""
import json
import os
import time

HBM_PEAK_BYTES_PER_S = 8.0e12       # the MI355X's HBM3E peak; a streaming copy reaches about 6.3e12 of it


# ---- timing ----------------------------------------------------------------------------------------------------------------
def _events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def window_us(fn, launches, before=None):
    """microseconds per launch of `launches` back-to-back calls of fn between one pair of events; `before` (restoring what fn
    overwrites, say) runs ahead of the first event"""
    import torch
    if before is not None:
        before()
    torch.cuda.synchronize()
    t0, t1 = _events()
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches


def each_us(fn, reps, warmup):
    """the microseconds of each of `reps` calls of fn, a pair of events around every call, after `warmup` untimed calls"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = _events()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return times


def wall_s(fn):
    """(seconds on the host clock, fn's result); the device is idle when the clock starts and when it stops"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def wall_ms(fn, reps, warmup):
    """the milliseconds of each of `reps` calls of fn by wall_s, after `warmup` untimed calls"""
    for _ in range(warmup):
        fn()
    return [wall_s(fn)[0] * 1e3 for _ in range(reps)]


# ---- statistics ------------------------------------------------------------------------------------------------------------
def median(xs):
    import numpy as np
    return float(np.median(xs))


def upper_median(xs):
    """the middle sample, the upper of the two middle ones of an even count"""
    return sorted(xs)[len(xs) // 2]


def spread(xs, places):
    return [round(min(xs), places), round(max(xs), places)]


def us_record(times):
    """what the per-call family reports of a list from each_us"""
    return {"median_us": round(upper_median(times), 1), "min_us": round(min(times), 1)}


def frac_of_peak(nbytes, us):
    """algorithmic bytes over time, over the HBM peak"""
    return nbytes / (us * 1e-6) / HBM_PEAK_BYTES_PER_S


# ---- set-up ----------------------------------------------------------------------------------------------------------------
def bench_grid(blocks, cull=True, mirror=True):
    """the synthetic grid every script measures on (`city2ba synthetic --blocks B`); cull=False, mirror=False is bench.py's
    instance, which stays on the device"""
    from city2ba_amd import synthetic as S
    return S.synthetic_grid(10, 10, blocks, 20.0, 1.0, 1.0, 1.0, 10.0, cull=cull, mirror=mirror)


def level0(ba, point_rows=False):
    """a resident problem as the Level-0 launchers take it: camblk (the camera table), rows (Rows), prows (PointRows, on
    request), pts4, pt_idx, uv, n_cam, n_pts, n_obs"""
    from types import SimpleNamespace
    from city2ba_amd import device as D
    n_cam, n_pts, n_obs = ba._sizes()
    ex = ba.export_device()
    rows = D.Rows(ex["row_ptr"], ex["n_obs"])
    return SimpleNamespace(camblk=D.cameras_prepare_state(ex["cam15"]), rows=rows,
                           prows=D.PointRows(rows, ex["pt_idx"], n_pts) if point_rows else None,
                           pts4=ex["pts4"], pt_idx=ex["pt_idx"], uv=ex["uv"], n_cam=n_cam, n_pts=n_pts, n_obs=n_obs)


# ---- output ----------------------------------------------------------------------------------------------------------------
def emit(result, out_path=""):
    """one JSON line to stdout, and to out_path when given"""
    line = json.dumps(result)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
