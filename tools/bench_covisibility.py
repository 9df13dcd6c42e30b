#!/usr/bin/env python3
"""Size and time of the camera covisibility graph and of the windows grown over it on the synthetic grid, as it is
built and again with its cameras permuted by a seeded permutation (ba.subset(perm, arange(n_pts))): index order then says nothing
about the street, which is the case covisibility windows exist for.

For each of the two lists:
1. the graph at --min-shared: directed edges, maximum and mean degree, its bytes, and how many cameras took the heavy path;
2. the degree pass and the fill pass (c2b_covisibility_degree_rows / _fill_rows on the exported list, the outputs allocated
   beforehand) by HIP events, and the whole c2b_problem_covisibility call (transpose cached; temporaries, both passes, the read
   of the edge count between them) by a host clock around the synchronous call: medians of --repeats after a warm-up;
3. the host comparator: scipy.sparse B B^T on the downloaded list, by a host clock (one run);
4. BAProblem.neighbourhood from the middle camera, hops=None, at max_cameras 1 024 and 16 384 (the graph cached), by a host
   clock: medians of --repeats.
On the permuted list also one sweep's windows of --size cameras by="index" and by="covisibility": the windows are extracted
(BAProblem.window, halo) but not solved, and the children's cameras and observations are summed: the halo ratio of each is
(child cameras) / (cameras), an observation of how much of every window is rim.
Prints one JSON line.

    python tools/bench_covisibility.py [--blocks 128] [--repeats 7] [--out profiles/covisibility_bench_blocks128.json]
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
    ap.add_argument("--min-shared", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=7, help="timed calls; the median is reported")
    ap.add_argument("--size", type=int, default=16384, help="cameras per window of the sweep")
    ap.add_argument("--seed", type=int, default=11, help="of the camera permutation")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy comparator")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import ctypes as C
    import numpy as np
    import torch
    import benchkit                                          # (B is the incidence matrix of the host comparator here)
    from city2ba_amd import _lib as L, device as D
    lib = L.lib()
    ms = a.min_shared

    def median_ms(samples):
        return round(benchkit.median(samples), 4), benchkit.spread(samples, 4)

    def wall(fn):
        return median_ms(benchkit.wall_ms(fn, a.repeats, 1))

    def figures(ba, with_host):
        n_cam, n_pts, n_obs = ba._sizes()
        nbr_ptr, nbr, shared = ba.covisibility(ms)
        deg = np.diff(nbr_ptr.astype(np.int64))
        rec = dict(n_cam=n_cam, n_pts=n_pts, n_obs=n_obs, min_shared=ms, edges_directed=int(len(nbr)), max_degree=int(deg.max()) if n_cam else 0,
                   mean_degree=round(float(deg.mean()), 2) if n_cam else 0.0, graph_bytes=int(nbr_ptr.nbytes + nbr.nbytes + shared.nbytes),
                   heavy_cameras=ba.covisibility_heavy_cameras(), wave_slots=D.COVIS_WAVE_SLOTS)
        # the whole Level-1 call: another threshold drops the graph, so every timed call builds (the transpose stays)
        other = ms + 1
        ba.covisibility(other)

        def build():
            n = C.c_int64()
            L.check(lib.c2b_problem_covisibility(ba._h, other, C.byref(n)))
            L.check(lib.c2b_problem_covisibility(ba._h, ms, C.byref(n)))
        both, spread = wall(build)
        rec["problem_covisibility_two_thresholds_ms"] = both
        rec["problem_covisibility_two_thresholds_spread_ms"] = spread
        # the two passes alone, on the exported list, by three events in a chain: the fill pass follows the degree pass at once, as
        # in the Level-1 call
        lv = benchkit.level0(ba, point_rows=True)
        rows, prows, dev = lv.rows, lv.prows, lv.pt_idx.device
        temp = D._covis_temp(n_cam, L.COVIS_TEMP_GRAPH, dev)
        d_ptr = torch.empty(n_cam + 1, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        d_nbr = torch.empty(max(len(nbr), 1), dtype=torch.int32, device=dev)
        d_shared = torch.empty(max(len(nbr), 1), dtype=torch.int32, device=dev)
        args = (D._p(rows.row_ptr), D._p(lv.pt_idx), D._p(prows.pt_row_ptr), D._p(prows.obs_of), D._p(prows.cam_of), n_cam, n_pts, n_obs, ms, D._p(temp))
        t_deg, t_fill = [], []
        for k in range(a.repeats + 1):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            L.check(lib.c2b_covisibility_degree_rows(*args, D._p(d_ptr), D._p(counts), D._stream()))
            e[1].record()
            L.check(lib.c2b_covisibility_fill_rows(*args, D._p(d_ptr), D._p(d_nbr), D._p(d_shared), D._stream()))
            e[2].record()
            torch.cuda.synchronize()
            if k:
                t_deg.append(e[0].elapsed_time(e[1]))
                t_fill.append(e[1].elapsed_time(e[2]))
        assert int(counts[0].item()) == len(nbr) and np.array_equal(d_nbr.cpu().numpy()[:len(nbr)].view(np.uint32), nbr)
        rec["degree_pass_ms"], rec["degree_pass_spread_ms"] = median_ms(t_deg)
        rec["fill_pass_ms"], rec["fill_pass_spread_ms"] = median_ms(t_fill)
        del lv, rows, prows, temp, d_ptr, d_nbr, d_shared
        if with_host:
            import scipy.sparse as sp
            t0 = time.perf_counter()
            row_ptr, pt_idx = ba.row_ptr.astype(np.int64), ba.pt_idx.astype(np.int64)          # the downloaded list
            B = sp.csr_matrix((np.ones(len(pt_idx), dtype=np.int32), pt_idx, row_ptr), shape=(n_cam, n_pts))
            B.sum_duplicates()
            B.data[:] = 1
            G = (B @ B.T).tocsr()
            G.setdiag(0)
            G.eliminate_zeros()
            rec["host_scipy_bbt_s"] = round(time.perf_counter() - t0, 3)
            if ms == 1:
                assert G.nnz == len(nbr), (G.nnz, len(nbr))
            del B, G
        ba.covisibility(ms)
        for cap in (1024, 16384):
            if cap > n_cam:
                continue
            got = ba.neighbourhood([n_cam // 2], hops=None, min_shared=ms, max_cameras=cap)
            t, spread = wall(lambda: ba.neighbourhood([n_cam // 2], hops=None, min_shared=ms, max_cameras=cap))
            rec["neighbourhood_%d_ms" % cap], rec["neighbourhood_%d_spread_ms" % cap], rec["neighbourhood_%d_cameras" % cap] = t, spread, int(len(got))
        return rec

    def sweep(ba, by):
        """one sweep's windows, extracted and measured, not solved"""
        n_cam = ba.num_cameras()
        cams = obs = windows = 0
        if by == "index":
            for lo in range(0, n_cam, a.size):
                child = ba.window(range(lo, min(lo + a.size, n_cam)), halo=True)
                c, _, o = child._sizes()
                child.close()
                cams, obs, windows = cams + c, obs + o, windows + 1
        else:
            todo = np.ones(n_cam, dtype=bool)
            first = 0
            while first < n_cam:
                idx = ba.neighbourhood([first], hops=None, min_shared=ms, max_cameras=a.size, within=todo)
                child = ba.window(idx, halo=True)
                c, _, o = child._sizes()
                child.close()
                cams, obs, windows = cams + c, obs + o, windows + 1
                todo[idx] = False
                while first < n_cam and not todo[first]:
                    first += 1
        return dict(windows=windows, child_cameras=int(cams), child_observations=int(obs), halo_ratio=round(cams / max(n_cam, 1), 3),
                    observation_ratio=round(obs / max(ba.num_observations(), 1), 3))

    ba = benchkit.bench_grid(a.blocks)
    n_cam, n_pts, _ = ba._sizes()
    result = dict(bench="covisibility", blocks=a.blocks, repeats=a.repeats, grid=figures(ba, not a.no_host))
    perm = np.random.default_rng(a.seed).permutation(n_cam)
    shuffled = ba.subset(perm, np.arange(n_pts))
    ba.close()
    result["permuted"] = figures(shuffled, False)
    result["permuted_sweep"] = dict(size=a.size, index=sweep(shuffled, "index"), covisibility=sweep(shuffled, "covisibility"))
    shuffled.close()
    benchkit.emit(result, a.out)


if __name__ == "__main__":
    main()
