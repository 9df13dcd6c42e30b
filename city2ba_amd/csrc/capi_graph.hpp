// capi_graph.hpp -- Level 1, what changes or produces the resident problem's observation graph: cull, adopt_visibility, the outlier filter,
// the visibility entries (pairs, cell lists, the dense sweep and its occlusion filter), generate_world_points, graph download / export
// Part of the one translation unit of the C ABI: included by capi_problem.hpp where this text sat, never compiled or included on its own.

int c2b_problem_visibility_pairs(c2b_problem *p, int64_t n_pairs, const uint32_t *cam_idx, const uint32_t *pt_idx,
                                 double max_dist, double *uv_out, uint8_t *keep) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_visibility_pairs");
    if (n_pairs < 0 || (n_pairs && (!cam_idx || !pt_idx || !uv_out || !keep)))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_pairs: bad arguments");
    if (!n_pairs) return C2B_OK;
    for (int64_t i = 0; i < n_pairs; ++i)
        if (cam_idx[i] >= (uint64_t)p->n_cam || pt_idx[i] >= (uint64_t)p->n_pts)
            return fail(C2B_ERR_INDEX_OUT_OF_RANGE, "problem_visibility_pairs: pair %lld out of range", (long long)i);
    int rc = ensure_camblk(p);
    if (rc) return rc;
    DevBuf<uint32_t> d_c, d_p;
    DevBuf<double> d_uv;
    DevBuf<uint8_t> d_k;
    hipError_t e = d_c.alloc((size_t)n_pairs);
    if (e == hipSuccess) e = d_p.alloc((size_t)n_pairs);
    if (e == hipSuccess) e = d_uv.alloc(2 * (size_t)n_pairs);
    if (e == hipSuccess) e = d_k.alloc((size_t)n_pairs);
    if (e == hipSuccess) e = hipMemcpyAsync(d_c, cam_idx, sizeof(uint32_t) * n_pairs, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_p, pt_idx, sizeof(uint32_t) * n_pairs, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) {
        rc = c2b_visibility_pairs(p->camblk, p->pts4, d_c, d_p, n_pairs, max_dist, d_uv, d_k, p->stream);
        if (!rc) {
            e = hipMemcpyAsync(uv_out, d_uv, sizeof(double) * 2 * n_pairs, hipMemcpyDeviceToHost, p->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(keep, d_k, n_pairs, hipMemcpyDeviceToHost, p->stream);
        }
        hipError_t e2 = hipStreamSynchronize(p->stream);
        if (e == hipSuccess) e = e2;
    }
    if (rc) return rc;
    if (e != hipSuccess) return fail(hip_code(e), "problem_visibility_pairs: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_visibility_pairs")
}

/* ---- BAProblem::cull on the device (src/baproblem.rs:538-549) ---- */
extern "C++" {
namespace {

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }

// exclusive scan of n flags or counts into pos (the tiled form; tile_scratch: scan_scratch_count(n) words); *total_host =
// their sum.  Synchronises.
hipError_t scan_flags(hipStream_t st, const uint32_t *flags, int64_t n, uint32_t *pos, uint32_t *tile_scratch, uint32_t *d_total,
                      uint32_t *total_host) {
    scan_tiled(st, flags, n, 0u, pos, d_total, tile_scratch);
    hipError_t e = launch_error();
    if (e == hipSuccess) e = hipMemcpyAsync(total_host, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

// THE place where the problem's observation list is replaced (cull, adopt_visibility, filter_observations): n_obs
// observations in uv / pt_idx, their cameras in *cam_idx, or (cam_idx NULL) expanded here from the device row pointer `rows`
// over the problem's cameras.  Two phases: cam_idx, a workspace for the new count and whatever the caller queues behind them
// (`more`) are allocated and queued first; the problem is touched only after the stream has synchronised without error:
// then the four arrays move in, n_obs is set and what was derived from the old list goes.  A failure leaves the problem as it was.
template <class More>
int install_observations(c2b_problem *p, const char *who, int64_t n_obs, DevBuf<double> &uv, DevBuf<uint32_t> &pt_idx,
                         DevBuf<uint32_t> *cam_idx, const uint64_t *rows, More &&more) {
    DevBuf<uint32_t> expanded;
    DevBuf<char> ws;
    int rc = C2B_OK;
    hipError_t e = cam_idx ? hipSuccess : expanded.alloc((size_t)n_obs);
    if (e == hipSuccess && !cam_idx) rc = c2b_expand_rows(rows, p->n_cam, 0, n_obs, expanded, p->stream);
    if (e == hipSuccess && !rc) rc = new_workspace(ws, n_obs, p->stream);
    if (e == hipSuccess && !rc) e = more();
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(p->stream);
    if (rc || e != hipSuccess) {
        (void)hipStreamSynchronize(p->stream);               // no temporary may be freed while queued work still uses it
        return rc ? rc : fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    }
    p->uv = std::move(uv); p->pt_idx = std::move(pt_idx); p->cam_idx = std::move(cam_idx ? *cam_idx : expanded); p->ws = std::move(ws);
    p->n_obs = n_obs;
    drop_rows(p);
    return C2B_OK;
}
inline hipError_t nothing_more() { return hipSuccess; }

}  // namespace
}  // extern "C++"

// mode 0: cull() = both passes to a fixed point; 1: largest_connected_component() once; 2: remove_singletons() once
static int cull_impl(c2b_problem *p, int faithful, int mode) {
    NEED_UPLOADED(p, "problem_cull");
    if (p->n_obs >= ((int64_t)1 << 32) || p->n_cam + p->n_pts >= ((int64_t)1 << 32))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_cull: more than 2^32 observations or entities");
    free_dense(p);
    hipStream_t st = p->stream;
    const int64_t nc0 = p->n_cam, np0 = p->n_pts, no0 = p->n_obs;
    const int64_t nodes0 = nc0 + np0, big0 = std::max(std::max(nc0, np0), no0);
    // current graph (ping-pong pairs) + where everything came from
    DevBuf<uint32_t> cam[2], pt[2], eorig[2], corig[2], porig[2];
    DevBuf<uint32_t> parent, sets, size, keep_c, keep_p, keep_o, pos_c, pos_p, pos_o, tiles, total, deg, cnt;
    DevBuf<unsigned long long> best;
    hipError_t e = hipSuccess;
    // cam / pt are allocations of their own (one of each pair becomes the problem's index array); every other temporary
    // is a view into one arena
    for (int k = 0; k < 2; ++k) {
        if (e == hipSuccess) e = cam[k].alloc((size_t)no0);
        if (e == hipSuccess) e = pt[k].alloc((size_t)no0);
    }
    DevArena arena;
    auto temporaries = [&](auto &&each) {
        each(eorig[0], (size_t)no0); each(eorig[1], (size_t)no0); each(corig[0], (size_t)nc0); each(corig[1], (size_t)nc0);
        each(porig[0], (size_t)np0); each(porig[1], (size_t)np0);
        each(parent, (size_t)nodes0); each(sets, (size_t)nodes0); each(size, (size_t)nodes0);
        each(keep_c, (size_t)nc0); each(keep_p, (size_t)np0); each(keep_o, (size_t)no0);
        each(pos_c, (size_t)nc0); each(pos_p, (size_t)np0); each(pos_o, (size_t)no0);
        each(tiles, scan_scratch_count(big0)); each(best, (size_t)1); each(total, (size_t)1); each(deg, (size_t)nc0); each(cnt, (size_t)np0);
    };
    size_t arena_bytes = 0;
    temporaries([&](auto &b, size_t n) { arena_bytes += DevArena::room(b, n); });
    if (e == hipSuccess) e = arena.reserve(arena_bytes);
    if (e == hipSuccess) temporaries([&](auto &b, size_t n) { arena.carve(b, n); });
    if (e != hipSuccess) return fail(hip_code(e), "problem_cull: %s", hipGetErrorString(e));

    int cur = 0;
    int64_t nc = nc0, np = np0, no = no0;
    if (no) {
        e = hipMemcpyAsync(cam[0].ptr, p->cam_idx, 4 * (size_t)no, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pt[0].ptr, p->pt_idx, 4 * (size_t)no, hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_uf_init, dim3(blocks_of(no, kBlock)), dim3(kBlock), 0, st, eorig[0], no);   // iota
        hipLaunchKernelGGL(k_uf_init, dim3(blocks_of(nc, kBlock)), dim3(kBlock), 0, st, corig[0], nc);
        hipLaunchKernelGGL(k_uf_init, dim3(blocks_of(np, kBlock)), dim3(kBlock), 0, st, porig[0], np);
        e = launch_error();
    }

    // renumber by the keep flags currently in keep_c / keep_p / keep_o
    auto compact = [&]() -> hipError_t {
        uint32_t nc_new = 0, np_new = 0, no_new = 0;
        hipError_t s = scan_flags(st, keep_c, nc, pos_c, tiles, total, &nc_new);
        if (s == hipSuccess) s = scan_flags(st, keep_p, np, pos_p, tiles, total, &np_new);
        if (s == hipSuccess) s = scan_flags(st, keep_o, no, pos_o, tiles, total, &no_new);
        if (s != hipSuccess) return s;
        const int nxt = cur ^ 1;
        hipLaunchKernelGGL(k_cull_move_nodes, dim3(blocks_of(nc, kBlock)), dim3(kBlock), 0, st, keep_c, pos_c, nc, corig[cur], corig[nxt]);
        hipLaunchKernelGGL(k_cull_move_nodes, dim3(blocks_of(np, kBlock)), dim3(kBlock), 0, st, keep_p, pos_p, np, porig[cur], porig[nxt]);
        hipLaunchKernelGGL(k_cull_move_edges, dim3(blocks_of(no, kBlock)), dim3(kBlock), 0, st, keep_o, pos_o, no, cam[cur], pt[cur], eorig[cur],
                           pos_c, pos_p, cam[nxt], pt[nxt], eorig[nxt]);
        cur = nxt;
        nc = nc_new; np = np_new; no = no_new;
        return launch_error();
    };
    auto lcc_pass = [&]() -> hipError_t {
        if (nc == 0) return hipSuccess;                      // largest_connected_component returns self (:457-459)
        const int64_t nodes = nc + np, big = std::max(std::max(nc, np), no);
        hipError_t s = hipMemsetAsync(size.ptr, 0, 4 * (size_t)nodes, st);
        if (s == hipSuccess) s = hipMemsetAsync(best.ptr, 0, 8, st);
        if (s != hipSuccess) return s;
        hipLaunchKernelGGL(k_uf_init, dim3(blocks_of(nodes, kBlock)), dim3(kBlock), 0, st, parent, nodes);
        if (no) hipLaunchKernelGGL(k_uf_union, dim3(blocks_of(no, kBlock)), dim3(kBlock), 0, st, parent, cam[cur], pt[cur], no, (uint32_t)nc);
        hipLaunchKernelGGL(k_uf_flatten, dim3(blocks_of(nodes, kBlock)), dim3(kBlock), 0, st, parent, nodes, sets, size);
        hipLaunchKernelGGL(k_uf_largest, dim3(blocks_of(nodes, kBlock)), dim3(kBlock), 0, st, sets, size, nodes, best);
        hipLaunchKernelGGL(k_lcc_flags, dim3(blocks_of(big, kBlock)), dim3(kBlock), 0, st, sets, best, (uint32_t)nc,
                           (uint32_t)np, cam[cur], pt[cur], no, faithful ? 1 : 0, keep_c, keep_p, keep_o);
        s = launch_error();
        return s == hipSuccess ? compact() : s;
    };
    auto singleton_pass = [&]() -> hipError_t {
        const int64_t big = std::max(std::max(nc, np), no);
        hipError_t s = hipMemsetAsync(deg.ptr, 0, 4 * (size_t)(nc ? nc : 1), st);
        if (s == hipSuccess) s = hipMemsetAsync(cnt.ptr, 0, 4 * (size_t)(np ? np : 1), st);
        if (s != hipSuccess) return s;
        if (no) hipLaunchKernelGGL(k_degree, dim3(blocks_of(no, kBlock)), dim3(kBlock), 0, st, cam[cur], pt[cur], no, deg, cnt);
        hipLaunchKernelGGL(k_singleton_flags, dim3(blocks_of(big, kBlock)), dim3(kBlock), 0, st, deg, cnt, (uint32_t)nc,
                           (uint32_t)np, cam[cur], pt[cur], no, keep_c, keep_p, keep_o);
        s = launch_error();
        return s == hipSuccess ? compact() : s;
    };
    // culled = lcc().remove_singletons(); while the counts change: again (src/baproblem.rs:541-547)
    int64_t pnc = nc, pnp = np;
    if (e == hipSuccess && mode != 2) e = lcc_pass();
    if (e == hipSuccess && mode != 1) e = singleton_pass();
    while (mode == 0 && e == hipSuccess && (nc != pnc || np != pnp)) {
        pnc = nc; pnp = np;
        e = lcc_pass();
        if (e == hipSuccess) e = singleton_pass();
    }

    // gather the payloads once and swap them in
    DevBuf<double> n_cam15, n_bal9, n_camblk, n_cen4, n_pts4, n_uv;
    if (e == hipSuccess) e = n_cam15.alloc(15 * (size_t)nc);
    if (e == hipSuccess) e = n_bal9.alloc(9 * (size_t)nc);
    if (e == hipSuccess) e = n_camblk.alloc((size_t)cam_table_doubles(nc));
    if (e == hipSuccess) e = n_cen4.alloc(4 * (size_t)nc);
    if (e == hipSuccess) e = n_pts4.alloc(4 * (size_t)np);
    if (e == hipSuccess) e = n_uv.alloc(2 * (size_t)no);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(hip_code(e), "problem_cull: %s", hipGetErrorString(e));
    }
    auto gathers = [&]() -> hipError_t {
        auto gather = [&](const double *in, const uint32_t *orig, int64_t n, int width, double *out) {
            if (n) hipLaunchKernelGGL(k_gather_rows, dim3(blocks_of(n * width, kBlock)), dim3(kBlock), 0, st, in, orig, n, width, out);
        };
        gather(p->cam15, corig[cur], nc, 15, n_cam15);
        if (p->bal_valid) gather(p->bal9, corig[cur], nc, 9, n_bal9);
        gather(p->pts4, porig[cur], np, 4, n_pts4);
        gather(p->uv, eorig[cur], no, 2, n_uv);
        return launch_error();
    };
    if (const int rc = install_observations(p, "problem_cull", no, n_uv, pt[cur], &cam[cur], nullptr, gathers)) return rc;
    // the list is in; the entities, which cull alone replaces and renumbers
    p->cam15 = std::move(n_cam15); p->bal9 = std::move(n_bal9); p->camblk = std::move(n_camblk); p->cen4 = std::move(n_cen4);
    p->pts4 = std::move(n_pts4); p->n_cam = nc; p->n_pts = np;
    drop_constant(p);                                         // the survivors are renumbered
    entities_replaced(p);
    drop_priors(p);
    drop_lm_state(p);
    p->blk_valid = false;                                     // camblk is rebuilt on demand from the gathered cameras
    p->bal9_fresh = false;                                    // (bal9 was gathered only when it was the truth)
    return C2B_OK;
}

int c2b_problem_cull(c2b_problem *p, int faithful) { return cull_impl(p, faithful, 0); }
int c2b_problem_largest_connected_component(c2b_problem *p, int faithful) { return cull_impl(p, faithful, 1); }
int c2b_problem_remove_singletons(c2b_problem *p) { return cull_impl(p, 1, 2); }

int c2b_problem_adopt_visibility(c2b_problem *p) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_adopt_visibility");
    if (!p->dense_pt || !p->dense_uv || !p->dense_row)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_adopt_visibility: no pending visibility result");
    const int64_t n = p->dense_n;
    if (n >= ((int64_t)1 << 32)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_adopt_visibility: more than 2^32 observations");
    if (const int rc = install_observations(p, "problem_adopt_visibility", n, p->dense_uv, p->dense_pt, nullptr, p->dense_row, nothing_more)) return rc;
    free_dense(p);                                            // the pending result is spent (its row pointer; the lists were moved out)
    return C2B_OK;
    C2B_API_END("problem_adopt_visibility")
}

int c2b_problem_download_graph(c2b_problem *p, uint64_t *row_ptr, uint64_t *pt_idx) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_download_graph");
    if (!row_ptr || (p->n_obs && !pt_idx)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_download_graph: bad arguments");
    const int64_t n_cam = p->n_cam, n_obs = p->n_obs;
    // the point indices are widened to the host's u64 on the device and leave in ONE copy (r01-r02: a u32 copy into a
    // fresh host vector, then a serial widening loop over 19 M entries -- a third of the 120-ms download at --blocks 128)
    DevBuf<uint64_t> d_row, d_pt64;
    hipError_t e = d_row.alloc((size_t)n_cam + 1);
    if (e == hipSuccess && n_obs) e = d_pt64.alloc((size_t)n_obs);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rows_from_sorted, dim3(blocks_for(n_obs + 1)), dim3(kBlock), 0, p->stream, (const uint32_t *)p->cam_idx, n_obs,
                           n_cam, d_row);
        if (n_obs) hipLaunchKernelGGL(k_widen_u32, dim3(blocks_for(n_obs)), dim3(kBlock), 0, p->stream, (const uint32_t *)p->pt_idx, n_obs,
                                      d_pt64);
        e = launch_error();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(row_ptr, d_row.ptr, sizeof(uint64_t) * (size_t)(n_cam + 1), hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess && n_obs) e = hipMemcpyAsync(pt_idx, d_pt64.ptr, sizeof(uint64_t) * (size_t)n_obs, hipMemcpyDeviceToHost, p->stream);
    hipError_t e2 = hipStreamSynchronize(p->stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(hip_code(e), "problem_download_graph: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_download_graph")
}

// The bridge from a problem that was BORN on the device (layout, visibility loop, cull, file read) to the Level-0
// launchers: the resident arrays -- or the slice that belongs to the camera range [cam_lo, cam_hi) -- copied device to
// device into buffers the caller owns.  No byte crosses PCIe but the two row-pointer words that size the slice.
__global__ __launch_bounds__(256) void k_rows_rebase(const uint64_t *__restrict__ in, int64_t n, uint64_t base, uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i] - base;
}

int c2b_problem_export_device(c2b_problem *p, int64_t cam_lo, int64_t cam_hi, double *cam15, double *pts4, uint64_t *row_ptr,
                              uint32_t *pt_idx, double *uv, int64_t *obs_lo, int64_t *n_obs_slice) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_export_device");
    if (cam_lo < 0 || cam_hi < cam_lo || cam_hi > p->n_cam)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_export_device: camera range [%lld, %lld) outside [0, %lld]", (long long)cam_lo,
                    (long long)cam_hi, (long long)p->n_cam);
    int rc = ensure_rows(p);
    if (rc) return rc;
    hipStream_t st = p->stream;
    uint64_t ends[2] = {0, 0};
    if (p->n_obs) {
        HIP_TRY(hipMemcpyAsync(&ends[0], p->rows_ptr + cam_lo, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&ends[1], p->rows_ptr + cam_hi, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const int64_t o0 = (int64_t)ends[0], n = (int64_t)(ends[1] - ends[0]), nc = cam_hi - cam_lo;
    if (obs_lo) *obs_lo = o0;
    if (n_obs_slice) *n_obs_slice = n;
    if (cam15 && nc) HIP_TRY(hipMemcpyAsync(cam15, p->cam15 + 15 * cam_lo, sizeof(double) * 15 * (size_t)nc, hipMemcpyDeviceToDevice, st));
    if (pts4 && p->n_pts) HIP_TRY(hipMemcpyAsync(pts4, p->pts4, sizeof(double) * 4 * (size_t)p->n_pts, hipMemcpyDeviceToDevice, st));
    if (row_ptr) {
        if (p->n_obs) {
            hipLaunchKernelGGL(k_rows_rebase, dim3(blocks_of(nc + 1, 256)), dim3(256), 0, st, (const uint64_t *)(p->rows_ptr + cam_lo), nc + 1,
                               ends[0], row_ptr);
            LAUNCH_CHECK();
        } else {
            HIP_TRY(hipMemsetAsync(row_ptr, 0, sizeof(uint64_t) * (size_t)(nc + 1), st));
        }
    }
    if (pt_idx && n) HIP_TRY(hipMemcpyAsync(pt_idx, p->pt_idx + o0, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (uv && n) HIP_TRY(hipMemcpyAsync(uv, p->uv + 2 * o0, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return C2B_OK;
    C2B_API_END("problem_export_device")
}

// Stable compaction of CSR lists (point index, uv) by a keep mask, on the device: kept count per row -> row scan ->
// one wave per camera scatters in order.  The new row pointer goes to row_ptr_host; on success the three new lists are
// in row_new / pt_new / uv_new, *w = kept count (on failure what they hold is not a result).  Synchronises the problem's stream.
// stop_at: a kept count at which the caller wants no lists (the mask kept everything): pt_new / uv_new are then left empty.
static hipError_t compact_rows_on_device(c2b_problem *p, const uint64_t *d_row_old, const uint8_t *d_keep, const uint32_t *d_pt,
                                         const double *d_uv, int64_t n_cam, uint64_t *row_ptr_host, DevBuf<uint64_t> &row_new,
                                         DevBuf<uint32_t> &pt_new, DevBuf<double> &uv_new, int64_t *w, int64_t stop_at = -1) {
    DevBuf<uint64_t> d_tot;
    *w = 0;
    hipError_t e = d_tot.alloc((size_t)n_cam + 1);
    if (e == hipSuccess) e = row_new.alloc((size_t)n_cam + 1);
    if (e != hipSuccess) return e;
    const unsigned row_blocks = (unsigned)((n_cam + 3) / 4);
    if (n_cam) hipLaunchKernelGGL((k_keep_row_counts<RowSame, KeepByte>), dim3(row_blocks), dim3(256), 0, p->stream, d_row_old, RowSame{},
                                  KeepByte{d_keep}, d_pt, n_cam, d_tot.ptr);
    scan_short(p->stream, (const uint64_t *)d_tot, n_cam, (uint64_t)0, row_new.ptr, row_new.ptr + n_cam);      // cameras: one workgroup
    e = hipMemcpyAsync(row_ptr_host, row_new, sizeof(uint64_t) * (size_t)(n_cam + 1), hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return e;
    *w = (int64_t)row_ptr_host[n_cam];
    if (*w == stop_at) return hipSuccess;
    e = pt_new.alloc((size_t)*w);
    if (e == hipSuccess) e = uv_new.alloc(2 * (size_t)*w);
    if (e == hipSuccess && n_cam) {
        hipLaunchKernelGGL((k_keep_row_scatter<RowSame, KeepByte>), dim3(row_blocks), dim3(256), 0, p->stream, d_row_old,
                           (const uint64_t *)row_new, RowSame{}, KeepByte{d_keep}, d_pt, reinterpret_cast<const double2 *>(d_uv), n_cam,
                           pt_new.ptr, reinterpret_cast<double2 *>(uv_new.ptr));
        e = launch_error();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    return e;
}

// The resident list compacted by a keep mask of its n_old entries and swapped in (install_observations: cam_idx from the new
// row pointer, a workspace for the new count, swapped in only once the stream has synchronised without error).  A mask that
// keeps everything changes nothing and drops no cache.  *n_removed (may be NULL) is written on success alone.
static int compact_and_install(c2b_problem *p, const char *who, const uint8_t *d_keep, int64_t n_old, int64_t *n_removed) {
    DevBuf<uint64_t> row_new;
    DevBuf<uint32_t> pt_new;
    DevBuf<double> uv_new;
    std::vector<uint64_t> row_host((size_t)p->n_cam + 1);
    int64_t w = 0;
    const hipError_t e = compact_rows_on_device(p, p->rows_ptr, d_keep, p->pt_idx, p->uv, p->n_cam, row_host.data(), row_new, pt_new, uv_new, &w, n_old);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(p->stream);
        return fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    }
    if (w == n_old) return C2B_OK;
    const int rc = install_observations(p, who, w, uv_new, pt_new, nullptr, row_new, nothing_more);
    if (rc) return rc;
    if (n_removed) *n_removed = n_old - w;
    return C2B_OK;
}

// The outlier filter: the residual predicate over the resident list, a stable compaction of (pt_idx, uv) by its
// mask and its installation (compact_and_install).  The entities do not move: cameras, points, both counts, the masks, the
// loss, the preconditioner, the checkpoint and the LM scratch stay; what was derived from the list (drop_rows) goes.
int c2b_problem_filter_observations(c2b_problem *p, double max_error, int flags, int64_t *n_removed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_filter_observations");
    if (n_removed) *n_removed = 0;
    if (!(max_error >= 0.0)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_filter_observations: max_error must be >= 0 (+inf keeps every finite residual)");
    if (flags & ~C2B_FILTER_IN_FRONT)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_filter_observations: unknown flag bits 0x%x", (unsigned)(flags & ~C2B_FILTER_IN_FRONT));
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_filter_observations: a shard is not filtered alone (its list is a slice of the whole one)");
    if (!p->n_obs) return C2B_OK;
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    const int64_t n_old = p->n_obs;
    DevBuf<uint8_t> keep;
    const hipError_t e = keep.alloc((size_t)n_old);
    if (e != hipSuccess) return fail(hip_code(e), "problem_filter_observations: %s", hipGetErrorString(e));
    rc = c2b_residual_keep_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv, n_old, max_error, flags, keep, p->stream);
    if (rc) {
        (void)hipStreamSynchronize(p->stream);
        return rc;
    }
    return compact_and_install(p, "problem_filter_observations", keep, n_old, n_removed);
    C2B_API_END("problem_filter_observations")
}

// Consensus triangulation: c2b_triangulate_consensus_rows over the cached transpose, as
// c2b_problem_triangulate_points runs c2b_triangulate_rows -- only pts4 changes, nothing the problem caches is derived from
// the points -- and, with C2B_TRI_DROP_OUTLIERS, the filter's compaction of the list by the pass's inlier mask: then what was
// derived from the list goes, and nothing else.  The points have moved by the time the list is compacted.
int c2b_problem_triangulate_consensus(c2b_problem *p, double min_angle, double max_error, int min_inliers, int max_hypotheses, int flags,
                                      uint8_t *status, int32_t *hyp, uint8_t *inlier, int64_t *counts, int64_t *n_removed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_triangulate_consensus");
    if (!good_min_angle(min_angle)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_consensus: min_angle must lie in [0, pi/2] radians");
    if (!good_tri_max_error(max_error)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_consensus: max_error must be finite and >= 0");
    if (min_inliers < 2) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_consensus: min_inliers must be at least 2");
    if (max_hypotheses < 1 || max_hypotheses > kTrcSample)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_consensus: max_hypotheses must lie in [1, %d]", kTrcSample);
    if (flags & ~C2B_TRI_DROP_OUTLIERS)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_consensus: unknown flag bits 0x%x", (unsigned)(flags & ~C2B_TRI_DROP_OUTLIERS));
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_consensus: a shard is not triangulated alone (a point's observations span every rank)");
    if (n_removed) *n_removed = 0;
    const int64_t np = p->n_pts, n_old = p->n_obs;
    StatusReport rep(kTrcKinds);
    if (!n_old) {                                            // no observation: every point has too few, nothing is read or written
        if (hyp && np) std::fill(hyp, hyp + np, (int32_t)-1);
        return rep.all_have(kTriTooFew, np, status, counts);
    }
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (!rc) rc = ensure_transpose(p);
    if (rc) return rc;
    DevBuf<uint8_t> d_inlier;
    DevBuf<int32_t> d_hyp;
    hipError_t e = rep.alloc(np);
    if (e == hipSuccess) e = d_inlier.alloc((size_t)n_old);
    if (e == hipSuccess) e = d_hyp.alloc((size_t)np);
    if (e != hipSuccess) return fail(hip_code(e), "problem_triangulate_consensus: allocation: %s", hipGetErrorString(e));
    rc = c2b_triangulate_consensus_rows(p->camblk, p->pts4, np, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, n_old, min_angle, max_error, min_inliers,
                                        max_hypotheses, p->pmask, rep.d_status, d_hyp, nullptr, d_inlier, rep.d_counts, p->stream);
    if (!rc && hyp) e = hipMemcpyAsync(hyp, d_hyp, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, p->stream);
    if (!rc && e == hipSuccess && inlier) e = hipMemcpyAsync(inlier, d_inlier, (size_t)n_old, hipMemcpyDeviceToHost, p->stream);
    rc = rep.read_back("problem_triangulate_consensus", p->stream, rc, e, np, status, counts);
    if (rc || !(flags & C2B_TRI_DROP_OUTLIERS)) return rc;
    return compact_and_install(p, "problem_triangulate_consensus", d_inlier, n_old, n_removed);     // the filter's compaction, by the inlier mask
    C2B_API_END("problem_triangulate_consensus")
}

// Consensus resection: c2b_resect_consensus_rows over the row structure, in place on bal9 made the truth as
// c2b_problem_resect_cameras makes it -- the cameras moved, so their caches go -- and, with C2B_RES_DROP_OUTLIERS, the filter's
// compaction of the list by the pass's inlier mask, as c2b_problem_triangulate_consensus does it.  The cameras have moved by the
// time the list is compacted.
int c2b_problem_resect_consensus(c2b_problem *p, double max_error, int min_inliers, double min_gap, int max_hypotheses, int flags,
                                 uint8_t *status, int32_t *hyp, int32_t *n_inl, uint8_t *inlier, int64_t *counts, int64_t *n_removed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_resect_consensus");
    if (!good_tri_max_error(max_error)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_consensus: max_error must be finite and >= 0");
    if (min_inliers < kResMinPoints)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_consensus: min_inliers must be at least %d", kResMinPoints);
    if (!good_min_gap(min_gap)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_consensus: min_gap must lie in [0, 1)");
    if (max_hypotheses < 1 || max_hypotheses > kRrcSample)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_consensus: max_hypotheses must lie in [1, %d]", kRrcSample);
    if (flags & ~C2B_RES_DROP_OUTLIERS)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_consensus: unknown flag bits 0x%x", (unsigned)(flags & ~C2B_RES_DROP_OUTLIERS));
    if (p->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_consensus: a shard is not resected alone");
    if (n_removed) *n_removed = 0;
    const int64_t nc = p->n_cam, n_old = p->n_obs;
    StatusReport rep(kRrcKinds);
    if (!n_old) {                                            // no observation: every camera has too few, nothing is read or written
        if (hyp && nc) std::fill(hyp, hyp + nc, (int32_t)-1);
        if (n_inl && nc) std::fill(n_inl, n_inl + nc, (int32_t)0);
        return rep.all_have(kResTooFew, nc, status, counts);
    }
    int rc = ensure_rows(p);
    if (rc) return rc;
    DevBuf<uint8_t> d_inlier;
    DevBuf<int32_t> d_hyp, d_ninl;
    hipError_t e = rep.alloc(nc);
    if (e == hipSuccess) e = d_inlier.alloc((size_t)n_old);
    if (e == hipSuccess) e = d_hyp.alloc((size_t)nc);
    if (e == hipSuccess) e = d_ninl.alloc((size_t)nc);
    if (e != hipSuccess) return fail(hip_code(e), "problem_resect_consensus: allocation: %s", hipGetErrorString(e));
    hipStream_t st = p->stream;
    if ((rc = bal9_edit_begin(p))) return rc;                // state mode: the pass works on to_vec(cam15)
    rc = c2b_resect_consensus_rows(p->bal9, p->pts4, p->rows_ptr, nc, p->pt_idx, p->uv, n_old, max_error, min_inliers, min_gap, max_hypotheses,
                                   p->cmask, rep.d_status, d_hyp, d_ninl, d_inlier, rep.d_counts, st);
    rc = bal9_edit_end(p, rc);
    if (!rc && hyp) e = hipMemcpyAsync(hyp, d_hyp, sizeof(int32_t) * (size_t)nc, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess && n_inl) e = hipMemcpyAsync(n_inl, d_ninl, sizeof(int32_t) * (size_t)nc, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess && inlier) e = hipMemcpyAsync(inlier, d_inlier, (size_t)n_old, hipMemcpyDeviceToHost, st);
    rc = rep.read_back("problem_resect_consensus", st, rc, e, nc, status, counts);
    if (rc || !(flags & C2B_RES_DROP_OUTLIERS)) return rc;
    return compact_and_install(p, "problem_resect_consensus", d_inlier, n_old, n_removed);     // the filter's compaction, by the inlier mask
    C2B_API_END("problem_resect_consensus")
}

int c2b_problem_visibility_pairs_compact(c2b_problem *p, int64_t n_pairs, const uint32_t *cam_idx, const uint32_t *pt_idx,
                                         double max_dist, uint64_t *row_ptr) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_visibility_pairs_compact");
    if (n_pairs < 0 || !row_ptr || (n_pairs && (!cam_idx || !pt_idx)))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_pairs_compact: bad arguments");
    for (int64_t i = 0; i < n_pairs; ++i) {
        if (cam_idx[i] >= (uint64_t)p->n_cam || pt_idx[i] >= (uint64_t)p->n_pts)
            return fail(C2B_ERR_INDEX_OUT_OF_RANGE, "problem_visibility_pairs_compact: pair %lld out of range", (long long)i);
        if (i && cam_idx[i] < cam_idx[i - 1])
            return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_pairs_compact: cam_idx must be non-decreasing (pair %lld)", (long long)i);
    }
    int rc = ensure_camblk(p);
    if (rc) return rc;
    free_dense(p);
    const int64_t n_cam = p->n_cam;
    const size_t n = (size_t)(n_pairs ? n_pairs : 1);
    DevBuf<uint32_t> d_c, d_p, d_pt_new;
    DevBuf<double> d_uv, d_uv_new;
    DevBuf<uint8_t> d_k;
    DevBuf<uint64_t> d_row, d_row_new;
    int64_t w = 0;
    hipError_t e = d_c.alloc(n);
    if (e == hipSuccess) e = d_p.alloc(n);
    if (e == hipSuccess) e = d_uv.alloc(2 * n);
    if (e == hipSuccess) e = d_k.alloc(n);
    if (e == hipSuccess) e = d_row.alloc((size_t)n_cam + 1);
    if (e == hipSuccess && n_pairs) e = hipMemcpyAsync(d_c, cam_idx, sizeof(uint32_t) * n, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess && n_pairs) e = hipMemcpyAsync(d_p, pt_idx, sizeof(uint32_t) * n, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) {
        if (n_pairs) rc = c2b_visibility_pairs(p->camblk, p->pts4, d_c, d_p, n_pairs, max_dist, d_uv, d_k, p->stream);
        if (!rc) {
            hipLaunchKernelGGL(k_rows_from_sorted, dim3(blocks_for(n_pairs + 1)), dim3(kBlock), 0, p->stream, (const uint32_t *)d_c,
                               n_pairs, n_cam, d_row);
            e = launch_error();
            if (e == hipSuccess)
                e = compact_rows_on_device(p, d_row, d_k, d_p, d_uv, n_cam, row_ptr, d_row_new, d_pt_new, d_uv_new, &w);
        }
    }
    if (rc || e != hipSuccess) (void)hipStreamSynchronize(p->stream);
    if (!rc && e == hipSuccess) {                 // becomes the pending visibility result (fetch with _dense_fetch)
        p->dense_row = std::move(d_row_new); p->dense_pt = std::move(d_pt_new); p->dense_uv = std::move(d_uv_new); p->dense_n = w;
    }
    if (rc) return rc;
    if (e != hipSuccess) return fail(hip_code(e), "problem_visibility_pairs_compact: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_visibility_pairs_compact")
}

// A statistics record's extent (stats[6..11]: min and max) and max_dist -> the cell grid over x / z.  Cells are a hair
// wider than max_dist so that rounding in the cell arithmetic can never separate two positions within max_dist by more
// than one cell; they double until there are at most 2^24 of them (wider cells stay correct, only slower).
static int cell_grid_from_stats(const double *stats, double max_dist, const char *who, CellGrid *g, int64_t *n_cells) {
    g->x0 = stats[6]; g->z0 = stats[8];
    const double ex = stats[9] - stats[6], ez = stats[11] - stats[8];
    double cs = (max_dist > 0.0 ? max_dist : 1.0) * (1.0 + 0x1.0p-20);
    if (!(ex >= 0.0) || !(ez >= 0.0) || !std::isfinite(ex) || !std::isfinite(ez) || !std::isfinite(cs))
        return fail(C2B_ERR_INVALID_ARGUMENT, "%s: non-finite coordinates", who);
    auto cells = [&](double c) { return (std::floor(ex / c) + 1.0) * (std::floor(ez / c) + 1.0); };
    while (cells(cs) > (double)(1 << 24)) cs *= 2.0;
    g->inv_cs = 1.0 / cs;
    g->ncx = (int)std::floor(ex / cs) + 1; g->ncz = (int)std::floor(ez / cs) + 1;
    *n_cells = (int64_t)g->ncx * g->ncz;
    return C2B_OK;
}

// The cell list of n > 0 positions (32-byte rows) on that grid: count, exclusive scan (start[n_cells] = n), fill.  `counts`
// [n_cells + 1] is zero on entry -- the caller's memset -- and holds the fill's cursors afterwards.  Synchronises (scan_flags).
static int build_cell_list(hipStream_t st, const char *who, const double4 *pos4, int64_t n, const CellGrid &g, int64_t n_cells,
                           uint32_t *cell_of, uint32_t *counts, uint32_t *start, uint32_t *sorted, uint32_t *tiles, uint32_t *total) {
    hipLaunchKernelGGL(k_cells_assign, dim3(blocks_of(n, 256)), dim3(256), 0, st, pos4, n, g, cell_of, counts);
    uint32_t n_sorted = 0;
    hipError_t e = scan_flags(st, counts, n_cells + 1, start, tiles, total, &n_sorted);
    if (e == hipSuccess && (int64_t)n_sorted != n) return fail(C2B_ERR_HIP, "%s: cell counts do not add up", who);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 4 * (size_t)(n_cells + 1), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bucket_fill<uint32_t>, dim3(blocks_of(n, 256)), dim3(256), 0, st, (const uint32_t *)cell_of, n, n_cells, (const uint32_t *)start, counts, sorted);
        e = launch_error();
    }
    if (e != hipSuccess) return fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    return C2B_OK;
}

// ---- landmark merging (merge_kernels.hpp) --------------------------------------------------------------------
static bool good_merge_length(double v) { return v >= 0.0 && std::isfinite(v); }       // (a NaN fails the first)

// the double whose merge_order_key is k
static double merge_key_value(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    std::memcpy(&v, &u, sizeof v);
    return v;
}

// The x / z cell list of a point table for a search within `radius` (merging, re-matching): the grid comes from the extent of
// the finite points, with cells of radius (1 + 2^-20) doubled as cell_grid_from_stats doubles them, so a result never depends
// on it.  Its temporaries and whatever else the caller names in `extra` (called with the each(buffer, count) of the arena's two
// passes) are ONE allocation, freed with the object: the caller synchronises before it lets go of it.
extern "C++" {
struct PointCells {
    CellGrid g;
    DevArena arena;
    DevBuf<uint32_t> cell_of, cnt, start, sorted, tiles, total;
    DevBuf<unsigned long long> ext;
};
// radius_of(stats): the radius from the extent (stats[6..11] as a statistics record holds it; all 0 without a finite point)
template <class Radius, class Extra>
static int build_point_cells_by(hipStream_t st, const char *who, const double4 *pos4, int64_t n_pts, Radius &&radius_of, PointCells &pc, Extra &&extra) {
    // the extent of the points -> the cell grid
    const unsigned long long ext0[4] = {~0ull, ~0ull, 0ull, 0ull};
    unsigned long long ext_h[4] = {0, 0, 0, 0};
    HIP_TRY(pc.ext.alloc(4));
    HIP_TRY(hipMemcpyAsync(pc.ext.ptr, ext0, sizeof ext0, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_merge_extent, dim3(std::min(blocks_of(n_pts, 256), 1024u)), dim3(256), 0, st, pos4, n_pts, pc.ext.ptr);
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(ext_h, pc.ext.ptr, sizeof ext_h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double stats[C2B_STATS_DOUBLES] = {0.0};
    if (ext_h[2] != 0ull) {                                  // (no finite point: one cell at the origin, and no pair)
        stats[6] = merge_key_value(ext_h[0]); stats[8] = merge_key_value(ext_h[1]);
        stats[9] = merge_key_value(ext_h[2]); stats[11] = merge_key_value(ext_h[3]);
    }
    int64_t n_cells = 0;
    int rc = cell_grid_from_stats(stats, radius_of((const double *)stats), who, &pc.g, &n_cells);
    if (rc) return rc;
    auto temporaries = [&](auto &&each) {
        each(pc.cell_of, (size_t)n_pts); each(pc.cnt, (size_t)(n_cells + 1)); each(pc.start, (size_t)(n_cells + 1));
        each(pc.sorted, (size_t)n_pts); each(pc.tiles, scan_scratch_count(n_cells + 1)); each(pc.total, (size_t)1);
        extra(each);
    };
    size_t arena_bytes = 0;
    temporaries([&](auto &b, size_t n) { arena_bytes += DevArena::room(b, n); });
    const hipError_t ea = pc.arena.reserve(arena_bytes);
    if (ea != hipSuccess) return fail(hip_code(ea), "%s: %s", who, hipGetErrorString(ea));
    temporaries([&](auto &b, size_t n) { pc.arena.carve(b, n); });
    HIP_TRY(hipMemsetAsync(pc.cnt.ptr, 0, 4 * (size_t)(n_cells + 1), st));
    rc = build_cell_list(st, who, pos4, n_pts, pc.g, n_cells, pc.cell_of, pc.cnt, pc.start, pc.sorted, pc.tiles, pc.total);
    if (rc) (void)hipStreamSynchronize(st);
    return rc;
}
template <class Extra>
static int build_point_cells(hipStream_t st, const char *who, const double4 *pos4, int64_t n_pts, double radius, PointCells &pc, Extra &&extra) {
    return build_point_cells_by(st, who, pos4, n_pts, [radius](const double *) { return radius; }, pc, extra);
}
}  // extern "C++"

// One round's partner choice over a point-major transpose: the cell list over x / z is built here (build_point_cells).  The
// temporaries are freed on return, so the call synchronises `stream` as a scan does.
int c2b_merge_partner_rows(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                           const uint32_t *cam_of, const double *uv_obs, int64_t n_obs, double radius, double max_error,
                           const uint8_t *pt_held, int32_t *partner, uint8_t *status, int64_t *counts, void *stream) {
    C2B_API_BEGIN
    if (!good_merge_length(radius)) return fail(C2B_ERR_INVALID_ARGUMENT, "merge_partner_rows: radius must be finite and >= 0");
    if (!good_merge_length(max_error)) return fail(C2B_ERR_INVALID_ARGUMENT, "merge_partner_rows: max_error must be finite and >= 0");
    if (n_pts < 0 || n_pts >= ((int64_t)1 << 31)) return fail(C2B_ERR_INVALID_ARGUMENT, "merge_partner_rows: n_pts out of range");
    if (n_obs < 0 || n_obs > (int64_t)0x7fffffff - 64)        // (a row's length and its chunk offsets are ints in the kernel)
        return fail(C2B_ERR_INVALID_ARGUMENT, "merge_partner_rows: n_obs out of range");
    if (!counts || (n_pts && (!pts4 || !pt_row_ptr || !partner || !status))) return fail(C2B_ERR_INVALID_ARGUMENT, "merge_partner_rows: NULL argument");
    if (!aligned16(camblk) || !aligned16(pts4) || !aligned16(uv_obs) || !aligned8(pt_row_ptr) || !aligned8(counts) ||
        (reinterpret_cast<uintptr_t>(obs_of) & 3) || (reinterpret_cast<uintptr_t>(cam_of) & 3) || (reinterpret_cast<uintptr_t>(partner) & 3))
        return fail(C2B_ERR_INVALID_ARGUMENT, "merge_partner_rows: misaligned pointer");
    hipStream_t st = S(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * kMergeKinds, st));
    if (!n_pts) return C2B_OK;
    const double4 *pos4 = reinterpret_cast<const double4 *>(pts4);
    PointCells cells;
    const int rc = build_point_cells(st, "merge_partner_rows", pos4, n_pts, radius, cells, [](auto &&) {});
    if (rc) return rc;
    const CellGrid g = cells.g;
    const DevBuf<uint32_t> &startb = cells.start, &sorted = cells.sorted;
    hipLaunchKernelGGL(k_merge_partner, dim3(blocks_for(n_pts, kMrgWaves)), dim3(kMrgBlock), 0, st, camblk, pos4, n_pts, pt_row_ptr, obs_of,
                       cam_of, reinterpret_cast<const double2 *>(uv_obs), g, (const uint32_t *)startb, (const uint32_t *)sorted,
                       radius * radius, max_error * max_error, pt_held, partner, status, reinterpret_cast<unsigned long long *>(counts));
    const hipError_t el = launch_error(), es = hipStreamSynchronize(st);          // the arena is freed on return
    if (el != hipSuccess || es != hipSuccess)
        return fail(hip_code(el != hipSuccess ? el : es), "merge_partner_rows: %s", hipGetErrorString(el != hipSuccess ? el : es));
    return C2B_OK;
    C2B_API_END("merge_partner_rows")
}

// Merging on the resident problem: per round the partner pass over the cached transpose, the mutual pairs
// applied to pts4, and pt_idx rewritten through the round's map.  The entities do not move and nothing is renumbered: cameras,
// both counts, the masks, the priors, the loss, the preconditioner, the checkpoint and the LM scratch stay; after a round
// that merged, what was derived from the list (drop_rows) goes, as after a filter that removed something.
int c2b_problem_merge_points(c2b_problem *p, double radius, double max_error, int rounds, int32_t *merged_into, int64_t *n_merged,
                             int *rounds_run) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_merge_points");
    if (!good_merge_length(radius)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_merge_points: radius must be finite and >= 0");
    if (!good_merge_length(max_error)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_merge_points: max_error must be finite and >= 0");
    if (rounds < 1) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_merge_points: rounds must be at least 1");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_merge_points: a shard is not merged alone (a point's observations span every rank)");
    const int64_t np = p->n_pts;
    if (np >= ((int64_t)1 << 31)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_merge_points: too many points");
    if (n_merged) *n_merged = 0;
    if (rounds_run) *rounds_run = 0;
    if (merged_into)
        for (int64_t i = 0; i < np; ++i) merged_into[i] = (int32_t)i;
    if (!p->n_obs || !np) return C2B_OK;                     // no observation: every point is unobserved, nothing is launched
    hipStream_t st = p->stream;
    DevBuf<uint8_t> held, status;
    DevBuf<int32_t> partner;
    DevBuf<uint32_t> into, map;
    DevBuf<int64_t> counts;
    DevBuf<unsigned long long> moved;
    const bool any_held = p->pmask || p->pxw;
    hipError_t e = status.alloc((size_t)np);
    if (e == hipSuccess) e = partner.alloc((size_t)np);
    if (e == hipSuccess) e = into.alloc((size_t)np);
    if (e == hipSuccess) e = counts.alloc(kMergeKinds);
    if (e == hipSuccess) e = moved.alloc(1);
    if (e == hipSuccess && any_held) e = held.alloc((size_t)np);
    if (e == hipSuccess && merged_into) e = map.alloc((size_t)np);
    if (e != hipSuccess) return fail(hip_code(e), "problem_merge_points: allocation: %s", hipGetErrorString(e));
    if (any_held) {
        hipLaunchKernelGGL(k_merge_held, dim3(blocks_of(np, 256)), dim3(256), 0, st, np, (const uint8_t *)p->pmask, (const double *)p->pxw, held.ptr);
        LAUNCH_CHECK();
    }
    int64_t total = 0;
    int run = 0;
    int rc = C2B_OK;
    while (run < rounds) {
        rc = ensure_camblk(p);
        if (!rc) rc = ensure_rows(p);
        if (!rc) rc = ensure_transpose(p);
        if (!rc) rc = c2b_merge_partner_rows(p->camblk, p->pts4, np, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, p->n_obs, radius, max_error,
                                             any_held ? held.ptr : nullptr, partner, status, counts, st);
        if (rc) break;
        unsigned long long m = 0;
        e = hipMemsetAsync(moved.ptr, 0, 8, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_merge_apply, dim3(blocks_of(np, 256)), dim3(256), 0, st, reinterpret_cast<double4 *>(p->pts4.ptr), np,
                               (const uint64_t *)p->nt_ptr, (const int32_t *)partner, into.ptr, moved.ptr);
            e = launch_error();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&m, moved.ptr, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        ++run;
        if (!m) break;                                       // nothing merged: the list, the points and every cache are as they were
        hipLaunchKernelGGL(k_merge_remap, dim3(blocks_of(p->n_obs, 256)), dim3(256), 0, st, p->pt_idx.ptr, p->n_obs, (const uint32_t *)into);
        if (merged_into) {
            if (!total) e = hipMemcpyAsync(map.ptr, into.ptr, sizeof(uint32_t) * (size_t)np, hipMemcpyDeviceToDevice, st);
            else hipLaunchKernelGGL(k_merge_remap, dim3(blocks_of(np, 256)), dim3(256), 0, st, map.ptr, np, (const uint32_t *)into);
        }
        const hipError_t el = launch_error();
        if (e == hipSuccess) e = el;
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess) e = es;
        drop_rows(p);                                        // pt_idx changed: rows' tiles, the transpose and the solve buffers go
        if (e != hipSuccess) break;
        total += (int64_t)m;
    }
    if (!rc && e == hipSuccess && merged_into && total)
        e = hipMemcpy(merged_into, map.ptr, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost);
    if (rc || e != hipSuccess) (void)hipStreamSynchronize(st);
    if (n_merged) *n_merged = total;
    if (rounds_run) *rounds_run = run;
    if (rc) return rc;
    if (e != hipSuccess) return fail(hip_code(e), "problem_merge_points: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_merge_points")
}

// ---- guided re-matching (rematch_kernels.hpp) ------------------------------------------------------------------
// The choice and its resolution over a camera-major list, given the filter's mask of it (`fits`) and the points that may be
// judged or assigned (`pt_trusted`; NULL: every finite point).  The cell list over x / z is built here (build_point_cells);
// the temporaries are freed on return, so the call synchronises `stream` as c2b_merge_partner_rows does.
int c2b_rematch_rows(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx,
                     const double *uv_obs, int64_t n_obs, const uint8_t *fits, const uint8_t *pt_trusted, double radius, double max_error,
                     int32_t *choice, uint8_t *status, int64_t *counts, void *stream) {
    C2B_API_BEGIN
    if (!good_merge_length(radius)) return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: radius must be finite and >= 0");
    if (!good_merge_length(max_error)) return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: max_error must be finite and >= 0");
    if (n_pts < 0 || n_pts >= ((int64_t)1 << 31)) return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: n_pts out of range");
    if (n_cam < 0 || n_cam >= ((int64_t)1 << 32)) return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: n_cam out of range");
    if (n_obs < 0 || n_obs > (int64_t)0x7fffffff - 64)        // (a row's length and its chunk offsets are ints in the kernel)
        return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: n_obs out of range");
    if (n_obs && (!n_pts || !n_cam)) return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: observations without points or cameras");
    if (!counts || (n_obs && (!camblk || !pts4 || !row_ptr || !pt_idx || !uv_obs || !fits || !choice || !status)))
        return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: NULL argument");
    if (!aligned16(camblk) || !aligned16(pts4) || !aligned16(uv_obs) || !aligned8(row_ptr) || !aligned8(counts) ||
        (reinterpret_cast<uintptr_t>(pt_idx) & 3) || (reinterpret_cast<uintptr_t>(choice) & 3))
        return fail(C2B_ERR_INVALID_ARGUMENT, "rematch_rows: misaligned pointer");
    hipStream_t st = S(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * kRematchKinds, st));
    if (!n_obs) return C2B_OK;
    const double4 *pos4 = reinterpret_cast<const double4 *>(pts4);
    PointCells cells;
    DevBuf<unsigned long long> r2bits;
    DevBuf<uint8_t> finite;
    const int rc = build_point_cells(st, "rematch_rows", pos4, n_pts, radius, cells, [&](auto &&each) {
        each(r2bits, (size_t)n_obs);
        if (!pt_trusted) each(finite, (size_t)n_pts);
    });
    if (rc) return rc;
    if (!pt_trusted) {
        hipLaunchKernelGGL(k_rematch_trusted, dim3(blocks_of(n_pts, 256)), dim3(256), 0, st, pos4, n_pts, (const uint64_t *)nullptr,
                           (const uint32_t *)nullptr, (const uint8_t *)nullptr, 0, finite.ptr);
        pt_trusted = finite.ptr;
    }
    hipLaunchKernelGGL(k_rematch_choose, dim3(blocks_for(n_cam, kRmtWaves)), dim3(kRmtBlock), 0, st, camblk, pos4, row_ptr, n_cam, pt_idx,
                       reinterpret_cast<const double2 *>(uv_obs), fits, pt_trusted, cells.g, (const uint32_t *)cells.start.ptr,
                       (const uint32_t *)cells.sorted.ptr, radius * radius, max_error * max_error, choice, r2bits.ptr, status);
    hipLaunchKernelGGL(k_rematch_resolve, dim3(blocks_for(n_cam, kRmtWaves)), dim3(kRmtBlock), 0, st, row_ptr, n_cam, (const int32_t *)choice,
                       (const unsigned long long *)r2bits.ptr, status, reinterpret_cast<unsigned long long *>(counts));
    const hipError_t el = launch_error(), es = hipStreamSynchronize(st);          // the arena is freed on return
    if (el != hipSuccess || es != hipSuccess)
        return fail(hip_code(el != hipSuccess ? el : es), "rematch_rows: %s", hipGetErrorString(el != hipSuccess ? el : es));
    return C2B_OK;
    C2B_API_END("rematch_rows")
}

// Re-matching on the resident problem: the filter's mask, the trusted points over the cached transpose, the
// choice, and -- when something was reassigned or removed -- the new labels in a list of their own, compacted by the keep mask
// as the filter compacts and swapped in (install_observations).  The entities do not move: cameras, points, both counts, the
// masks, the priors, the loss, the preconditioner, the checkpoint and the LM scratch stay; what was derived from the list
// (drop_rows) goes, and only after a call that changed it.  A failure leaves the problem as it was.
int c2b_problem_rematch_observations(c2b_problem *p, double radius, double max_error, int min_fits, uint8_t *status_out,
                                     int64_t *n_reassigned, int64_t *n_removed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_rematch_observations");
    if (!good_merge_length(radius)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_rematch_observations: radius must be finite and >= 0");
    if (!good_merge_length(max_error)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_rematch_observations: max_error must be finite and >= 0");
    if (min_fits < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_rematch_observations: min_fits must be >= 0");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_rematch_observations: a shard is not re-matched alone (a point's observations span every rank)");
    const int64_t np = p->n_pts, n_old = p->n_obs;
    if (np >= ((int64_t)1 << 31)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_rematch_observations: too many points");
    if (n_reassigned) *n_reassigned = 0;
    if (n_removed) *n_removed = 0;
    if (!n_old) return C2B_OK;                               // no observation: nothing is launched
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (!rc) rc = ensure_transpose(p);
    if (rc) return rc;
    hipStream_t st = p->stream;
    DevArena arena;
    DevBuf<uint8_t> fits, trusted, status, keep;
    DevBuf<int32_t> choice;
    DevBuf<int64_t> counts;
    auto temporaries = [&](auto &&each) {
        each(counts, (size_t)kRematchKinds); each(choice, (size_t)n_old); each(fits, (size_t)n_old); each(status, (size_t)n_old);
        each(keep, (size_t)n_old); each(trusted, (size_t)np);
    };
    size_t arena_bytes = 0;
    temporaries([&](auto &b, size_t n) { arena_bytes += DevArena::room(b, n); });
    hipError_t e = arena.reserve(arena_bytes);
    if (e != hipSuccess) return fail(hip_code(e), "problem_rematch_observations: allocation: %s", hipGetErrorString(e));
    temporaries([&](auto &b, size_t n) { arena.carve(b, n); });
    rc = c2b_residual_keep_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv, n_old, max_error, C2B_FILTER_IN_FRONT,
                                fits, st);
    if (!rc) {
        hipLaunchKernelGGL(k_rematch_trusted, dim3(blocks_of(np, 256)), dim3(256), 0, st, reinterpret_cast<const double4 *>(p->pts4.ptr), np,
                           (const uint64_t *)p->nt_ptr.ptr, (const uint32_t *)p->nt_obs.ptr, (const uint8_t *)fits.ptr, min_fits, trusted.ptr);
        rc = c2b_rematch_rows(p->camblk, p->pts4, np, p->rows_ptr, p->n_cam, p->pt_idx, p->uv, n_old, fits, trusted, radius, max_error, choice,
                              status, counts, st);
    }
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    int64_t cnt[kRematchKinds] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, counts.ptr, sizeof cnt, hipMemcpyDeviceToHost, st));
    if (status_out) HIP_TRY(hipMemcpyAsync(status_out, status.ptr, (size_t)n_old, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_reassigned) *n_reassigned = cnt[kRematchReassigned];
    if (n_removed) *n_removed = cnt[kRematchRemoved];
    if (!cnt[kRematchReassigned] && !cnt[kRematchRemoved]) return C2B_OK;          // the list and every cache are as they were
    DevBuf<uint32_t> pt_new;
    e = pt_new.alloc((size_t)n_old);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rematch_apply, dim3(blocks_of(n_old, 256)), dim3(256), 0, st, (const uint32_t *)p->pt_idx.ptr, n_old,
                           (const int32_t *)choice.ptr, (const uint8_t *)status.ptr, pt_new.ptr, keep.ptr);
        e = launch_error();
    }
    if (e == hipSuccess && !cnt[kRematchRemoved]) {          // labels alone: the new list takes the old one's place
        e = hipStreamSynchronize(st);
        if (e == hipSuccess) {
            p->pt_idx = std::move(pt_new);
            drop_rows(p);
            return C2B_OK;
        }
    }
    DevBuf<uint64_t> row_new;
    DevBuf<uint32_t> pt_kept;
    DevBuf<double> uv_kept;
    std::vector<uint64_t> row_host((size_t)p->n_cam + 1);
    int64_t w = 0;
    if (e == hipSuccess) e = compact_rows_on_device(p, p->rows_ptr, keep, pt_new, p->uv, p->n_cam, row_host.data(), row_new, pt_kept, uv_kept, &w);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        if (n_reassigned) *n_reassigned = 0;
        if (n_removed) *n_removed = 0;
        return fail(hip_code(e), "problem_rematch_observations: %s", hipGetErrorString(e));
    }
    rc = install_observations(p, "problem_rematch_observations", w, uv_kept, pt_kept, nullptr, row_new, nothing_more);
    if (rc) {
        if (n_reassigned) *n_reassigned = 0;
        if (n_removed) *n_removed = 0;
    }
    return rc;
    C2B_API_END("problem_rematch_observations")
}

// The generators' whole visibility loop (src/synthetic.rs:268-297, :353-378) on the device: candidates by a cell list
// (rstar's locate_within_distance), the sight line against the buildings (hits_building), the predicate, and the kept
// (point, uv) lists compacted per camera in ascending point index -- csrc/cell_kernels.hpp.  The result becomes the
// pending visibility result like c2b_problem_visibility_pairs_compact's (adopt / fetch it the same way); row_ptr (host,
// n_cam + 1) may be NULL.
int c2b_problem_visibility_within_distance(c2b_problem *p, double max_dist, int occlusion, double block_length, double block_inset,
                                           uint64_t *row_ptr) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_visibility_within_distance");
    if (!(max_dist >= 0.0) || (occlusion && !(block_length > 0.0)))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_within_distance: max_dist must be >= 0 (and block_length > 0 with occlusion)");
    const int64_t n_cam = p->n_cam, n_pts = p->n_pts;
    if (n_pts >= ((int64_t)1 << 32) || n_cam >= ((int64_t)1 << 31))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_within_distance: too many cameras or points");
    int rc = ensure_camblk(p);
    if (rc) return rc;
    free_dense(p);
    hipStream_t st = p->stream;
    if (n_cam == 0 || n_pts == 0) {                                      // nothing can be seen: an empty graph
        DevBuf<uint64_t> row0;
        DevBuf<uint32_t> pt0;
        DevBuf<double> uv0;
        hipError_t e0 = row0.alloc((size_t)n_cam + 1);
        if (e0 == hipSuccess) e0 = pt0.alloc(1);
        if (e0 == hipSuccess) e0 = uv0.alloc(2);
        if (e0 == hipSuccess) e0 = hipMemsetAsync(row0.ptr, 0, sizeof(uint64_t) * (size_t)(n_cam + 1), st);
        if (e0 == hipSuccess) e0 = hipStreamSynchronize(st);
        if (e0 != hipSuccess) return fail(C2B_ERR_HIP, "problem_visibility_within_distance: %s", hipGetErrorString(e0));
        if (row_ptr) std::fill(row_ptr, row_ptr + n_cam + 1, (uint64_t)0);
        p->dense_row = std::move(row0); p->dense_pt = std::move(pt0); p->dense_uv = std::move(uv0);
        p->dense_n = 0;
        return C2B_OK;
    }
    // extent of cameras and points -> the cell grid
    double stats[C2B_STATS_DOUBLES];
    CellGrid g;
    int64_t n_cells = 0;
    rc = compute_stats(p);
    if (!rc) rc = scalars_to_host(st, p->stats, C2B_STATS_DOUBLES, stats);
    if (!rc) rc = cell_grid_from_stats(stats, max_dist, "problem_visibility_within_distance", &g, &n_cells);
    if (rc) return rc;

    DevArena arena;
    DevBuf<uint32_t> cell_of, counts, cursor, sorted, tiles, total, cam_count, pos, max32;
    DevBuf<unsigned long long> sum64;
    DevBuf<uint64_t> row64;
    const int64_t big = std::max(n_cells + 1, n_cam + 1);
    auto temporaries = [&](auto &&each) {
        each(cell_of, (size_t)n_pts); each(counts, (size_t)(n_cells + 1)); each(cursor, (size_t)(n_cells + 1));
        each(sorted, (size_t)n_pts); each(tiles, scan_scratch_count(big)); each(total, (size_t)1);
        each(cam_count, (size_t)(n_cam + 1)); each(pos, (size_t)(n_cam + 1)); each(sum64, (size_t)1); each(max32, (size_t)1);
    };
    size_t arena_bytes = 0;
    temporaries([&](auto &b, size_t n) { arena_bytes += DevArena::room(b, n); });
    hipError_t e = arena.reserve(arena_bytes);
    if (e == hipSuccess) e = row64.alloc((size_t)n_cam + 1);
    if (e != hipSuccess) return fail(hip_code(e), "problem_visibility_within_distance: %s", hipGetErrorString(e));
    temporaries([&](auto &b, size_t n) { arena.carve(b, n); });

    // cell list: count, exclusive scan (start[n_cells] = n_pts), fill
    HIP_TRY(hipMemsetAsync(counts.ptr, 0, 4 * (size_t)(n_cells + 1), st));
    HIP_TRY(hipMemsetAsync(cursor.ptr, 0, 4 * (size_t)(n_cells + 1), st));
    HIP_TRY(hipMemsetAsync(cam_count.ptr, 0, 4 * (size_t)(n_cam + 1), st));
    HIP_TRY(hipMemsetAsync(sum64.ptr, 0, 8, st));
    HIP_TRY(hipMemsetAsync(max32.ptr, 0, 4, st));
    uint32_t n_kept32 = 0;
    uint32_t *start = cursor;                             // scanned counts; the fill's cursors live in `counts` afterwards
    rc = build_cell_list(st, "problem_visibility_within_distance", reinterpret_cast<const double4 *>(p->pts4.ptr), n_pts, g, n_cells,
                         cell_of, counts, start, sorted, tiles, total);
    if (rc) return rc;
    // pass 1: survivors per camera; scan; total
    const unsigned cam_blocks = blocks_of(n_cam, kCellWPB);
    if (e == hipSuccess && n_cam && n_pts) {
        hipLaunchKernelGGL((k_cells_visibility<false>), dim3(cam_blocks), dim3(kCellWPB * 64), 0, st, (const double *)p->camblk, n_cam,
                           reinterpret_cast<const double4 *>(p->pts4.ptr), g, (const uint32_t *)start, sorted,
                           max_dist, occlusion ? 1 : 0, block_length, block_inset, cam_count, (const uint64_t *)nullptr,
                           (uint32_t *)nullptr, (double2 *)nullptr);
        hipLaunchKernelGGL(k_sum_u32_u64, dim3(256), dim3(256), 0, st, cam_count, n_cam, sum64);
        hipLaunchKernelGGL(k_max_u32, dim3(256), dim3(256), 0, st, cam_count, n_cam, max32);
    }
    if (e == hipSuccess) e = scan_flags(st, cam_count, n_cam + 1, pos, tiles, total, &n_kept32);
    unsigned long long n_kept = 0;
    uint32_t longest = 0;
    if (e == hipSuccess) e = hipMemcpy(&n_kept, sum64.ptr, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&longest, max32.ptr, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && n_kept != (unsigned long long)n_kept32)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_within_distance: more than 2^32 observations");
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_widen_u32, dim3(blocks_for(n_cam + 1)), dim3(kBlock), 0, st, pos, n_cam + 1, row64);
        e = launch_error();
    }
    // pass 2: fill in meeting order, then every row into ascending point index
    DevBuf<uint32_t> tmp_pt, out_pt;
    DevBuf<double2> tmp_uv;
    DevBuf<double> out_uv;
    const size_t w = (size_t)n_kept;
    if (e == hipSuccess) e = tmp_pt.alloc(w);
    if (e == hipSuccess) e = tmp_uv.alloc(w);
    if (e == hipSuccess) e = out_pt.alloc(w);
    if (e == hipSuccess) e = out_uv.alloc(2 * w);
    if (e == hipSuccess && w) {
        hipLaunchKernelGGL((k_cells_visibility<true>), dim3(cam_blocks), dim3(kCellWPB * 64), 0, st, (const double *)p->camblk, n_cam,
                           reinterpret_cast<const double4 *>(p->pts4.ptr), g, (const uint32_t *)start, sorted,
                           max_dist, occlusion ? 1 : 0, block_length, block_inset, (uint32_t *)nullptr, row64,
                           tmp_pt, tmp_uv);
        // The device row sort is quadratic in the row length: right for the generators' rows (a few dozen entries), wrong
        // for a radius that makes one camera see tens of thousands of points.  Beyond `long_row` entries the rows are sorted on the
        // host instead (threads over cameras) -- a path for odd inputs, not a fast one; such problems belong to the dense
        // sweep (c2b_problem_visibility_dense).
        // (2 048: a lane of the rank sort then makes at most 64 k dependent compares -- ~0.1 ms per row-wave; at the 8 192 of
        // round 4 a scene with thousands of cameras seeing several thousand points each was a multi-second cliff)
        const uint32_t long_row = p->opt.rank_sort_max_row > 0 ? (uint32_t)p->opt.rank_sort_max_row : 2048u;
        if (longest <= long_row) {
            hipLaunchKernelGGL(k_rows_rank_sort, dim3(cam_blocks), dim3(kCellWPB * 64), 0, st, row64, n_cam, tmp_pt, tmp_uv, out_pt,
                               reinterpret_cast<double2 *>(out_uv.ptr));
            e = launch_error();
        } else {
            e = launch_error();
            std::vector<uint64_t> rp((size_t)n_cam + 1);
            std::vector<uint32_t> hp(w), hq(w);
            std::vector<double> hu(2 * w), hv(2 * w);
            if (e == hipSuccess) e = hipMemcpyAsync(rp.data(), row64.ptr, 8 * ((size_t)n_cam + 1), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(hp.data(), tmp_pt.ptr, 4 * w, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(hu.data(), tmp_uv.ptr, 16 * w, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e == hipSuccess) {
                const int T = (int)std::min<int64_t>(std::max(1u, std::thread::hardware_concurrency()), std::max<int64_t>(1, n_cam));
                c2b_host::run_threads(T, [&](int t) {
                        std::vector<uint32_t> order;
                        for (int64_t c = n_cam * t / T; c < n_cam * (t + 1) / T; ++c) {
                            const size_t b = (size_t)rp[(size_t)c], k = (size_t)(rp[(size_t)c + 1] - rp[(size_t)c]);
                            order.resize(k);
                            for (size_t i = 0; i < k; ++i) order[i] = (uint32_t)i;
                            std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hp[b + x] < hp[b + y]; });
                            for (size_t i = 0; i < k; ++i) {
                                hq[b + i] = hp[b + order[i]];
                                hv[2 * (b + i)] = hu[2 * (b + order[i])];
                                hv[2 * (b + i) + 1] = hu[2 * (b + order[i]) + 1];
                            }
                        }
                    });
                e = hipMemcpyAsync(out_pt.ptr, hq.data(), 4 * w, hipMemcpyHostToDevice, st);
                if (e == hipSuccess) e = hipMemcpyAsync(out_uv.ptr, hv.data(), 16 * w, hipMemcpyHostToDevice, st);
                if (e == hipSuccess) e = hipStreamSynchronize(st);
            }
        }
    }
    if (e == hipSuccess && row_ptr)
        e = hipMemcpyAsync(row_ptr, row64.ptr, sizeof(uint64_t) * (size_t)(n_cam + 1), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(hip_code(e), "problem_visibility_within_distance: %s", hipGetErrorString(e));
    }
    p->dense_row = std::move(row64); p->dense_pt = std::move(out_pt); p->dense_uv = std::move(out_uv);
    p->dense_n = (int64_t)n_kept;
    return C2B_OK;
    C2B_API_END("problem_visibility_within_distance")
}

// generate_world_points_uniform (src/generate.rs:356-420) for the cameras of the resident problem, on the device
// (cell_kernels.hpp: k_world_*): the problem's points are REPLACED by the sampled ones (its observations must be empty).
// Candidate k draws from the k-th splitmix64 stream of `seed` exactly like c2b_generate_world_points, and candidates are
// accepted in order, so the points are that function's, bit for bit.  tri9: HOST triangles [n_tri][9] f32.
int c2b_problem_generate_world_points(c2b_problem *p, const float *tri9, int64_t n_tri, int64_t num_points, double max_dist,
                                      uint64_t seed, int64_t *n_out) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_generate_world_points");
    if (!tri9 || n_tri < 0 || num_points < 0 || !n_out || num_points >= ((int64_t)1 << 31))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_generate_world_points: bad arguments");
    if (p->n_obs != 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_generate_world_points: the problem already has observations");
    if (p->n_cam == 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "Cannot generate world points with 0 cameras. Try increasing the number of cameras generated (via --cameras).");
    if (n_tri == 0) return fail(C2B_ERR_INVALID_ARGUMENT, "the model has no triangles");
    int rc = ensure_camblk(p);
    if (rc) return rc;
    hipStream_t st = p->stream;
    const int64_t n_cam = p->n_cam;
    // triangle areas and their running sum, on the host in the host sampler's own arithmetic (a sequential sum: 1 ms)
    std::vector<double> cum((size_t)n_tri);
    {
        double acc = 0.0;
        for (int64_t t = 0; t < n_tri; ++t) {
            const float *q = tri9 + 9 * t;
            const double a[3] = {(double)q[3] - (double)q[0], (double)q[4] - (double)q[1], (double)q[5] - (double)q[2]};
            const double b[3] = {(double)q[6] - (double)q[0], (double)q[7] - (double)q[1], (double)q[8] - (double)q[2]};
            const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
            acc += std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) / 2.0;
            cum[(size_t)t] = acc;
        }
    }
    // the cell list over the camera centres
    DevBuf<float> d_tri;
    DevBuf<double> d_cum;
    const double4 *centres = reinterpret_cast<const double4 *>(p->cen4.ptr);     // written with camblk (ensure_camblk above)
    hipError_t e = d_tri.alloc(9 * (size_t)n_tri);
    if (e == hipSuccess) e = d_cum.alloc((size_t)n_tri);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tri.ptr, tri9, 36 * (size_t)n_tri, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cum.ptr, cum.data(), 8 * (size_t)n_tri, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(hip_code(e), "problem_generate_world_points: %s", hipGetErrorString(e));
    // the centres' extent (a reduction the statistics kernel already is: cameras only)
    double stats[C2B_STATS_DOUBLES];
    CellGrid g;
    int64_t n_cells = 0;
    rc = c2b_stats(p->camblk, p->cen4, n_cam, p->pts4, 0, p->ws, p->stats, st);
    if (!rc) rc = scalars_to_host(st, p->stats, C2B_STATS_DOUBLES, stats);
    if (!rc) rc = cell_grid_from_stats(stats, max_dist, "problem_generate_world_points", &g, &n_cells);
    if (rc) return rc;
    const int64_t chunk = std::max<int64_t>(4096, std::min<int64_t>(num_points, (int64_t)1 << 20));      // the host sampler's chunks
    DevBuf<uint32_t> cell_of, counts, startb, sorted, tiles, total, ok, pos;
    DevBuf<double4> cand;
    DevBuf<unsigned long long> cutoff;
    DevBuf<double> out;
    const int64_t big = std::max(n_cells + 1, chunk);
    e = cell_of.alloc((size_t)n_cam);
    if (e == hipSuccess) e = counts.alloc((size_t)(n_cells + 1));
    if (e == hipSuccess) e = startb.alloc((size_t)(n_cells + 1));
    if (e == hipSuccess) e = sorted.alloc((size_t)n_cam);
    if (e == hipSuccess) e = tiles.alloc(scan_scratch_count(big));
    if (e == hipSuccess) e = total.alloc(1);
    if (e == hipSuccess) e = cand.alloc((size_t)chunk);
    if (e == hipSuccess) e = ok.alloc((size_t)chunk);
    if (e == hipSuccess) e = pos.alloc((size_t)chunk);
    if (e == hipSuccess) e = cutoff.alloc(1);
    if (e == hipSuccess) e = out.alloc(4 * (size_t)std::max<int64_t>(num_points, 1));
    if (e == hipSuccess) e = hipMemsetAsync(counts.ptr, 0, 4 * (size_t)(n_cells + 1), st);
    if (e != hipSuccess) return fail(hip_code(e), "problem_generate_world_points: %s", hipGetErrorString(e));
    rc = build_cell_list(st, "problem_generate_world_points", centres, n_cam, g, n_cells, cell_of, counts, startb, sorted, tiles, total);
    if (rc) return rc;
    // the reference's loop, a chunk of candidates at a time
    int64_t accepted = 0, failed = 0;
    const int64_t fail_threshold = 10 * num_points;
    for (int64_t k0 = 0; e == hipSuccess && accepted < num_points && failed < fail_threshold; k0 += chunk) {
        const unsigned long long all = (unsigned long long)chunk;
        e = hipMemcpyAsync(cutoff.ptr, &all, 8, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_world_candidates, dim3(blocks_of(chunk, 256)), dim3(256), 0, st, d_tri, n_tri, d_cum, seed, k0, chunk,
                           centres, g, startb, sorted, max_dist, cand, ok);
        uint32_t n_ok = 0;
        e = scan_flags(st, ok, chunk, pos, tiles, total, &n_ok);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_world_cutoff, dim3(blocks_of(chunk, 256)), dim3(256), 0, st, pos, chunk,
                           (uint64_t)(num_points - accepted), (uint64_t)(fail_threshold - failed), cutoff);
        hipLaunchKernelGGL(k_world_accept, dim3(blocks_of(chunk, 256)), dim3(256), 0, st, cand, ok, pos, chunk, cutoff,
                           reinterpret_cast<double4 *>(out.ptr) + accepted);
        e = launch_error();
        unsigned long long cut = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&cut, cutoff.ptr, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        uint32_t took = n_ok;                                 // accepted among the candidates before the cutoff
        if ((int64_t)cut < chunk) {
            e = hipMemcpy(&took, pos + cut, 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
        }
        accepted += (int64_t)took;
        failed += (int64_t)cut - (int64_t)took;
    }
    if (e != hipSuccess) return fail(C2B_ERR_HIP, "problem_generate_world_points: %s", hipGetErrorString(e));
    if (failed >= fail_threshold && num_points > 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "Failed to generate enough points. %lld successes, %lld failures, %lld requested points.",
                    (long long)accepted, (long long)failed, (long long)num_points);
    // the sampled points become the problem's
    free_dense(p);
    drop_rows(p);
    drop_constant(p);
    entities_replaced(p);
    drop_priors(p);
    drop_lm_state(p);
    p->pts4 = std::move(out);
    p->n_pts = accepted;
    *n_out = accepted;
    return C2B_OK;
    C2B_API_END("problem_generate_world_points")
}

int c2b_problem_visibility_dense(c2b_problem *p, double max_dist, uint64_t *row_ptr) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_visibility_dense");
    if (!row_ptr) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_dense: row_ptr is NULL");
    if (!(max_dist >= 0.0)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_dense: max_dist must be >= 0");
    int rc = ensure_camblk(p);
    if (rc) return rc;
    free_dense(p);
    const int64_t n_tiles = c2b_visibility_dense_tiles(p->n_pts);
    const int64_t cells = p->n_cam * n_tiles;
    if (cells > ((int64_t)1 << 33))
        return fail(C2B_ERR_INVALID_ARGUMENT,
                    "problem_visibility_dense: %lld cameras x %lld point tiles is too large for the dense sweep; "
                    "use candidate pairs + c2b_problem_visibility_pairs", (long long)p->n_cam, (long long)n_tiles);
    DevBuf<uint32_t> d_counts;
    DevBuf<uint64_t> d_tot, d_row;
    hipError_t e = d_counts.alloc((size_t)cells);
    if (e == hipSuccess) e = d_tot.alloc((size_t)p->n_cam + 1);
    if (e == hipSuccess) e = d_row.alloc((size_t)p->n_cam + 1);
    if (e == hipSuccess) {
        rc = c2b_visibility_dense_count(p->camblk, p->n_cam, p->pts4, p->n_pts, max_dist, d_counts, d_tot, d_row, p->stream);
        if (!rc) e = hipMemcpyAsync(row_ptr, d_row, sizeof(uint64_t) * (size_t)(p->n_cam + 1), hipMemcpyDeviceToHost, p->stream);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (!rc && e == hipSuccess) {
            const int64_t total = (int64_t)row_ptr[p->n_cam];
            e = p->dense_pt.alloc((size_t)total);
            if (e == hipSuccess) e = p->dense_uv.alloc(2 * (size_t)total);
            if (e == hipSuccess && total) {
                rc = c2b_visibility_dense_fill(p->camblk, p->n_cam, p->pts4, p->n_pts, max_dist, d_counts, d_row, p->dense_pt,
                                               p->dense_uv, p->stream);
                if (!rc) e = hipStreamSynchronize(p->stream);
            }
            if (!rc && e == hipSuccess) { p->dense_n = total; p->dense_row = std::move(d_row); }
        }
    }
    if (rc || e != hipSuccess) free_dense(p);
    if (rc) return rc;
    if (e != hipSuccess) return fail(hip_code(e), "problem_visibility_dense: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_visibility_dense")
}

// `ready`: a hierarchy the caller built over the same triangles (c2b_bvh_build), or NULL: built here when the mesh is
// large enough for one
static int occlude_impl(c2b_problem *p, const float *tri9, int64_t n_tri, const c2b_bvh *ready, uint64_t *row_ptr) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_visibility_dense_occlude");
    if (!p->dense_pt || !p->dense_uv || !p->dense_row)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_dense_occlude: no sweep result");
    if (!row_ptr || n_tri < 0 || (n_tri && !tri9 && !ready)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_dense_occlude: bad arguments");
    const int64_t n = p->dense_n, n_cam = p->n_cam;
    if (!n || !n_tri) {
        HIP_TRY(hipMemcpyAsync(row_ptr, p->dense_row, sizeof(uint64_t) * (size_t)(n_cam + 1), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return C2B_OK;
    }
    DevBuf<char> d_tri, d_nodes;
    DevBuf<uint32_t> d_cam, d_pt_new, d_flag;
    uint32_t stack_overflow = 0;
    DevBuf<uint8_t> d_keep;
    DevBuf<uint64_t> d_row_new;
    DevBuf<double> d_uv_new;
    int rc = C2B_OK;
    // small meshes: every ray against every triangle; larger ones through a hierarchy built here on the host
    const bool use_bvh = ready || n_tri >= kBvhMinTriangles;
    c2b_bvh *built = nullptr;
    int64_t n_nodes = 0;
    if (use_bvh && !ready) {
        rc = c2b_bvh_build(tri9, n_tri, &built);
        if (rc) return rc;
    }
    const c2b_bvh *bvh = ready ? ready : built;
    if (use_bvh) n_nodes = (int64_t)bvh->b.nodes.size();
    const size_t tri_bytes = use_bvh ? (size_t)C2B_BVH_TRI_BYTES * (size_t)n_tri : sizeof(float) * 9 * (size_t)n_tri;
    const void *tri_src = use_bvh ? (const void *)bvh->b.tris.data() : (const void *)tri9;
    hipError_t e = d_tri.alloc(tri_bytes);
    if (e == hipSuccess && use_bvh) e = d_nodes.alloc((size_t)C2B_BVH_NODE_BYTES * (size_t)n_nodes);
    if (e == hipSuccess) e = d_cam.alloc((size_t)n);
    if (e == hipSuccess) e = d_keep.alloc((size_t)n);
    if (e == hipSuccess) e = d_flag.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(uint32_t), p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tri, tri_src, tri_bytes, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess && use_bvh)
        e = hipMemcpyAsync(d_nodes, bvh->b.nodes.data(), (size_t)C2B_BVH_NODE_BYTES * (size_t)n_nodes, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) {
        rc = c2b_expand_rows(p->dense_row, n_cam, 0, n, d_cam, p->stream);
        if (!rc)
            rc = use_bvh ? c2b_occlusion_filter_bvh(p->camblk, p->pts4, d_cam, p->dense_pt, n, d_nodes, n_nodes, d_tri, n_tri, d_keep, d_flag, p->stream)
                         : c2b_occlusion_filter(p->camblk, p->pts4, d_cam, p->dense_pt, n, reinterpret_cast<const float *>(d_tri.ptr), n_tri,
                                                d_keep, p->stream);
        // Stable compaction of the survivor lists on the device (per-camera order of the sweep is kept): kept count per
        // row, row scan, scatter.  Only the new row pointer travels to the host.
        if (!rc) {                                         // a traversal-stack overflow invalidates the whole mask
            e = hipMemcpyAsync(&stack_overflow, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
            if (e == hipSuccess && stack_overflow)
                rc = fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_dense_occlude: hierarchy deeper than the traversal stack");
        }
        if (!rc && e == hipSuccess) {
            int64_t w = 0;
            e = compact_rows_on_device(p, p->dense_row, d_keep, p->dense_pt, p->dense_uv, n_cam, row_ptr, d_row_new, d_pt_new, d_uv_new, &w);
            if (e == hipSuccess) {                           // the filtered lists replace the sweep's
                p->dense_pt = std::move(d_pt_new); p->dense_uv = std::move(d_uv_new); p->dense_row = std::move(d_row_new);
                p->dense_n = w;
            }
        }
    }
    if (rc || e != hipSuccess) (void)hipStreamSynchronize(p->stream);   // no temporary may be freed while a copy still reads it
    c2b_bvh_free(built);
    if (rc) return rc;
    if (e != hipSuccess) return fail(hip_code(e), "problem_visibility_dense_occlude: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_visibility_dense_occlude")
}

int c2b_problem_visibility_dense_occlude(c2b_problem *p, const float *tri9, int64_t n_tri, uint64_t *row_ptr) {
    return occlude_impl(p, tri9, n_tri, nullptr, row_ptr);
}
int c2b_problem_visibility_dense_occlude_bvh(c2b_problem *p, const c2b_bvh *bvh, uint64_t *row_ptr) {
    if (!bvh) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_dense_occlude_bvh: bvh is NULL");
    return occlude_impl(p, nullptr, (int64_t)(bvh->b.tris.size() / (C2B_BVH_TRI_BYTES / sizeof(bvh->b.tris[0]))), bvh, row_ptr);
}

int c2b_problem_visibility_dense_fetch(c2b_problem *p, uint64_t *pt_idx, double *uv) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_visibility_dense_fetch");
    if (!p->dense_pt || !p->dense_uv) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_dense_fetch: no sweep result");
    const int64_t n = p->dense_n;
    if (!n) return C2B_OK;
    if (uv) HIP_TRY(hipMemcpyAsync(uv, p->dense_uv, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, p->stream));
    if (pt_idx) {
        std::vector<uint32_t> tmp((size_t)n);
        HIP_TRY(hipMemcpyAsync(tmp.data(), p->dense_pt, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        for (int64_t i = 0; i < n; ++i) pt_idx[i] = tmp[(size_t)i];
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_visibility_dense_fetch")
}

// ---- the camera covisibility graph of the resident list and the search over it -------------------------------
// The graph at min_shared, built on first use (covisibility_build, capi_solve.hpp, which the solver's own pattern shares) into
// locals and moved in on success, as ensure_transpose does; kept until the list changes (drop_rows) or another threshold is asked for.
static int ensure_covisibility(c2b_problem *p, int min_shared) {
    if (p->cv_ptr && p->cv_min_shared == min_shared) return C2B_OK;
    DevBuf<uint64_t> ptr;
    DevBuf<uint32_t> nbr, shared;
    int64_t h[2] = {0, 0};
    if (const int rc = covisibility_build(p, min_shared, ptr, nbr, shared, h)) return rc;
    p->cv_ptr = std::move(ptr); p->cv_nbr = std::move(nbr); p->cv_shared = std::move(shared);
    p->cv_min_shared = min_shared;
    p->cv_edges = h[0]; p->cv_heavy = h[1];
    return C2B_OK;
}

int c2b_problem_covisibility(c2b_problem *p, int min_shared, int64_t *n_edges) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_covisibility: problem is NULL");
    if (min_shared < 1) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_covisibility: min_shared must be at least 1");
    NEED_UPLOADED(p, "problem_covisibility");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_covisibility: a shard has no graph of its own (a point's observations span every rank)");
    if (const int rc = ensure_covisibility(p, min_shared)) return rc;
    if (n_edges) *n_edges = p->cv_edges;
    return C2B_OK;
    C2B_API_END("problem_covisibility")
}

int c2b_problem_get_covisibility(c2b_problem *p, uint64_t *nbr_ptr, uint32_t *nbr, uint32_t *shared, int *min_shared, int64_t *n_heavy) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_covisibility: problem is NULL");
    if (!p->cv_ptr) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_covisibility: no graph (c2b_problem_covisibility builds it; a change of the list drops it)");
    HIP_TRY(hipSetDevice(p->device));
    const size_t ne = (size_t)p->cv_edges;
    if (nbr_ptr) HIP_TRY(hipMemcpyAsync(nbr_ptr, p->cv_ptr, sizeof(uint64_t) * ((size_t)p->n_cam + 1), hipMemcpyDeviceToHost, p->stream));
    if (nbr && ne) HIP_TRY(hipMemcpyAsync(nbr, p->cv_nbr, sizeof(uint32_t) * ne, hipMemcpyDeviceToHost, p->stream));
    if (shared && ne) HIP_TRY(hipMemcpyAsync(shared, p->cv_shared, sizeof(uint32_t) * ne, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (min_shared) *min_shared = p->cv_min_shared;
    if (n_heavy) *n_heavy = p->cv_heavy;
    return C2B_OK;
    C2B_API_END("problem_get_covisibility")
}

int c2b_problem_neighbourhood(c2b_problem *p, const uint8_t *seed, int hops, int min_shared, int64_t max_cameras, const uint8_t *within,
                              uint8_t *member, int32_t *level, int64_t *n) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_neighbourhood: problem is NULL");
    if (!seed) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_neighbourhood: seed is NULL");
    if (min_shared < 1) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_neighbourhood: min_shared must be at least 1");
    NEED_UPLOADED(p, "problem_neighbourhood");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_neighbourhood: a shard has no graph of its own (a point's observations span every rank)");
    const int64_t n_cam = p->n_cam, cap = max_cameras > 0 ? max_cameras : 0;
    int64_t n_seed = 0;
    for (int64_t c = 0; c < n_cam; ++c) {
        if (!seed[c]) continue;
        ++n_seed;
        if (within && !within[c]) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_neighbourhood: seed camera %lld lies outside `within`", (long long)c);
    }
    if (!n_seed) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_neighbourhood: no seed camera");
    if (cap && n_seed > cap)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_neighbourhood: %lld seed cameras, max_cameras %lld", (long long)n_seed, (long long)cap);
    if (const int rc = ensure_covisibility(p, min_shared)) return rc;
    hipStream_t st = p->stream;
    DevBuf<uint8_t> d_seed, d_within, select;
    DevBuf<int32_t> d_level;
    DevBuf<uint32_t> front, next, n_next;
    DevBuf<uint64_t> keys;
    DevBuf<char> temp;
    DevArena arena;
    const size_t nc = (size_t)n_cam;
    auto temporaries = [&](auto &&each) {
        each(d_seed, nc); each(d_within, nc); each(select, nc); each(d_level, nc); each(front, nc); each(next, nc); each(n_next, (size_t)1);
        each(keys, nc); each(temp, (size_t)c2b_covisibility_temp_bytes(n_cam, C2B_COVIS_TEMP_EXPAND));
    };
    size_t arena_bytes = 0;
    temporaries([&](auto &b, size_t k) { arena_bytes += DevArena::room(b, k); });
    hipError_t e = arena.reserve(arena_bytes);
    if (e != hipSuccess) return fail(hip_code(e), "problem_neighbourhood: %s", hipGetErrorString(e));
    temporaries([&](auto &b, size_t k) { arena.carve(b, k); });
    struct SyncOnExit { hipStream_t s; ~SyncOnExit() { (void)hipStreamSynchronize(s); } } sync_on_exit{st};      // before the arena is freed
    const CovisTemp T(temp.ptr, n_cam, false);
    HIP_TRY(hipMemcpyAsync(d_seed, seed, nc, hipMemcpyHostToDevice, st));
    if (within) HIP_TRY(hipMemcpyAsync(d_within, within, nc, hipMemcpyHostToDevice, st));
    const uint8_t *w = within ? d_within.ptr : nullptr;
    hipLaunchKernelGGL(k_covis_seed_levels, dim3(blocks_for(n_cam, 256)), dim3(256), 0, st, (const uint8_t *)d_seed, n_cam, d_level.ptr);
    covis_collect_level(st, T, d_level, n_cam, 0, front.ptr, n_next.ptr);
    LAUNCH_CHECK();
    int64_t taken = n_seed, n_front = n_seed;
    for (int h = 0; (hops < 0 || h < hops) && n_front && !(cap && taken == cap) && h < 0x7ffffffe; ++h) {
        int rc = c2b_covisibility_expand_rows(p->cv_ptr, p->cv_nbr, p->cv_shared, n_cam, min_shared, w, front, n_front, h, d_level, next, n_next, temp, st);
        if (rc) return rc;
        uint32_t got = 0;
        HIP_TRY(hipMemcpyAsync(&got, n_next.ptr, sizeof got, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!got) break;
        if (cap && taken + (int64_t)got > cap) {
            // the level does not fit: its best (score descending, index ascending) fill the remainder and the search ends
            const int64_t rem = cap - taken;
            HIP_TRY(hipMemsetAsync(keys, 0xff, sizeof(uint64_t) * nc, st));              // a camera that is no candidate sorts last
            hipLaunchKernelGGL(k_covis_score, dim3(blocks_for(got, 4)), dim3(256), 0, st, (const uint64_t *)p->cv_ptr, (const uint32_t *)p->cv_nbr,
                               (const uint32_t *)p->cv_shared, (uint32_t)min_shared, (const uint32_t *)next, (int64_t)got, (int32_t)h,
                               (const int32_t *)d_level, keys.ptr);
            LAUNCH_CHECK();
            if ((rc = c2b_select_smallest_keys_rows(keys, n_cam, 0, 0, 0, rem, select, st))) return rc;
            hipLaunchKernelGGL(k_covis_unselect, dim3(blocks_for(got, 256)), dim3(256), 0, st, (const uint32_t *)next, (int64_t)got, (const uint8_t *)select,
                               d_level.ptr);
            LAUNCH_CHECK();
            taken = cap;
            break;
        }
        taken += got;
        n_front = got;
        std::swap(front, next);
    }
    std::vector<int32_t> h_level(nc);
    if (nc) HIP_TRY(hipMemcpyAsync(h_level.data(), d_level, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int64_t count = 0;
    for (size_t c = 0; c < nc; ++c) count += h_level[c] >= 0;
    if (count != taken) return fail(C2B_ERR_HIP, "problem_neighbourhood: %lld cameras reached instead of %lld", (long long)count, (long long)taken);
    for (size_t c = 0; c < nc; ++c) {
        if (member) member[c] = h_level[c] >= 0 ? 1 : 0;
        if (level) level[c] = h_level[c];
    }
    if (n) *n = count;
    return C2B_OK;
    C2B_API_END("problem_neighbourhood")
}
