// capi_index_noise.hpp -- Level 0 and Level 1 of the index noise on the device (index_noise_kernels.hpp): noise.rs'
// drop_features, add_incorrect_correspondences, split_landmarks and join_landmarks (src/noise.rs:179-378) in place on the
// resident problem, by counter-based draws.  The host functions of capi_host_rows.hpp keep their own (sequential) draw scheme.
// Part of the one translation unit of the C ABI: included by capi_problem.hpp after capi_subset.hpp, never compiled or included on its own.

extern "C++" {
namespace {

bool good_fraction(double v) { return v == v; }              // anything but a NaN: negative counts as 0, above 1 saturates

// floor(fraction * count), negative as 0, capped at `cap` (host_noise.hpp: fraction_of)
int64_t fraction_count(double fraction, int64_t count, int64_t cap) {
    const double v = fraction * (double)count;
    if (!(v > 0.0)) return 0;
    return v >= (double)cap ? cap : (int64_t)v;
}

// sel[i] = 1 for the n_sel smallest (key, index) of n entities, else 0 (index_noise_kernels.hpp: select).  Synchronises.
int select_smallest(hipStream_t st, const char *who, const uint64_t *keys, int64_t n, uint64_t entity_base, uint64_t seed, uint32_t stream_id,
                    uint32_t slot, int64_t n_sel, uint8_t *sel) {
    if (n <= 0) return C2B_OK;
    if (n_sel <= 0 || n_sel >= n) {
        HIP_TRY(hipMemsetAsync(sel, n_sel > 0 ? 1 : 0, (size_t)n, st));
        HIP_TRY(hipStreamSynchronize(st));
        return C2B_OK;
    }
    DevBuf<unsigned long long> hist;
    HIP_TRY(hist.alloc(256));
    unsigned long long h[256];
    uint64_t prefix = 0, need = (uint64_t)n_sel, equal = 0;
    const unsigned blocks = std::min(blocks_of(n, 256), 2048u);
    for (int shift = 56; shift >= 0; shift -= 8) {
        HIP_TRY(hipMemsetAsync(hist.ptr, 0, sizeof h, st));
        hipLaunchKernelGGL(k_select_hist, dim3(blocks), dim3(256), 0, st, keys, n, entity_base, seed, stream_id, slot, prefix, shift, hist.ptr);
        LAUNCH_CHECK();
        HIP_TRY(hipMemcpyAsync(h, hist.ptr, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int d = 0;
        while (d < 255 && need > h[d]) need -= h[d++];
        if (need > h[d]) return fail(C2B_ERR_HIP, "%s: the key histogram does not add up", who);
        prefix |= (uint64_t)d << shift;
        equal = h[d];
    }
    // `equal` keys are T = prefix, `need` of them are taken: all of them, or the first by index
    if (need == equal) {
        hipLaunchKernelGGL(k_select_mark, dim3(blocks_of(n, 256)), dim3(256), 0, st, keys, n, entity_base, seed, stream_id, slot, prefix, 1, sel,
                           (uint32_t *)nullptr);
        LAUNCH_CHECK();
        HIP_TRY(hipStreamSynchronize(st));
        return C2B_OK;
    }
    DevBuf<uint32_t> eq, pos, tiles, total;
    HIP_TRY(eq.alloc((size_t)n));
    HIP_TRY(pos.alloc((size_t)n));
    HIP_TRY(tiles.alloc(scan_scratch_count(n)));
    HIP_TRY(total.alloc(1));
    hipLaunchKernelGGL(k_select_mark, dim3(blocks_of(n, 256)), dim3(256), 0, st, keys, n, entity_base, seed, stream_id, slot, prefix, 0, sel, eq.ptr);
    scan_by_length(st, (const uint32_t *)eq.ptr, n, 0u, pos.ptr, total.ptr, tiles.ptr);
    hipLaunchKernelGGL(k_select_ties, dim3(blocks_of(n, 256)), dim3(256), 0, st, (const uint32_t *)eq.ptr, (const uint32_t *)pos.ptr, n, (uint32_t)need, sel);
    const hipError_t el = launch_error(), es = hipStreamSynchronize(st);          // the temporaries are freed on return
    if (el != hipSuccess || es != hipSuccess) return fail(hip_code(el != hipSuccess ? el : es), "%s: %s", who, hipGetErrorString(el != hipSuccess ? el : es));
    return C2B_OK;
}

// the scan's total of a selection against the count it was asked for.  Synchronises.
int selected_count_is(hipStream_t st, const char *who, const uint32_t *d_total, int64_t n) {
    uint32_t got = 0;
    hipError_t e = launch_error();
    if (e == hipSuccess) e = hipMemcpyAsync(&got, d_total, sizeof got, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    if ((int64_t)got != n) return fail(C2B_ERR_HIP, "%s: %lld entities selected instead of %lld", who, (long long)got, (long long)n);
    return C2B_OK;
}

// about four points per cell over the live ones of x and z, as PointGrid (host_noise.hpp) sizes its cells
double nearest_cell_size(const double *stats, int64_t n_pts) {
    const double ex = stats[9] - stats[6], ez = stats[11] - stats[8], n = (double)std::max<int64_t>(n_pts, 1);
    double cs = 1.0;
    if (ex > 0.0 && ez > 0.0) cs = std::sqrt(ex * ez * 4.0 / n);
    else if (ex > 0.0 || ez > 0.0) cs = (ex + ez) * 4.0 / n;
    if (!(cs > 0.0) || !std::isfinite(cs)) cs = std::max(ex, ez) > 0.0 && std::isfinite(std::max(ex, ez)) ? std::max(ex, ez) : 1.0;
    return cs;
}

}  // namespace
}  // extern "C++"

int c2b_drop_keep_rows(const uint64_t *row_ptr, int64_t n_cam, int64_t n_obs, double keep_fraction, uint64_t seed, uint8_t *keep, void *stream) {
    C2B_API_BEGIN
    if (!good_fraction(keep_fraction)) return fail(C2B_ERR_INVALID_ARGUMENT, "drop_keep_rows: keep_fraction is NaN");
    if (n_cam < 0 || n_obs < 0 || (n_obs && (!row_ptr || !keep || !n_cam))) return fail(C2B_ERR_INVALID_ARGUMENT, "drop_keep_rows: bad arguments");
    if (!aligned8(row_ptr)) return fail(C2B_ERR_INVALID_ARGUMENT, "drop_keep_rows: misaligned pointer");
    if (!n_obs) return C2B_OK;
    hipStream_t st = S(stream);
    hipLaunchKernelGGL(k_drop_keep, dim3(blocks_for(n_cam, kIdxWaves)), dim3(kIdxBlock), 0, st, row_ptr, n_cam, keep_fraction, seed, keep);
    LAUNCH_CHECK();
    return C2B_OK;
    C2B_API_END("drop_keep_rows")
}

int c2b_mismatch_partner_rows(const uint64_t *row_ptr, int64_t n_cam, const double *uv_obs, int64_t n_obs, double mismatch_chance, uint64_t seed,
                              int32_t *partner, int64_t *n_zero_rows, void *stream) {
    C2B_API_BEGIN
    if (!good_fraction(mismatch_chance)) return fail(C2B_ERR_INVALID_ARGUMENT, "mismatch_partner_rows: mismatch_chance is NaN");
    if (n_cam < 0 || n_obs < 0 || n_obs > (int64_t)0x7fffffff - 64)          // (a row's length and its chunk offsets are ints in the kernel)
        return fail(C2B_ERR_INVALID_ARGUMENT, "mismatch_partner_rows: n_obs out of range");
    if (!n_zero_rows || (n_obs && (!row_ptr || !uv_obs || !partner || !n_cam))) return fail(C2B_ERR_INVALID_ARGUMENT, "mismatch_partner_rows: NULL argument");
    if (!aligned8(row_ptr) || !aligned16(uv_obs) || !aligned8(n_zero_rows) || (reinterpret_cast<uintptr_t>(partner) & 3))
        return fail(C2B_ERR_INVALID_ARGUMENT, "mismatch_partner_rows: misaligned pointer");
    hipStream_t st = S(stream);
    HIP_TRY(hipMemsetAsync(n_zero_rows, 0, sizeof(int64_t), st));
    if (!n_obs) return C2B_OK;
    hipLaunchKernelGGL(k_mismatch_partner, dim3(blocks_for(n_cam, kIdxWaves)), dim3(kIdxBlock), 0, st, row_ptr, n_cam,
                       reinterpret_cast<const double2 *>(uv_obs), mismatch_chance, seed, partner, reinterpret_cast<unsigned long long *>(n_zero_rows));
    LAUNCH_CHECK();
    return C2B_OK;
    C2B_API_END("mismatch_partner_rows")
}

int c2b_select_smallest_keys_rows(const uint64_t *keys, int64_t n, uint64_t seed, int draw_stream, int slot, int64_t n_select, uint8_t *select,
                                  void *stream) {
    C2B_API_BEGIN
    if (n < 0 || n >= ((int64_t)1 << 32) || (n && !select)) return fail(C2B_ERR_INVALID_ARGUMENT, "select_smallest_keys_rows: bad arguments");
    if (draw_stream < 0 || slot < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "select_smallest_keys_rows: stream and slot must be >= 0");
    if (!aligned8(keys)) return fail(C2B_ERR_INVALID_ARGUMENT, "select_smallest_keys_rows: misaligned pointer");
    if (!n) return C2B_OK;
    return select_smallest(S(stream), "select_smallest_keys_rows", keys, n, 0, seed, (uint32_t)draw_stream, (uint32_t)slot, n_select, select);
    C2B_API_END("select_smallest_keys_rows")
}

int c2b_nearest_points_rows(const double *pts4, int64_t n_pts, const uint32_t *query, int64_t n_query, int32_t *nearest, void *stream) {
    C2B_API_BEGIN
    if (n_pts < 0 || n_pts >= ((int64_t)1 << 31) || n_query < 0 || n_query >= ((int64_t)1 << 31))
        return fail(C2B_ERR_INVALID_ARGUMENT, "nearest_points_rows: count out of range");
    if (n_query && (!n_pts || !pts4 || !query || !nearest)) return fail(C2B_ERR_INVALID_ARGUMENT, "nearest_points_rows: NULL argument or no points");
    if (!aligned16(pts4) || (reinterpret_cast<uintptr_t>(query) & 3) || (reinterpret_cast<uintptr_t>(nearest) & 3))
        return fail(C2B_ERR_INVALID_ARGUMENT, "nearest_points_rows: misaligned pointer");
    if (!n_query) return C2B_OK;
    hipStream_t st = S(stream);
    const double4 *pos4 = reinterpret_cast<const double4 *>(pts4);
    PointCells cells;
    const int rc = build_point_cells_by(st, "nearest_points_rows", pos4, n_pts, [n_pts](const double *stats) { return nearest_cell_size(stats, n_pts); },
                                        cells, [](auto &&) {});
    if (rc) return rc;
    hipLaunchKernelGGL(k_nearest_points, dim3(blocks_for(n_query, kIdxWaves)), dim3(kIdxBlock), 0, st, pos4, n_pts, query, n_query, cells.g,
                       1.0 / cells.g.inv_cs, (const uint32_t *)cells.start.ptr, (const uint32_t *)cells.sorted.ptr, nearest);
    const hipError_t el = launch_error(), es = hipStreamSynchronize(st);          // the arena is freed on return
    if (el != hipSuccess || es != hipSuccess)
        return fail(hip_code(el != hipSuccess ? el : es), "nearest_points_rows: %s", hipGetErrorString(el != hipSuccess ? el : es));
    return C2B_OK;
    C2B_API_END("nearest_points_rows")
}

// ---- Level 1 ------------------------------------------------------------------------------------------------------------------
// drop_features: the keep bits, then the filter's compaction and installation.  The entities do not move: what
// c2b_problem_filter_observations leaves (cameras, points, masks, priors, loss, options, checkpoint) stays here too.
int c2b_problem_drop_features(c2b_problem *p, double keep_fraction, uint64_t seed, int64_t *n_removed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_drop_features");
    if (n_removed) *n_removed = 0;
    if (!good_fraction(keep_fraction)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_drop_features: keep_fraction is NaN");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_drop_features: a shard is not thinned alone (its list is a slice of the whole one)");
    if (!p->n_obs) return C2B_OK;
    int rc = ensure_rows(p);
    if (rc) return rc;
    const int64_t n_old = p->n_obs;
    DevBuf<uint8_t> keep;
    const hipError_t e = keep.alloc((size_t)n_old);
    if (e != hipSuccess) return fail(hip_code(e), "problem_drop_features: %s", hipGetErrorString(e));
    rc = c2b_drop_keep_rows(p->rows_ptr, p->n_cam, n_old, keep_fraction, seed, keep, p->stream);
    if (rc) {
        (void)hipStreamSynchronize(p->stream);
        return rc;
    }
    return compact_and_install(p, "problem_drop_features", keep, n_old, n_removed);
    C2B_API_END("problem_drop_features")
}

// add_incorrect_correspondences: the partner pass, and -- unless it counted a row without a positive total weight -- the swaps.
// uv, the row lengths and every per-entity state stay; after a call that swapped, what was derived from the list goes
// (drop_rows), as after c2b_problem_rematch_observations.
int c2b_problem_add_incorrect_correspondences(c2b_problem *p, double mismatch_chance, uint64_t seed, int64_t *n_swaps) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_incorrect_correspondences");
    if (n_swaps) *n_swaps = 0;
    if (!good_fraction(mismatch_chance)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_incorrect_correspondences: mismatch_chance is NaN");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_incorrect_correspondences: a shard is not corrupted alone (its list is a slice of the whole one)");
    if (!p->n_obs) return C2B_OK;
    int rc = ensure_rows(p);
    if (rc) return rc;
    hipStream_t st = p->stream;
    DevBuf<int32_t> partner;
    DevBuf<int64_t> counts;                                  // rows without a positive total, swaps
    hipError_t e = partner.alloc((size_t)p->n_obs);
    if (e == hipSuccess) e = counts.alloc(2);
    if (e != hipSuccess) return fail(hip_code(e), "problem_add_incorrect_correspondences: %s", hipGetErrorString(e));
    int64_t h[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(counts.ptr, 0, sizeof h, st));
    rc = c2b_mismatch_partner_rows(p->rows_ptr, p->n_cam, p->uv, p->n_obs, mismatch_chance, seed, partner, counts.ptr, st);
    if (!rc) {
        e = hipMemcpyAsync(h, counts.ptr, sizeof(int64_t), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess) e = es;
    } else {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (e != hipSuccess) return fail(hip_code(e), "problem_add_incorrect_correspondences: %s", hipGetErrorString(e));
    if (h[0]) return fail(C2B_ERR_INVALID_ARGUMENT, "add_incorrect_correspondences: all swap weights are zero (%lld cameras)", (long long)h[0]);
    hipLaunchKernelGGL(k_mismatch_apply, dim3(blocks_of(p->n_cam, 256)), dim3(256), 0, st, (const uint64_t *)p->rows_ptr.ptr, p->n_cam,
                       (const int32_t *)partner.ptr, p->pt_idx.ptr, reinterpret_cast<unsigned long long *>(counts.ptr + 1));
    e = launch_error();
    if (e == hipSuccess) e = hipMemcpyAsync(h + 1, counts.ptr + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(hip_code(e), "problem_add_incorrect_correspondences: %s", hipGetErrorString(e));
    if (h[1]) drop_rows(p);                                  // pt_idx changed
    if (n_swaps) *n_swaps = h[1];
    return C2B_OK;
    C2B_API_END("problem_add_incorrect_correspondences")
}

// split_landmarks: the point table grows by the copies.  THE POLICY for what has one entry per point is c2b_problem_cull's for a
// changed entity count: the masks and the priors are dropped, so are a checkpoint with the LM scratch and an origin
// (drop_constant, drop_priors, drop_lm_state, entities_replaced), and what was derived from the list (drop_rows).  A call that
// selects no point changes and drops nothing.
int c2b_problem_split_landmarks(c2b_problem *p, double split_fraction, uint64_t seed, int64_t *n_split) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_split_landmarks");
    if (n_split) *n_split = 0;
    if (!good_fraction(split_fraction)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_split_landmarks: split_fraction is NaN");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_split_landmarks: a shard is not split alone (a point's observations span every rank)");
    const int64_t np = p->n_pts, n = fraction_count(split_fraction, np, np);
    if (!n) return C2B_OK;
    if (np + n >= ((int64_t)1 << 31)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_split_landmarks: too many points");
    hipStream_t st = p->stream;
    DevBuf<uint8_t> sel;
    DevBuf<uint32_t> pos, tiles, total;
    DevBuf<double> pts_new;
    hipError_t e = sel.alloc((size_t)np);
    if (e == hipSuccess) e = pos.alloc((size_t)np);
    if (e == hipSuccess) e = tiles.alloc(scan_scratch_count(np));
    if (e == hipSuccess) e = total.alloc(1);
    if (e == hipSuccess) e = pts_new.alloc(4 * (size_t)(np + n));
    if (e != hipSuccess) return fail(hip_code(e), "problem_split_landmarks: %s", hipGetErrorString(e));
    int rc = select_smallest(st, "problem_split_landmarks", nullptr, np, 0, seed, kStreamSplit, 0, n, sel);
    if (rc) return rc;
    scan_by_length(st, (const uint8_t *)sel.ptr, np, 0u, pos.ptr, total.ptr, tiles.ptr);
    if ((rc = selected_count_is(st, "problem_split_landmarks", total.ptr, n))) return rc;      // the copies are addressed by it
    hipLaunchKernelGGL(k_split_points, dim3(blocks_of(np, 256)), dim3(256), 0, st, reinterpret_cast<const double4 *>(p->pts4.ptr), np,
                       (const uint8_t *)sel.ptr, (const uint32_t *)pos.ptr, reinterpret_cast<double4 *>(pts_new.ptr));
    e = launch_error();
    if (e == hipSuccess) e = hipStreamSynchronize(st);       // the problem is touched only once the new table stands
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(hip_code(e), "problem_split_landmarks: %s", hipGetErrorString(e));
    }
    if (p->n_obs) hipLaunchKernelGGL(k_split_obs, dim3(blocks_of(p->n_obs, 256)), dim3(256), 0, st, p->pt_idx.ptr, p->n_obs, np,
                                     (const uint8_t *)sel.ptr, (const uint32_t *)pos.ptr, seed);
    e = launch_error();
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(hip_code(e), "problem_split_landmarks: %s", hipGetErrorString(e));
    free_dense(p);                                            // (a pending visibility result names the old table)
    p->pts4 = std::move(pts_new);
    p->n_pts = np + n;
    drop_rows(p);
    drop_constant(p);
    entities_replaced(p);
    drop_priors(p);
    drop_lm_state(p);
    if (n_split) *n_split = n;
    return C2B_OK;
    C2B_API_END("problem_split_landmarks")
}

// join_landmarks: the selected observations take a neighbour of their point.  Nothing but pt_idx changes: the entities, the
// masks, the priors and a checkpoint stay; after a call that joined, what was derived from the list goes (drop_rows).
int c2b_problem_join_landmarks(c2b_problem *p, double join_fraction, uint64_t seed, int64_t *n_joined) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_join_landmarks");
    if (n_joined) *n_joined = 0;
    if (!good_fraction(join_fraction)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_join_landmarks: join_fraction is NaN");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_join_landmarks: a shard is not joined alone (a point's observations span every rank)");
    const int64_t np = p->n_pts, no = p->n_obs, n = fraction_count(join_fraction, np, no);
    if (!n) return C2B_OK;
    if (np < 2) return fail(C2B_ERR_INVALID_ARGUMENT, "join_landmarks: No neighbors?!");
    if (np >= ((int64_t)1 << 31) || no >= ((int64_t)1 << 32)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_join_landmarks: too many points or observations");
    hipStream_t st = p->stream;
    DevBuf<uint8_t> sel;
    DevBuf<uint32_t> pos, tiles, total, list, query;
    DevBuf<int32_t> nn;
    hipError_t e = sel.alloc((size_t)no);
    if (e == hipSuccess) e = pos.alloc((size_t)no);
    if (e == hipSuccess) e = tiles.alloc(scan_scratch_count(no));
    if (e == hipSuccess) e = total.alloc(1);
    if (e == hipSuccess) e = list.alloc((size_t)n);
    if (e == hipSuccess) e = query.alloc((size_t)n);
    if (e == hipSuccess) e = nn.alloc((size_t)n * kNearest);
    if (e != hipSuccess) return fail(hip_code(e), "problem_join_landmarks: %s", hipGetErrorString(e));
    int rc = select_smallest(st, "problem_join_landmarks", nullptr, no, 0, seed, kStreamJoin, 0, n, sel);
    if (rc) return rc;
    scan_by_length(st, (const uint8_t *)sel.ptr, no, 0u, pos.ptr, total.ptr, tiles.ptr);
    if ((rc = selected_count_is(st, "problem_join_landmarks", total.ptr, n))) return rc;       // the list is addressed by it
    hipLaunchKernelGGL(k_select_list, dim3(blocks_of(no, 256)), dim3(256), 0, st, (const uint8_t *)sel.ptr, (const uint32_t *)pos.ptr, no, list.ptr);
    hipLaunchKernelGGL(k_join_queries, dim3(blocks_of(n, 256)), dim3(256), 0, st, (const uint32_t *)p->pt_idx.ptr, (const uint32_t *)list.ptr, n, query.ptr);
    e = launch_error();
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(hip_code(e), "problem_join_landmarks: %s", hipGetErrorString(e));
    }
    rc = c2b_nearest_points_rows(p->pts4, np, query, n, nn, st);         // synchronises
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    hipLaunchKernelGGL(k_join_apply, dim3(blocks_of(n, 256)), dim3(256), 0, st, p->pt_idx.ptr, (const uint32_t *)list.ptr, n, (const int32_t *)nn.ptr,
                       (int)std::min<int64_t>(kNearest - 1, np - 1), seed);
    e = launch_error();
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(hip_code(e), "problem_join_landmarks: %s", hipGetErrorString(e));
    drop_rows(p);                                            // pt_idx changed
    if (n_joined) *n_joined = n;
    return C2B_OK;
    C2B_API_END("problem_join_landmarks")
}
