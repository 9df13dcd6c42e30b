// capi_subset.hpp -- Level 1, sub-problems on the device: c2b_problem_subset (BAProblem::subset, src/baproblem.rs:394-423,
// for a caller's selection), c2b_problem_window (a window of cameras, its rim held fixed), c2b_problem_get_origin and
// c2b_problem_write_back.  Both extractions end in one routine, build_child, once they hold the same three device lists.
// Part of the one translation unit of the C ABI: included by capi_problem.hpp where this text sat, never compiled or included on its own.

extern "C++" {
namespace {

// short or tiled by the length, as every caller of scan_kernels.hpp chooses (scratch: scan_scratch_count(n) elements of Out)
template <class In, class Out>
void scan_by_length(hipStream_t st, const In *in, int64_t n, Out first, Out *out, Out *total, Out *scratch) {
    if (n <= kScanTile) scan_short(st, in, n, first, out, total);
    else scan_tiled(st, in, n, first, out, total, scratch);
}

// what subset and window hand to build_child: child camera -> parent camera, child point -> parent point (device and host), parent
// point -> child point or -1 (device), the roles (host; empty: all 0), and what the child takes from the parent's handle
struct ChildLists {
    DevBuf<uint32_t> cam_of, pt_of;
    DevBuf<int32_t> new_of;
    std::vector<uint32_t> h_cam_of, h_pt_of;
    std::vector<uint8_t> h_cam_role, h_pt_role;
    bool carry = false, origin = false;
};

// a problem under construction on the stack: its buffers free themselves, and no queued work may still use them when they do
struct ScratchProblem {
    c2b_problem q;
    ~ScratchProblem() {
        if (q.stream) (void)hipStreamSynchronize(q.stream);
        q.stream = nullptr;                                   // borrowed
    }
};

// dst's contents replaced by t's, as an upload replaces them; with carry the handle state too.  Nothing here can fail.
void adopt_problem(c2b_problem *dst, c2b_problem &t, const c2b_problem *src, ChildLists &L) {
    free_buffers(dst);
    drop_constant(dst);
    drop_priors(dst);
    entities_replaced(dst);
    dst->cam15 = std::move(t.cam15); dst->bal9 = std::move(t.bal9); dst->camblk = std::move(t.camblk); dst->cen4 = std::move(t.cen4);
    dst->pts4 = std::move(t.pts4); dst->uv = std::move(t.uv); dst->cam_idx = std::move(t.cam_idx); dst->pt_idx = std::move(t.pt_idx);
    dst->ws = std::move(t.ws); dst->stats = std::move(t.stats); dst->scalar = std::move(t.scalar);
    dst->n_cam = t.n_cam; dst->n_pts = t.n_pts; dst->n_obs = t.n_obs;
    dst->bal_valid = t.bal_valid;                             // camblk is rebuilt on demand from the gathered cameras
    dst->shard_cam_base = 0; dst->shard_n_cam_global = -1; dst->shard_obs_base = 0;
    // the masks and priors the setters installed in t (none without carry)
    dst->cmask = std::move(t.cmask); dst->pmask = std::move(t.pmask);
    dst->h_cmask.swap(t.h_cmask); dst->h_pmask.swap(t.h_pmask);
    dst->const_n_cam = t.const_n_cam; dst->const_n_pts = t.const_n_pts; dst->const_params = t.const_params; dst->const_pts = t.const_pts;
    dst->pc0 = std::move(t.pc0); dst->pcw = std::move(t.pcw); dst->pi0 = std::move(t.pi0); dst->piw = std::move(t.piw);
    dst->px0 = std::move(t.px0); dst->pxw = std::move(t.pxw); dst->prior_part = std::move(t.prior_part);
    dst->h_pc0.swap(t.h_pc0); dst->h_pcw.swap(t.h_pcw); dst->h_pi0.swap(t.h_pi0); dst->h_piw.swap(t.h_piw);
    dst->h_px0.swap(t.h_px0); dst->h_pxw.swap(t.h_pxw);
    dst->prior_n_cam = t.prior_n_cam; dst->prior_n_pts = t.prior_n_pts;
    for (int k = 0; k < 3; ++k) dst->prior_rows[k] = t.prior_rows[k];
    if (L.carry) {
        dst->opt = src->opt;
        dst->loss_kind = src->loss_kind; dst->loss_scale = src->loss_scale;
        dst->inner_rounds = src->inner_rounds;
        dst->precond_kind = src->precond_kind;
        dst->schur_kind = src->schur_kind;
        dst->linear_kind = src->linear_kind;
        dst->precond_fallbacks = 0;
    }
    if (L.origin) {
        dst->has_origin = true;
        dst->origin_serial = src->serial; dst->origin_epoch = src->entity_epoch;
        dst->origin_n_cam = src->n_cam; dst->origin_n_pts = src->n_pts;
        dst->h_cam_of.swap(L.h_cam_of); dst->h_pt_of.swap(L.h_pt_of);
        dst->h_cam_role.swap(L.h_cam_role); dst->h_pt_role.swap(L.h_pt_role);
        dst->h_cam_role.resize((size_t)dst->n_cam, 0); dst->h_pt_role.resize((size_t)dst->n_pts, 0);
        dst->d_cam_of = std::move(L.cam_of); dst->d_pt_of = std::move(L.pt_of);
    }
}

// the parent's masks and priors gathered by the origin lists from its host mirrors, OR the roles, and installed in t by the
// setters themselves: one code path installs a mask or a prior and keeps its mirror and counts
int carry_masks_and_priors(const c2b_problem *src, c2b_problem *t, const ChildLists &L) {
    const size_t nc = (size_t)t->n_cam, np = (size_t)t->n_pts;
    std::vector<uint16_t> hc;
    std::vector<uint8_t> hp;
    if (!src->h_cmask.empty() || !L.h_cam_role.empty()) {
        hc.assign(nc, 0);
        for (size_t c = 0; c < nc; ++c)
            hc[c] = (uint16_t)((src->h_cmask.empty() ? 0 : src->h_cmask[L.h_cam_of[c]]) | (!L.h_cam_role.empty() && L.h_cam_role[c] ? C2B_CONST_ALL : 0));
    }
    if (!src->h_pmask.empty() || !L.h_pt_role.empty()) {
        hp.assign(np, 0);
        for (size_t i = 0; i < np; ++i)
            hp[i] = (uint8_t)((src->h_pmask.empty() ? 0 : src->h_pmask[L.h_pt_of[i]]) | (!L.h_pt_role.empty() && L.h_pt_role[i] ? 1 : 0));
    }
    if (!hc.empty() || !hp.empty())
        if (const int rc = c2b_problem_set_constant(t, hc.empty() ? nullptr : hc.data(), hp.empty() ? nullptr : hp.data())) return rc;
    std::vector<double> g[6];
    const std::vector<double> *kinds[6] = {&src->h_pc0, &src->h_pcw, &src->h_pi0, &src->h_piw, &src->h_px0, &src->h_pxw};
    bool any = false;
    for (int k = 0; k < 6; ++k) {
        if (kinds[k]->empty()) continue;
        const std::vector<uint32_t> &of = k < 4 ? L.h_cam_of : L.h_pt_of;
        g[k].resize(3 * of.size());
        for (size_t i = 0; i < of.size(); ++i)
            for (int j = 0; j < 3; ++j) g[k][3 * i + j] = (*kinds[k])[3 * (size_t)of[i] + j];
        any = any || !of.empty();
    }
    if (!any) return C2B_OK;
    auto ptr = [&](int k) { return kinds[k]->empty() || g[k].empty() ? nullptr : g[k].data(); };
    return c2b_problem_set_priors(t, ptr(0), ptr(1), ptr(2), ptr(3), ptr(4), ptr(5));
}

// The child of src by the lists, built in a problem of its own on src's stream and moved into dst only once everything has been
// queued and the stream has synchronised without error (install_observations' two phases): row counts through the camera
// list, their scan, the stable fill, cam_idx from the new row pointer, the entities by k_gather_rows exactly as cull gathers.
int build_child(c2b_problem *src, c2b_problem *dst, const char *who, ChildLists &L) {
    const int64_t nc = (int64_t)L.h_cam_of.size(), np = (int64_t)L.h_pt_of.size();
    hipStream_t st = src->stream;
    int rc = ensure_rows(src);
    if (rc) return rc;
    DevBuf<uint64_t> row_tot, row_new, scratch;
    hipError_t e = row_tot.alloc((size_t)nc + 1);
    if (e == hipSuccess) e = row_new.alloc((size_t)nc + 1);
    if (e == hipSuccess) e = scratch.alloc(scan_scratch_count(nc));
    if (e != hipSuccess) return fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    const unsigned row_blocks = (unsigned)((nc + 3) / 4);
    const bool rows = nc && src->n_obs;                       // (without observations the parent has no row pointer)
    uint64_t n_obs_new = 0;
    if (rows) {
        hipLaunchKernelGGL((k_keep_row_counts<RowVia, KeepMapped>), dim3(row_blocks), dim3(256), 0, st, (const uint64_t *)src->rows_ptr,
                           RowVia{L.cam_of}, KeepMapped{L.new_of}, (const uint32_t *)src->pt_idx, nc, row_tot.ptr);
        scan_by_length(st, (const uint64_t *)row_tot, nc, (uint64_t)0, row_new.ptr, row_new.ptr + nc, scratch.ptr);
        e = launch_error();
        if (e == hipSuccess) e = hipMemcpyAsync(&n_obs_new, row_new.ptr + nc, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    const int64_t no = (int64_t)n_obs_new;

    ScratchProblem sp;
    c2b_problem &t = sp.q;
    t.device = dst->device;
    t.stream = st;
    if ((rc = alloc_problem(&t, nc, np, no))) return rc;
    if (no) {
        hipLaunchKernelGGL((k_keep_row_scatter<RowVia, KeepMapped>), dim3(row_blocks), dim3(256), 0, st, (const uint64_t *)src->rows_ptr,
                           (const uint64_t *)row_new, RowVia{L.cam_of}, KeepMapped{L.new_of}, (const uint32_t *)src->pt_idx,
                           reinterpret_cast<const double2 *>(src->uv.ptr), nc, t.pt_idx.ptr, reinterpret_cast<double2 *>(t.uv.ptr));
        if ((rc = c2b_expand_rows(row_new, nc, 0, no, t.cam_idx, st))) return rc;
    }
    auto gather = [&](const double *in, const uint32_t *orig, int64_t n, int width, double *out) {
        if (n) hipLaunchKernelGGL(k_gather_rows, dim3(blocks_for(n * width, kBlock)), dim3(kBlock), 0, st, in, orig, n, width, out);
    };
    gather(src->cam15, L.cam_of, nc, 15, t.cam15);
    if (src->bal_valid) gather(src->bal9, L.cam_of, nc, 9, t.bal9);      // the truth alone, as cull gathers it
    gather(src->pts4, L.pt_of, np, 4, t.pts4);
    e = launch_error();
    if (e != hipSuccess) return fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    t.bal_valid = src->bal_valid;
    if (L.carry && (rc = carry_masks_and_priors(src, &t, L))) return rc;
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(hip_code(e), "%s: %s", who, hipGetErrorString(e));
    adopt_problem(dst, t, src, L);
    return C2B_OK;
}

int subset_pair_check(const char *who, const c2b_problem *src, const c2b_problem *dst) {
    if (!dst) return fail(C2B_ERR_INVALID_ARGUMENT, "%s: dst is NULL", who);
    if (dst == src) return fail(C2B_ERR_INVALID_ARGUMENT, "%s: dst is src (the child is a problem of its own)", who);
    if (dst->device != src->device)
        return fail(C2B_ERR_INVALID_ARGUMENT, "%s: src lives on device %d, dst on device %d", who, src->device, dst->device);
    if (src->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "%s: a shard is not cut alone (its list is a slice of the whole one)", who);
    if (src->n_pts >= ((int64_t)1 << 31) || src->n_cam >= ((int64_t)1 << 31))
        return fail(C2B_ERR_INVALID_ARGUMENT, "%s: 2^31 or more cameras or points", who);
    return C2B_OK;
}

// whether no index of the list (all < n) occurs twice
bool repeat_free(const std::vector<uint32_t> &sel, int64_t n) {
    std::vector<uint8_t> seen((size_t)n, 0);
    for (const uint32_t i : sel) {
        if (seen[i]) return false;
        seen[i] = 1;
    }
    return true;
}

}  // namespace
}  // extern "C++"

int c2b_problem_subset(c2b_problem *src, const uint32_t *cam_sel, int64_t n_cam_sel, const uint32_t *pt_sel, int64_t n_pt_sel, int flags,
                       c2b_problem *dst) {
    C2B_API_BEGIN
    if (!src || !dst) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_subset: NULL problem");
    if (n_cam_sel < 0 || n_pt_sel < 0 || (n_cam_sel && !cam_sel) || (n_pt_sel && !pt_sel))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_subset: a NULL list with a non-zero count, or a negative count");
    if (flags & ~C2B_SUBSET_CARRY) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_subset: unknown flag bits 0x%x", (unsigned)(flags & ~C2B_SUBSET_CARRY));
    if (n_cam_sel >= ((int64_t)1 << 31) || n_pt_sel >= ((int64_t)1 << 31))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_subset: 2^31 or more selected cameras or points");
    NEED_UPLOADED(src, "problem_subset");
    if (const int rc = subset_pair_check("problem_subset", src, dst)) return rc;
    for (int64_t i = 0; i < n_cam_sel; ++i)
        if (cam_sel[i] >= (uint64_t)src->n_cam)
            return fail(C2B_ERR_INDEX_OUT_OF_RANGE, "problem_subset: camera index %u at %lld out of range [0, %lld)", cam_sel[i], (long long)i,
                        (long long)src->n_cam);
    for (int64_t i = 0; i < n_pt_sel; ++i)
        if (pt_sel[i] >= (uint64_t)src->n_pts)
            return fail(C2B_ERR_INDEX_OUT_OF_RANGE, "problem_subset: point index %u at %lld out of range [0, %lld)", pt_sel[i], (long long)i,
                        (long long)src->n_pts);
    ChildLists L;
    if (n_cam_sel) L.h_cam_of.assign(cam_sel, cam_sel + n_cam_sel);
    if (n_pt_sel) L.h_pt_of.assign(pt_sel, pt_sel + n_pt_sel);
    L.carry = (flags & C2B_SUBSET_CARRY) != 0;
    L.origin = L.carry && repeat_free(L.h_cam_of, src->n_cam) && repeat_free(L.h_pt_of, src->n_pts);
    hipStream_t st = src->stream;
    hipError_t e = L.cam_of.alloc((size_t)n_cam_sel);
    if (e == hipSuccess) e = L.pt_of.alloc((size_t)n_pt_sel);
    if (e == hipSuccess) e = L.new_of.alloc((size_t)src->n_pts);
    if (e == hipSuccess && n_cam_sel) e = hipMemcpyAsync(L.cam_of, cam_sel, sizeof(uint32_t) * (size_t)n_cam_sel, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_pt_sel) e = hipMemcpyAsync(L.pt_of, pt_sel, sizeof(uint32_t) * (size_t)n_pt_sel, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && src->n_pts) e = hipMemsetAsync(L.new_of, 0xff, sizeof(int32_t) * (size_t)src->n_pts, st);      // -1: no slot
    if (e == hipSuccess && n_pt_sel) {
        hipLaunchKernelGGL(k_subset_point_map, dim3(blocks_for(n_pt_sel, 256)), dim3(256), 0, st, (const uint32_t *)L.pt_of, n_pt_sel, L.new_of.ptr);
        e = launch_error();
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(hip_code(e), "problem_subset: %s", hipGetErrorString(e));
    }
    const int rc = build_child(src, dst, "problem_subset", L);
    (void)hipStreamSynchronize(st);                           // the lists are freed here
    return rc;
    C2B_API_END("problem_subset")
}

int c2b_problem_window(c2b_problem *src, const uint8_t *seed, int flags, c2b_problem *dst) {
    C2B_API_BEGIN
    if (!src || !dst || !seed) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_window: NULL argument");
    if (flags & ~C2B_WINDOW_HALO) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_window: unknown flag bits 0x%x", (unsigned)(flags & ~C2B_WINDOW_HALO));
    NEED_UPLOADED(src, "problem_window");
    if (const int rc = subset_pair_check("problem_window", src, dst)) return rc;
    const int64_t n_cam = src->n_cam, n_pts = src->n_pts, n_obs = src->n_obs;
    int64_t n_seed = 0;
    for (int64_t c = 0; c < n_cam; ++c) n_seed += seed[c] != 0;
    if (!n_seed) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_window: no seed camera");
    const bool halo = (flags & C2B_WINDOW_HALO) != 0;
    hipStream_t st = src->stream;
    // the marks, their scans and the lists: temporaries of one arena
    DevBuf<uint8_t> d_seed, shared, cam_role, pt_role;
    DevBuf<uint32_t> cam_flag, in_P, cam_pos, pt_pos, tiles, totals;
    DevArena arena;
    auto temporaries = [&](auto &&each) {
        each(d_seed, (size_t)n_cam); each(shared, (size_t)n_pts); each(cam_flag, (size_t)n_cam); each(in_P, (size_t)n_pts);
        each(cam_pos, (size_t)n_cam); each(pt_pos, (size_t)n_pts); each(tiles, scan_scratch_count(std::max(n_cam, n_pts))); each(totals, (size_t)2);
    };
    size_t arena_bytes = 0;
    temporaries([&](auto &b, size_t n) { arena_bytes += DevArena::room(b, n); });
    hipError_t e = arena.reserve(arena_bytes);
    if (e != hipSuccess) return fail(hip_code(e), "problem_window: %s", hipGetErrorString(e));
    temporaries([&](auto &b, size_t n) { arena.carve(b, n); });
    struct SyncOnExit { hipStream_t s; ~SyncOnExit() { (void)hipStreamSynchronize(s); } } sync_on_exit{st};      // before the arena is freed
    e = hipMemcpyAsync(d_seed, seed, (size_t)n_cam, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_pts) e = hipMemsetAsync(in_P, 0, sizeof(uint32_t) * (size_t)n_pts, st);
    if (e == hipSuccess && n_pts) e = hipMemsetAsync(shared, 0, (size_t)n_pts, st);
    uint32_t h_tot[2] = {0, 0};
    if (e == hipSuccess) {
        const unsigned go = blocks_for(n_obs, 256);
        hipLaunchKernelGGL(k_window_seed_flags, dim3(blocks_for(n_cam, 256)), dim3(256), 0, st, (const uint8_t *)d_seed, n_cam, cam_flag.ptr);
        if (n_obs) {
            hipLaunchKernelGGL(k_window_mark_points, dim3(go), dim3(256), 0, st, (const uint32_t *)src->cam_idx, (const uint32_t *)src->pt_idx, n_obs,
                               (const uint8_t *)d_seed, in_P.ptr);
            if (halo)
                hipLaunchKernelGGL(k_window_mark_rim<true>, dim3(go), dim3(256), 0, st, (const uint32_t *)src->cam_idx, (const uint32_t *)src->pt_idx,
                                   n_obs, (const uint8_t *)d_seed, (const uint32_t *)in_P, cam_flag.ptr, shared.ptr);
            else
                hipLaunchKernelGGL(k_window_mark_rim<false>, dim3(go), dim3(256), 0, st, (const uint32_t *)src->cam_idx, (const uint32_t *)src->pt_idx,
                                   n_obs, (const uint8_t *)d_seed, (const uint32_t *)in_P, cam_flag.ptr, shared.ptr);
        }
        scan_by_length(st, (const uint32_t *)cam_flag, n_cam, 0u, cam_pos.ptr, totals.ptr, tiles.ptr);
        scan_by_length(st, (const uint32_t *)in_P, n_pts, 0u, pt_pos.ptr, totals.ptr + 1, tiles.ptr);
        e = launch_error();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_tot, totals, sizeof h_tot, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(hip_code(e), "problem_window: %s", hipGetErrorString(e));
    const int64_t nc = h_tot[0], np = h_tot[1];
    ChildLists L;
    L.carry = L.origin = true;
    L.h_cam_of.resize((size_t)nc); L.h_pt_of.resize((size_t)np); L.h_cam_role.resize((size_t)nc); L.h_pt_role.resize((size_t)np);
    e = L.cam_of.alloc((size_t)nc);
    if (e == hipSuccess) e = L.pt_of.alloc((size_t)np);
    if (e == hipSuccess) e = L.new_of.alloc((size_t)n_pts);
    if (e == hipSuccess) e = cam_role.alloc((size_t)nc);
    if (e == hipSuccess) e = pt_role.alloc((size_t)np);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_window_lists, dim3(blocks_for(std::max(n_cam, n_pts), 256)), dim3(256), 0, st, (const uint32_t *)cam_flag,
                           (const uint32_t *)cam_pos, n_cam, (const uint8_t *)d_seed, (const uint32_t *)in_P, (const uint32_t *)pt_pos, n_pts,
                           (const uint8_t *)shared, L.cam_of.ptr, cam_role.ptr, L.pt_of.ptr, pt_role.ptr, L.new_of.ptr);
        e = launch_error();
    }
    // the origin lists are what leaves the device: 5 bytes per entity of the child
    if (e == hipSuccess && nc) e = hipMemcpyAsync(L.h_cam_of.data(), L.cam_of, sizeof(uint32_t) * (size_t)nc, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && nc) e = hipMemcpyAsync(L.h_cam_role.data(), cam_role, (size_t)nc, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && np) e = hipMemcpyAsync(L.h_pt_of.data(), L.pt_of, sizeof(uint32_t) * (size_t)np, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && np) e = hipMemcpyAsync(L.h_pt_role.data(), pt_role, (size_t)np, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(hip_code(e), "problem_window: %s", hipGetErrorString(e));
    return build_child(src, dst, "problem_window", L);
    C2B_API_END("problem_window")
}

int c2b_problem_get_origin(const c2b_problem *child, uint32_t *cam_of, uint32_t *pt_of, uint8_t *cam_role, uint8_t *pt_role) {
    C2B_API_BEGIN
    if (!child) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_origin: problem is NULL");
    if (!child->has_origin) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_origin: the problem has no origin");
    if (cam_of) std::copy(child->h_cam_of.begin(), child->h_cam_of.end(), cam_of);
    if (pt_of) std::copy(child->h_pt_of.begin(), child->h_pt_of.end(), pt_of);
    if (cam_role) std::copy(child->h_cam_role.begin(), child->h_cam_role.end(), cam_role);
    if (pt_role) std::copy(child->h_pt_role.begin(), child->h_pt_role.end(), pt_role);
    return C2B_OK;
    C2B_API_END("problem_get_origin")
}

// Worded as c2b_problem_apply_step is: bal9 made editable on both sides, the scatters on the parent's stream once the child's
// has drained, bal9 the truth of the parent (and of a child that was in state mode) afterwards.
int c2b_problem_write_back(c2b_problem *child, c2b_problem *parent, int64_t *n_cam_written, int64_t *n_pts_written) {
    C2B_API_BEGIN
    if (!child || !parent) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_write_back: NULL problem");
    if (child == parent) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_write_back: the child is the parent");
    if (!child->has_origin) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_write_back: the child has no origin");
    if (child->device != parent->device)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_write_back: the child lives on device %d, the parent on device %d", child->device, parent->device);
    if (child->shard_n_cam_global >= 0 || parent->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_write_back: a shard takes no part in a write-back");
    if (parent->serial != child->origin_serial)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_write_back: the child was not taken from this parent");
    if (parent->entity_epoch != child->origin_epoch || parent->n_cam != child->origin_n_cam || parent->n_pts != child->origin_n_pts)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_write_back: the parent's cameras or points were replaced or renumbered since the child was taken");
    NEED_UPLOADED(child, "problem_write_back");
    NEED_UPLOADED(parent, "problem_write_back");
    const int64_t nc = child->n_cam, np = child->n_pts;
    const bool child_state = !child->bal_valid;
    int rc = bal9_edit_begin(parent);                         // state mode: the entries written are those of to_vec(cam15)
    if (!rc) rc = bal9_edit_begin(child);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(child->stream));
    hipStream_t st = parent->stream;
    if (nc) hipLaunchKernelGGL(k_scatter_free_cameras, dim3(blocks_for(9 * nc, 256)), dim3(256), 0, st, (const double *)child->bal9,
                               (const uint32_t *)child->d_cam_of, (const uint16_t *)child->cmask, nc, parent->bal9.ptr);
    if (np) hipLaunchKernelGGL(k_scatter_free_points, dim3(blocks_for(np, 256)), dim3(256), 0, st, reinterpret_cast<const double4 *>(child->pts4.ptr),
                               (const uint32_t *)child->d_pt_of, (const uint8_t *)child->pmask, np, reinterpret_cast<double4 *>(parent->pts4.ptr));
    LAUNCH_CHECK();
    rc = bal9_edit_end(parent, C2B_OK);                       // the cameras' caches only: list, rows, transpose, solve buffers, masks stay
    if (!rc && child_state) rc = bal9_edit_end(child, C2B_OK);
    const hipError_t e1 = hipStreamSynchronize(st), e2 = hipStreamSynchronize(child->stream);
    if (rc) return rc;
    if (e1 != hipSuccess || e2 != hipSuccess)
        return fail(C2B_ERR_HIP, "problem_write_back: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    int64_t cams = nc, pts = np;
    if (child->cmask) {
        cams = 0;
        for (const uint16_t m : child->h_cmask) cams += (m & C2B_CONST_ALL) != C2B_CONST_ALL;
    }
    if (child->pmask) {
        pts = 0;
        for (const uint8_t m : child->h_pmask) pts += m == 0;
    }
    if (n_cam_written) *n_cam_written = cams;
    if (n_pts_written) *n_pts_written = pts;
    return C2B_OK;
    C2B_API_END("problem_write_back")
}
