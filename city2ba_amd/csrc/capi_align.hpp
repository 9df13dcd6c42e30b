// capi_align.hpp -- similarity alignment against ground truth (include/city2ba_hip_experimental.h): the host arithmetic's
// entries, Level 0 over device tables, and Level 1 on two resident problems (c2b_problem_align, c2b_problem_transform).
// Part of the one translation unit of the C ABI: included by capi.hip (inside its extern "C" block, after capi_problem.hpp), never
// compiled or included on its own.  All device memory of Level 1 is a DevBuf<T>.

static AlignSim align_sim(const c2b_similarity &s) {
    AlignSim T;
    T.s = s.scale;
    std::copy(s.rotation, s.rotation + 9, T.R);
    std::copy(s.translation, s.translation + 3, T.t);
    return T;
}
static c2b_similarity align_public(const c2b_host::Similarity &h) {
    c2b_similarity s;
    s.scale = h.s;
    std::copy(h.R, h.R + 9, s.rotation);
    std::copy(h.t, h.t + 3, s.translation);
    return s;
}
static int align_grid(int64_t n) { return stats_grid(n, kAlignBlock, kAlignGrid); }

void c2b_align_options_init(c2b_align_options *o) {
    if (o) *o = c2b_align_options{C2B_ALIGN_CAMERAS, 1, 0, 0, 0.0, nullptr, nullptr};
}

int c2b_similarity_from_moments(int64_t n, const double mean_x[3], const double mean_y[3], double var_x, double var_y, const double cov9[9],
                                int scale, c2b_similarity *sim, int *status) {
    C2B_API_BEGIN
    if (!mean_x || !mean_y || !cov9 || !sim || !status) return fail(C2B_ERR_INVALID_ARGUMENT, "similarity_from_moments: NULL argument");
    if (n < 0 || !(var_x >= 0.0) || !(var_y >= 0.0)) return fail(C2B_ERR_INVALID_ARGUMENT, "similarity_from_moments: n, var_x and var_y must be >= 0");
    c2b_host::Similarity T;
    *status = c2b_host::similarity_from_moments(n, mean_x, mean_y, var_x, cov9, scale != 0, T);
    *sim = align_public(T);
    return C2B_OK;
    C2B_API_END("similarity_from_moments")
}

int c2b_align_finish_moments(const double means7[7], const double moments23[23], double *n, double mean_x[3], double mean_y[3],
                             double *var_x, double *var_y, double cov9[9]) {
    C2B_API_BEGIN
    if (!means7 || !moments23 || !n || !mean_x || !mean_y || !var_x || !var_y || !cov9)
        return fail(C2B_ERR_INVALID_ARGUMENT, "align_finish_moments: NULL argument");
    c2b_host::align_finish_moments(means7, moments23, n, mean_x, mean_y, var_x, var_y, cov9);
    return C2B_OK;
    C2B_API_END("align_finish_moments")
}

int c2b_align_launch_shape(int *threads_per_workgroup, int *max_workgroups, int *entities_per_trip) {
    if (threads_per_workgroup) *threads_per_workgroup = kAlignBlock;
    if (max_workgroups) *max_workgroups = kAlignGrid;
    if (entities_per_trip) *entities_per_trip = kAlignBatch;
    return C2B_OK;
}

// ---- Level 0 -----------------------------------------------------------------------------------------------------------------------
static int align_src_args(const char *who, const double *xc, const double *yc, int64_t n_cam, const double *xp, const double *yp, int64_t n_pts,
                          const void *workspace, const void *out) {
    if (n_cam < 0 || n_pts < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "%s: negative count", who);
    if (!workspace || !out || (n_cam && (!xc || !yc)) || (n_pts && (!xp || !yp))) return fail(C2B_ERR_INVALID_ARGUMENT, "%s: NULL pointer", who);
    if (!aligned16(xc) || !aligned16(yc) || !aligned16(xp) || !aligned16(yp) || !aligned8(out) || (reinterpret_cast<uintptr_t>(workspace) & 127))
        return fail(C2B_ERR_INVALID_ARGUMENT, "%s: misaligned pointer (tables: 16 bytes, workspace: 128, results: 8)", who);
    return C2B_OK;
}

int c2b_align_means_rows(const double *x_cam4, const double *y_cam4, const uint8_t *use_cam, int64_t n_cam, const double *x_pts4,
                         const double *y_pts4, const uint8_t *use_pt, int64_t n_pts, void *workspace, double *means7, void *stream) {
    C2B_API_BEGIN
    if (int rc = align_src_args("align_means_rows", x_cam4, y_cam4, n_cam, x_pts4, y_pts4, n_pts, workspace, means7)) return rc;
    const int64_t n = n_cam + n_pts;
    const AlignSrc src{x_cam4, y_cam4, use_cam, n_cam, x_pts4, y_pts4, use_pt};
    hipLaunchKernelGGL(k_align_means, dim3(align_grid(n)), dim3(kAlignBlock), 0, S(stream), src, n, reinterpret_cast<double *>(workspace),
                       ws_ticket(workspace), means7);
    LAUNCH_CHECK();
    return C2B_OK;
    C2B_API_END("align_means_rows")
}

int c2b_align_moments_rows(const double *x_cam4, const double *y_cam4, const uint8_t *use_cam, int64_t n_cam, const double *x_pts4,
                           const double *y_pts4, const uint8_t *use_pt, int64_t n_pts, const double *means7, void *workspace,
                           double *moments23, void *stream) {
    C2B_API_BEGIN
    if (int rc = align_src_args("align_moments_rows", x_cam4, y_cam4, n_cam, x_pts4, y_pts4, n_pts, workspace, moments23)) return rc;
    if (!means7 || !aligned8(means7)) return fail(C2B_ERR_INVALID_ARGUMENT, "align_moments_rows: means7 is NULL or misaligned");
    const int64_t n = n_cam + n_pts;
    const AlignSrc src{x_cam4, y_cam4, use_cam, n_cam, x_pts4, y_pts4, use_pt};
    hipLaunchKernelGGL(k_align_moments, dim3(align_grid(n)), dim3(kAlignBlock), 0, S(stream), src, n, means7,
                       reinterpret_cast<double *>(workspace), ws_ticket(workspace), moments23);
    LAUNCH_CHECK();
    return C2B_OK;
    C2B_API_END("align_moments_rows")
}

int c2b_align_errors_rows(const double *x4, const double *y4, int64_t n, const c2b_similarity *sim, const uint8_t *base, const uint8_t *use,
                          double max_dist, double *err, uint8_t *next, void *workspace, double *summary7, void *stream) {
    C2B_API_BEGIN
    if (n < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "align_errors_rows: negative count");
    if (!sim || !workspace || !summary7 || (n && (!x4 || !y4))) return fail(C2B_ERR_INVALID_ARGUMENT, "align_errors_rows: NULL pointer");
    if (!aligned16(x4) || !aligned16(y4) || !aligned8(err) || !aligned8(summary7) || (reinterpret_cast<uintptr_t>(workspace) & 127))
        return fail(C2B_ERR_INVALID_ARGUMENT, "align_errors_rows: misaligned pointer (tables: 16 bytes, workspace: 128, results: 8)");
    if (next && next == use) return fail(C2B_ERR_INVALID_ARGUMENT, "align_errors_rows: next must not be use");
    if (std::isnan(max_dist)) return fail(C2B_ERR_INVALID_ARGUMENT, "align_errors_rows: max_dist is NaN");
    return align_errors_launch(AlignPosErr{x4, y4, align_sim(*sim)}, n, base, use, max_dist, err, next, workspace, summary7, S(stream));
    C2B_API_END("align_errors_rows")
}

int c2b_align_rotation_errors_rows(const double *x_cam15, const double *y_cam15, int64_t n, const c2b_similarity *sim, const uint8_t *use,
                                   double *err, void *workspace, double *summary7, void *stream) {
    C2B_API_BEGIN
    if (n < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "align_rotation_errors_rows: negative count");
    if (!sim || !workspace || !summary7 || (n && (!x_cam15 || !y_cam15))) return fail(C2B_ERR_INVALID_ARGUMENT, "align_rotation_errors_rows: NULL pointer");
    if (!aligned8(x_cam15) || !aligned8(y_cam15) || !aligned8(err) || !aligned8(summary7) || (reinterpret_cast<uintptr_t>(workspace) & 127))
        return fail(C2B_ERR_INVALID_ARGUMENT, "align_rotation_errors_rows: misaligned pointer (tables, results: 8 bytes, workspace: 128)");
    return align_errors_launch(AlignRotErr{x_cam15, y_cam15, align_sim(*sim)}, n, nullptr, use, 0.0, err, nullptr, workspace, summary7, S(stream));
    C2B_API_END("align_rotation_errors_rows")
}

int c2b_similarity_apply(double *cam15, int64_t n_cam, double *pts4, int64_t n_pts, const c2b_similarity *sim, void *stream) {
    C2B_API_BEGIN
    if (n_cam < 0 || n_pts < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "similarity_apply: negative count");
    if (!sim || (n_cam && !cam15) || (n_pts && !pts4)) return fail(C2B_ERR_INVALID_ARGUMENT, "similarity_apply: NULL pointer");
    if (!aligned8(cam15) || !aligned16(pts4)) return fail(C2B_ERR_INVALID_ARGUMENT, "similarity_apply: misaligned pointer (cam15: 8 bytes, pts4: 16)");
    const c2b_host::Similarity h{sim->scale, {sim->rotation[0], sim->rotation[1], sim->rotation[2], sim->rotation[3], sim->rotation[4],
                                              sim->rotation[5], sim->rotation[6], sim->rotation[7], sim->rotation[8]},
                                 {sim->translation[0], sim->translation[1], sim->translation[2]}};
    if (const char *why = c2b_host::similarity_defect(h)) return fail(C2B_ERR_INVALID_ARGUMENT, "similarity_apply: %s", why);
    const AlignSim T = align_sim(*sim);
    hipStream_t st = S(stream);
    if (n_cam) hipLaunchKernelGGL(k_similarity_apply_cameras, dim3(blocks_for(n_cam)), dim3(kBlock), 0, st, cam15, n_cam, T);
    if (n_pts) hipLaunchKernelGGL(k_similarity_apply_points, dim3(blocks_for(n_pts)), dim3(kBlock), 0, st, pts4, n_pts, T);
    LAUNCH_CHECK();
    return C2B_OK;
    C2B_API_END("similarity_apply")
}

// ---- Level 1 -----------------------------------------------------------------------------------------------------------------------
// the centre table of a problem, on its own stream (compute_stats's rule: the centres alone where only they are stale), waited for
static int align_centres(c2b_problem *p) {
    if (!p->n_cam) return C2B_OK;
    if (!p->blk_valid && !p->bal_valid) {
        hipLaunchKernelGGL(k_cameras_centers, dim3(blocks_for(p->n_cam)), dim3(kBlock), 0, S(p->stream), p->cam15, p->n_cam, p->cen4);
        LAUNCH_CHECK();
    } else if (int rc = ensure_camblk(p)) {
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
}

static int align_pair_check(const char *who, const c2b_problem *p, const c2b_problem *ref) {
    if (p->device != ref->device) return fail(C2B_ERR_INVALID_ARGUMENT, "%s: the two problems live on different devices", who);
    if (p->shard_n_cam_global >= 0 || ref->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "%s: a shard is not aligned alone", who);
    if (p->n_cam != ref->n_cam || p->n_pts != ref->n_pts)
        return fail(C2B_ERR_INVALID_ARGUMENT, "%s: sizes differ (%lld cameras, %lld points against %lld, %lld): index i of one must correspond to index i of the other",
                    who, (long long)p->n_cam, (long long)p->n_pts, (long long)ref->n_cam, (long long)ref->n_pts);
    return C2B_OK;
}

static c2b_align_stat align_stat(const double *s) { return c2b_align_stat{(int64_t)s[0], (int64_t)s[4], s[1], s[2], s[3]}; }

int c2b_problem_align(c2b_problem *p, c2b_problem *ref, const c2b_align_options *opt, c2b_similarity *sim, c2b_align_summary *summary,
                      double *cam_err, double *cam_rot_err, double *pt_err, uint8_t *cam_inlier, uint8_t *pt_inlier) {
    C2B_API_BEGIN
    NEED_UPLOADED(ref, "problem_align");
    NEED_UPLOADED(p, "problem_align");
    if (!opt || !sim) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_align: opt or sim is NULL");
    if (int rc = align_pair_check("problem_align", p, ref)) return rc;
    if (opt->on < C2B_ALIGN_CAMERAS || opt->on > C2B_ALIGN_BOTH || opt->rounds < 0 || opt->reserved != 0 || std::isnan(opt->max_dist))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_align: on must be C2B_ALIGN_CAMERAS, _POINTS or _BOTH, rounds >= 0, reserved 0, max_dist a number");
    const int64_t nc = p->n_cam, np = p->n_pts;
    const bool fit_cam = (opt->on & C2B_ALIGN_CAMERAS) != 0, fit_pt = (opt->on & C2B_ALIGN_POINTS) != 0;
    const bool trim = opt->max_dist > 0.0 && opt->rounds >= 1;
    hipStream_t st = p->stream;
    if (int rc = align_centres(ref)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (int rc = align_centres(p)) return rc;

    // the caller's masks (a), two sets to alternate between (b, c), the per-entity errors, the scalars of the passes
    DevBuf<uint8_t> cam_a, cam_b, cam_c, pt_a, pt_b, pt_c;
    DevBuf<double> d_cam_err, d_rot_err, d_pt_err, d_out;
    constexpr int kMeansAt = 0, kMomAt = 8, kSumAt = 32;                  // in d_out: means [7], moments [23], three summaries [7]
    HIP_TRY(d_out.alloc(kSumAt + 3 * 8));
    auto mask_up = [&](DevBuf<uint8_t> &a, DevBuf<uint8_t> &b, DevBuf<uint8_t> &c, const uint8_t *host, int64_t n) -> hipError_t {
        hipError_t e = hipSuccess;
        if (host && n) {
            e = a.alloc((size_t)n);
            if (e == hipSuccess) e = hipMemcpyAsync(a, host, (size_t)n, hipMemcpyHostToDevice, st);
        }
        if (e == hipSuccess && n && trim) e = b.alloc((size_t)n);
        if (e == hipSuccess && n && trim) e = c.alloc((size_t)n);
        return e;
    };
    HIP_TRY(mask_up(cam_a, cam_b, cam_c, opt->use_cam, nc));
    HIP_TRY(mask_up(pt_a, pt_b, pt_c, opt->use_pt, np));
    if (cam_err && nc) HIP_TRY(d_cam_err.alloc((size_t)nc));
    if (cam_rot_err && nc) HIP_TRY(d_rot_err.alloc((size_t)nc));
    if (pt_err && np) HIP_TRY(d_pt_err.alloc((size_t)np));

    // one fit over the sets (cam_use, pt_use: NULL = all on) of the kinds in `on`
    auto fit = [&](const uint8_t *cam_use, const uint8_t *pt_use, c2b_host::Similarity &T, int &status) -> int {
        const int64_t fc = fit_cam ? nc : 0, fp = fit_pt ? np : 0;
        double h[kSumAt] = {0};
        if (fc + fp) {
            int rc = c2b_align_means_rows(p->cen4, ref->cen4, cam_use, fc, p->pts4, ref->pts4, pt_use, fp, p->ws, d_out + kMeansAt, st);
            if (!rc) rc = c2b_align_moments_rows(p->cen4, ref->cen4, cam_use, fc, p->pts4, ref->pts4, pt_use, fp, d_out + kMeansAt, p->ws, d_out + kMomAt, st);
            if (!rc) rc = scalars_to_host(st, d_out, kSumAt, h);
            if (rc) return rc;
        }
        double n, mx[3], my[3], vx, vy, cov[9];
        c2b_host::align_finish_moments(h + kMeansAt, h + kMomAt, &n, mx, my, &vx, &vy, cov);
        status = c2b_host::similarity_from_moments((int64_t)n, mx, my, vx, cov, opt->scale != 0, T);
        return C2B_OK;
    };
    // the errors under T: per kind, `use` summarised, `next` (may be NULL) = the caller's mask && e <= max_dist; the summaries to the host
    auto errors = [&](const c2b_host::Similarity &T, const uint8_t *cam_use, const uint8_t *pt_use, uint8_t *cam_next, uint8_t *pt_next,
                      bool keep_err, double *h) -> int {
        const c2b_similarity s = align_public(T);
        const double md = trim ? opt->max_dist : 0.0;
        int rc = c2b_align_errors_rows(p->cen4, ref->cen4, nc, &s, cam_a, cam_use, fit_cam ? md : 0.0, keep_err ? d_cam_err.ptr : nullptr, cam_next,
                                       p->ws, d_out + kSumAt, st);
        if (!rc) rc = c2b_align_errors_rows(p->pts4, ref->pts4, np, &s, pt_a, pt_use, fit_pt ? md : 0.0, keep_err ? d_pt_err.ptr : nullptr, pt_next,
                                            p->ws, d_out + kSumAt + 8, st);
        if (!rc && keep_err) rc = c2b_align_rotation_errors_rows(p->cam15, ref->cam15, nc, &s, cam_use, d_rot_err, p->ws, d_out + kSumAt + 16, st);
        if (!rc) rc = scalars_to_host(st, d_out + kSumAt, 24, h);
        return rc;
    };

    c2b_host::Similarity T;
    int status = C2B_ALIGN_OK, refits = 0;
    if (int rc = fit(cam_a, pt_a, T, status)) return rc;
    if (status != C2B_ALIGN_OK) {                            // rule 3: the identity, nothing else written
        *sim = align_public(c2b_host::similarity_identity());
        if (summary) {
            *summary = c2b_align_summary{};
            summary->status = status;
            summary->cameras.argmax = summary->camera_rotations.argmax = summary->points.argmax = -1;
        }
        return C2B_OK;
    }
    const uint8_t *cam_cur = cam_a, *pt_cur = pt_a;          // the set T was fitted on
    uint8_t *cam_nxt = cam_b, *pt_nxt = pt_b;
    const uint8_t *cam_fin = cam_a, *pt_fin = pt_a;          // the set the summaries run over
    double h[24];
    if (trim) {
        for (int r = 0; r < opt->rounds; ++r) {
            if (int rc = errors(T, cam_cur, pt_cur, fit_cam ? cam_nxt : nullptr, fit_pt ? pt_nxt : nullptr, false, h)) return rc;
            const double changed = (fit_cam ? h[5] : 0.0) + (fit_pt ? h[8 + 5] : 0.0), n_next = (fit_cam ? h[6] : 0.0) + (fit_pt ? h[8 + 6] : 0.0);
            if (changed == 0.0) break;                       // the set repeats
            const uint8_t *cam_try = fit_cam ? cam_nxt : cam_cur, *pt_try = fit_pt ? pt_nxt : pt_cur;
            c2b_host::Similarity T2;
            int st2 = C2B_ALIGN_TOO_FEW;
            if (n_next >= 3.0) {
                if (int rc = fit(cam_try, pt_try, T2, st2)) return rc;
            }
            if (st2 != C2B_ALIGN_OK) {                       // the last good transform, the set that failed
                status = st2;
                cam_fin = cam_try; pt_fin = pt_try;
                break;
            }
            T = T2;
            ++refits;
            cam_fin = cam_cur = cam_try; pt_fin = pt_cur = pt_try;
            if (fit_cam) cam_nxt = cam_nxt == cam_b.ptr ? cam_c.ptr : cam_b.ptr;
            if (fit_pt) pt_nxt = pt_nxt == pt_b.ptr ? pt_c.ptr : pt_b.ptr;
        }
    }
    if (int rc = errors(T, cam_fin, pt_fin, nullptr, nullptr, true, h)) return rc;
    // the outputs
    auto mask_down = [&](uint8_t *host, const uint8_t *dev, int64_t n) -> hipError_t {
        if (!host || !n) return hipSuccess;
        if (!dev) { std::fill(host, host + n, (uint8_t)1); return hipSuccess; }
        return hipMemcpyAsync(host, dev, (size_t)n, hipMemcpyDeviceToHost, st);
    };
    HIP_TRY(mask_down(cam_inlier, cam_fin, nc));
    HIP_TRY(mask_down(pt_inlier, pt_fin, np));
    if (cam_err && nc) HIP_TRY(hipMemcpyAsync(cam_err, d_cam_err, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost, st));
    if (cam_rot_err && nc) HIP_TRY(hipMemcpyAsync(cam_rot_err, d_rot_err, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost, st));
    if (pt_err && np) HIP_TRY(hipMemcpyAsync(pt_err, d_pt_err, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *sim = align_public(T);
    if (summary) {
        summary->status = status;
        summary->rounds = refits;
        summary->cameras = align_stat(h);
        summary->points = align_stat(h + 8);
        summary->camera_rotations = align_stat(h + 16);
    }
    return C2B_OK;
    C2B_API_END("problem_align")
}

int c2b_problem_transform(c2b_problem *p, const c2b_similarity *sim) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_transform");
    if (!sim) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_transform: sim is NULL");
    if (p->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_transform: a shard is not transformed alone (the points are replicated on every rank)");
    if (int rc = c2b_similarity_apply(p->cam15, p->n_cam, p->pts4, p->n_pts, sim, p->stream)) return rc;
    cameras_mutated(p);                                      // the arithmetic-noise row of the cache table
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_transform")
}
