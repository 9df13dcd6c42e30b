// capi_solve.hpp -- Level 1, the solver side of the resident problem: constant parameters, robust loss, preconditioner, normal equations, the damped
// Gauss-Newton step (implicit Schur complement + PCG), apply_step, triangulation, checkpoint / rollback and Levenberg-Marquardt on the device
// Part of the one translation unit of the C ABI: included by capi_problem.hpp where this text sat, never compiled or included on its own.

// ---- constant parameters -----------------------------------------------------------------------------------
int c2b_problem_set_constant(c2b_problem *p, const uint16_t *cam_mask, const uint8_t *pt_mask) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_set_constant");
    const int64_t nc = p->n_cam, np = p->n_pts;
    int64_t n_params = 0, n_const_pts = 0;
    if (cam_mask)
        for (int64_t c = 0; c < nc; ++c) {
            if (cam_mask[c] & ~C2B_CONST_ALL)
                return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_constant: camera %lld has a bit above bit 8 set (0x%x)", (long long)c,
                            (unsigned)cam_mask[c]);
            n_params += __builtin_popcount(cam_mask[c]);
        }
    if (pt_mask)
        for (int64_t i = 0; i < np; ++i) {
            if (pt_mask[i] > 1)
                return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_constant: point %lld has mask %d, not 0 or 1", (long long)i, (int)pt_mask[i]);
            n_const_pts += pt_mask[i];
        }
    // the new device arrays first: a failure leaves the masks in force as they were.  An all-zero mask is no mask.
    std::vector<uint16_t> hc;
    std::vector<uint8_t> hp;
    DevBuf<uint16_t> dcm;
    DevBuf<uint8_t> dpm;
    hipError_t e = hipSuccess;
    if (n_params) {
        hc.assign(cam_mask, cam_mask + nc);
        e = dcm.alloc((size_t)nc);
        if (e == hipSuccess) e = hipMemcpyAsync(dcm, hc.data(), sizeof(uint16_t) * (size_t)nc, hipMemcpyHostToDevice, p->stream);
    }
    if (e == hipSuccess && n_const_pts) {
        hp.assign(pt_mask, pt_mask + np);
        e = dpm.alloc((size_t)np);
        if (e == hipSuccess) e = hipMemcpyAsync(dpm, hp.data(), sizeof(uint8_t) * (size_t)np, hipMemcpyHostToDevice, p->stream);
    }
    const hipError_t es = hipStreamSynchronize(p->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(hip_code(e), "problem_set_constant: %s", hipGetErrorString(e));
    drop_constant(p);
    p->cmask = std::move(dcm); p->pmask = std::move(dpm);
    p->h_cmask.swap(hc); p->h_pmask.swap(hp);
    p->const_n_cam = nc; p->const_n_pts = np;
    p->const_params = n_params; p->const_pts = n_const_pts;
    return C2B_OK;
    C2B_API_END("problem_set_constant")
}

int c2b_problem_get_constant(const c2b_problem *p, uint16_t *cam_mask, uint8_t *pt_mask, int64_t *n_const_cam_params, int64_t *n_const_pts) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_constant: problem is NULL");
    if (!p->ws) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_constant: nothing uploaded");
    if (cam_mask) {
        if (p->cmask) std::copy(p->h_cmask.begin(), p->h_cmask.end(), cam_mask);
        else std::fill(cam_mask, cam_mask + p->n_cam, (uint16_t)0);
    }
    if (pt_mask) {
        if (p->pmask) std::copy(p->h_pmask.begin(), p->h_pmask.end(), pt_mask);
        else std::fill(pt_mask, pt_mask + p->n_pts, (uint8_t)0);
    }
    if (n_const_cam_params) *n_const_cam_params = p->const_params;
    if (n_const_pts) *n_const_pts = p->const_pts;
    return C2B_OK;
    C2B_API_END("problem_get_constant")
}

// the zeros of J~ into blocks the passes filled from J (asynchronous; nothing is launched for a kind with nothing constant):
// rows and columns of A [n_cam][9][9] with `diag` on their diagonal, entries of y [n_cam][9] (either may be NULL) ...
static int constant_cameras(c2b_problem *p, double *A, double diag, double *y) {
    if (!p->cmask || !p->n_cam) return C2B_OK;
    if (A) hipLaunchKernelGGL(k_const_blocks, dim3(blocks_for(9 * p->n_cam, kSchurBlock)), dim3(kSchurBlock), 0, p->stream, 9 * p->n_cam,
                              (const uint16_t *)p->cmask, diag, A);
    if (y) hipLaunchKernelGGL(k_const_cameras, dim3(blocks_for(p->n_cam, kSchurBlock)), dim3(kSchurBlock), 0, p->stream, p->n_cam,
                              (const uint16_t *)p->cmask, y);
    LAUNCH_CHECK();
    return C2B_OK;
}

// ... V [n_pts][3][3] = diag I3 with gp [n_pts][3] = 0 (gp may be NULL), or t [n_pts][3] = 0 alone (V NULL), of the constant points
static int constant_points(c2b_problem *p, double *V, double diag, double *t) {
    if (!p->pmask || !p->n_pts) return C2B_OK;
    if (V) hipLaunchKernelGGL(k_const_point_blocks, dim3(blocks_for(p->n_pts, kSchurBlock)), dim3(kSchurBlock), 0, p->stream, p->n_pts,
                              (const uint8_t *)p->pmask, diag, V, t);
    else hipLaunchKernelGGL(k_const_points, dim3(blocks_for(p->n_pts, kSchurBlock)), dim3(kSchurBlock), 0, p->stream, p->n_pts,
                            (const uint8_t *)p->pmask, t);
    LAUNCH_CHECK();
    return C2B_OK;
}

// ---- priors on camera centres, intrinsics and points ------------------------------------------------------
// one (target, weights) pair of n rows of 3, checked and copied to the host vectors; `rows` = rows with a weight > 0
static int prior_pair(const char *what, int64_t n, const double *target, const double *w, std::vector<double> &ht, std::vector<double> &hw,
                      int64_t &rows) {
    rows = 0;
    if (!target != !w) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_priors: %s targets and weights go in pairs (both or neither)", what);
    if (!w) return C2B_OK;
    for (int64_t i = 0; i < n; ++i) {
        bool on = false;
        for (int k = 0; k < 3; ++k) {
            const double wk = w[3 * i + k];
            if (!std::isfinite(wk) || wk < 0.0)
                return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_priors: %s weight [%lld][%d] is negative or not finite", what, (long long)i, k);
            if (wk > 0.0 && !std::isfinite(target[3 * i + k]))
                return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_priors: %s target [%lld][%d] is not finite under a positive weight", what,
                            (long long)i, k);
            on = on || wk > 0.0;
        }
        rows += on;
    }
    if (rows) {                                              // all-zero weights are no prior, as an all-zero mask is no mask
        ht.assign(target, target + 3 * n);
        hw.assign(w, w + 3 * n);
    }
    return C2B_OK;
}

// prior_part, carved: two partial arrays [n_pp], n_pp = the camera pass's workgroups + the point pass's (the model pass has
// fewer), then four scalars: the cameras' cost, the points' cost, the model pass's sum of squares and decrease
struct PriorBufs {
    double *pa, *pb, *sc;
};
enum { kPrCostCam = 0, kPrCostPts = 1, kPrSumSq = 2, kPrModel = 3, kPrSlots = 4 };
static int64_t prior_parts(int64_t n_cam, int64_t n_pts) { return (int64_t)prior_cameras_grid(n_cam) + prior_points_grid(n_pts); }
static PriorBufs prior_bufs(c2b_problem *p) {
    const int64_t n_pp = prior_parts(p->n_cam, p->n_pts);
    return PriorBufs{p->prior_part, p->prior_part + n_pp, p->prior_part + 2 * n_pp};
}

int c2b_problem_set_priors(c2b_problem *p, const double *cam_center, const double *cam_center_w, const double *cam_intr, const double *cam_intr_w,
                           const double *pt, const double *pt_w) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_set_priors");
    if (p->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_priors: a shard takes no priors (it cannot be solved alone)");
    const int64_t nc = p->n_cam, np = p->n_pts;
    std::vector<double> h[6];
    int64_t rows[3];
    int rc = prior_pair("camera centre", nc, cam_center, cam_center_w, h[0], h[1], rows[0]);
    if (!rc) rc = prior_pair("intrinsics", nc, cam_intr, cam_intr_w, h[2], h[3], rows[1]);
    if (!rc) rc = prior_pair("point", np, pt, pt_w, h[4], h[5], rows[2]);
    if (rc) return rc;
    // the new device arrays first: a failure leaves the priors in force as they were
    DevBuf<double> d[6], part;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 6 && e == hipSuccess; ++k) {
        if (h[k].empty()) continue;
        e = d[k].alloc(h[k].size());
        if (e == hipSuccess) e = hipMemcpyAsync(d[k], h[k].data(), sizeof(double) * h[k].size(), hipMemcpyHostToDevice, p->stream);
    }
    const bool any = rows[0] || rows[1] || rows[2];
    if (e == hipSuccess && any) e = part.alloc((size_t)(2 * prior_parts(nc, np) + kPrSlots));
    const hipError_t es = hipStreamSynchronize(p->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(hip_code(e), "problem_set_priors: %s", hipGetErrorString(e));
    drop_priors(p);
    if (!any) return C2B_OK;
    p->pc0 = std::move(d[0]); p->pcw = std::move(d[1]); p->pi0 = std::move(d[2]); p->piw = std::move(d[3]);
    p->px0 = std::move(d[4]); p->pxw = std::move(d[5]); p->prior_part = std::move(part);
    p->h_pc0.swap(h[0]); p->h_pcw.swap(h[1]); p->h_pi0.swap(h[2]); p->h_piw.swap(h[3]); p->h_px0.swap(h[4]); p->h_pxw.swap(h[5]);
    p->prior_n_cam = nc; p->prior_n_pts = np;
    for (int k = 0; k < 3; ++k) p->prior_rows[k] = rows[k];
    return C2B_OK;
    C2B_API_END("problem_set_priors")
}

int c2b_problem_get_priors(const c2b_problem *p, double *cam_center, double *cam_center_w, double *cam_intr, double *cam_intr_w, double *pt,
                           double *pt_w, int64_t *n_center_rows, int64_t *n_intr_rows, int64_t *n_pt_rows) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_priors: problem is NULL");
    if (!p->ws) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_priors: nothing uploaded");
    auto give = [](const std::vector<double> &h, int64_t n, double *out) {
        if (!out) return;
        if (!h.empty()) std::copy(h.begin(), h.end(), out);
        else std::fill(out, out + 3 * n, 0.0);
    };
    give(p->h_pc0, p->n_cam, cam_center); give(p->h_pcw, p->n_cam, cam_center_w);
    give(p->h_pi0, p->n_cam, cam_intr); give(p->h_piw, p->n_cam, cam_intr_w);
    give(p->h_px0, p->n_pts, pt); give(p->h_pxw, p->n_pts, pt_w);
    if (n_center_rows) *n_center_rows = p->prior_rows[0];
    if (n_intr_rows) *n_intr_rows = p->prior_rows[1];
    if (n_pt_rows) *n_pt_rows = p->prior_rows[2];
    return C2B_OK;
    C2B_API_END("problem_get_priors")
}

// What follows a kind's observation pass, in the one order the stacked system is assembled in, written here and
// nowhere else: the kind's priors, then the zeros of its constant entries with `diag` on the blocks' diagonal.  Asynchronous; nothing
// is launched for a kind without priors or with nothing constant.  The cameras: A^T A into A9 [n_cam][9][9] = U or M and A^T r
// into gc (gc, or both, may be NULL); with want_cost the priors' cost into the kPrCostCam scalar ...
static int stack_cameras(c2b_problem *p, double *A9, double *gc, double diag, bool want_cost) {
    if ((p->pcw || p->piw) && p->n_cam && (A9 || want_cost)) {
        const PriorBufs P = prior_bufs(p);
        const int rc = c2b_prior_cameras_rows(p->camblk, p->n_cam, p->pc0, p->pcw, p->pi0, p->piw, A9, gc, nullptr, nullptr,
                                               want_cost ? P.pa : nullptr, want_cost ? P.sc + kPrCostCam : nullptr, p->stream);
        if (rc) return rc;
    }
    return A9 && (p->n_obs || has_priors(p)) ? constant_cameras(p, A9, diag, gc) : C2B_OK;
}

// ... the points: diag(w^2) into V and w o r into gp (both may be NULL), the cost into the kPrCostPts scalar
static int stack_points(c2b_problem *p, double *V, double *gp, double diag, bool want_cost) {
    if (p->pxw && p->n_pts && (V || want_cost)) {
        const PriorBufs P = prior_bufs(p);
        const int rc = c2b_prior_points_rows(p->pts4, p->n_pts, p->px0, p->pxw, V, gp, nullptr, want_cost ? P.pb : nullptr,
                                              want_cost ? P.sc + kPrCostPts : nullptr, p->stream);
        if (rc) return rc;
    }
    return V && (p->n_obs || has_priors(p)) ? constant_points(p, V, diag, gp) : C2B_OK;
}

// the two costs queued to host[2] (asynchronous: valid after the stream is synchronised); the priors' cost is their sum
static int prior_cost_queue(c2b_problem *p, double host[2]) {
    host[0] = host[1] = 0.0;
    const PriorBufs P = prior_bufs(p);
    if ((p->pcw || p->piw) && p->n_cam)
        HIP_TRY(hipMemcpyAsync(host, P.sc + kPrCostCam, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (p->pxw && p->n_pts) HIP_TRY(hipMemcpyAsync(host + 1, P.sc + kPrCostPts, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    return C2B_OK;
}

int c2b_problem_prior_cost(c2b_problem *p, double *cost) {
    C2B_API_BEGIN
    if (!p || !cost) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_prior_cost: NULL argument");
    NEED_UPLOADED(p, "problem_prior_cost");
    *cost = 0.0;
    if (!has_priors(p)) return C2B_OK;
    double h[2];
    int rc = ensure_camblk(p);
    if (!rc) rc = stack_cameras(p, nullptr, nullptr, 0.0, true);
    if (!rc) rc = stack_points(p, nullptr, nullptr, 0.0, true);
    if (!rc) rc = prior_cost_queue(p, h);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    *cost = h[0] + h[1];
    return C2B_OK;
    C2B_API_END("problem_prior_cost")
}

int c2b_problem_prior_residual_jacobian(c2b_problem *p, double *r_cam, double *A_cam, double *r_pt) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_prior_residual_jacobian");
    const int64_t nc = p->n_cam, np = p->n_pts;
    const bool cams = (p->pcw || p->piw) && nc && (r_cam || A_cam), pts = p->pxw && np && r_pt;
    if (!cams) {
        if (r_cam) std::fill(r_cam, r_cam + 6 * nc, 0.0);
        if (A_cam) std::fill(A_cam, A_cam + 18 * nc, 0.0);
    }
    if (!pts && r_pt) std::fill(r_pt, r_pt + 3 * np, 0.0);
    if (!cams && !pts) return C2B_OK;
    DevBuf<double> d_r, d_A, d_rp;
    hipStream_t st = p->stream;
    int rc = ensure_camblk(p);
    if (rc) return rc;
    if (cams) {
        HIP_TRY(d_r.alloc(6 * (size_t)nc));
        HIP_TRY(d_A.alloc(18 * (size_t)nc));
        rc = c2b_prior_cameras_rows(p->camblk, nc, p->pc0, p->pcw, p->pi0, p->piw, nullptr, nullptr, d_r, d_A, nullptr, nullptr, st);
        if (!rc && r_cam) HIP_TRY(hipMemcpyAsync(r_cam, d_r, sizeof(double) * 6 * (size_t)nc, hipMemcpyDeviceToHost, st));
        if (!rc && A_cam) HIP_TRY(hipMemcpyAsync(A_cam, d_A, sizeof(double) * 18 * (size_t)nc, hipMemcpyDeviceToHost, st));
    }
    if (!rc && pts) {
        HIP_TRY(d_rp.alloc(3 * (size_t)np));
        rc = c2b_prior_points_rows(p->pts4, np, p->px0, p->pxw, nullptr, nullptr, d_rp, nullptr, nullptr, st);
        if (!rc) HIP_TRY(hipMemcpyAsync(r_pt, d_rp, sizeof(double) * 3 * (size_t)np, hipMemcpyDeviceToHost, st));
    }
    const hipError_t es = hipStreamSynchronize(st);                  // (the temporaries are freed on return)
    if (rc) return rc;
    if (es != hipSuccess) return fail(C2B_ERR_HIP, "problem_prior_residual_jacobian: %s", hipGetErrorString(es));
    return C2B_OK;
    C2B_API_END("problem_prior_residual_jacobian")
}

// ---- robust loss -----------------------------------------------------------------------------------------
int c2b_problem_set_loss(c2b_problem *p, int kind, double scale) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_loss: problem is NULL");
    NEED_LOSS(kind, scale, "problem_set_loss");
    p->loss_kind = kind;
    p->loss_scale = kind == kLossSquared ? 1.0 : scale;
    return C2B_OK;
    C2B_API_END("problem_set_loss")
}

int c2b_problem_get_loss(const c2b_problem *p, int *kind, double *scale) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_loss: problem is NULL");
    if (kind) *kind = p->loss_kind;
    if (scale) *scale = p->loss_scale;
    return C2B_OK;
    C2B_API_END("problem_get_loss")
}

// ---- preconditioner of the step ----------------------------------------------------------------------------
int c2b_problem_set_preconditioner(c2b_problem *p, int kind) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_preconditioner: problem is NULL");
    if (kind != C2B_PRECOND_BLOCK_JACOBI && kind != C2B_PRECOND_SCHUR_JACOBI)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_preconditioner: kind must be 0 (block-Jacobi) or 1 (Schur-Jacobi), not %d", kind);
    p->precond_kind = kind;
    return C2B_OK;
    C2B_API_END("problem_set_preconditioner")
}

int c2b_problem_get_preconditioner(const c2b_problem *p, int *kind) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_preconditioner: problem is NULL");
    if (kind) *kind = p->precond_kind;
    return C2B_OK;
    C2B_API_END("problem_get_preconditioner")
}

int c2b_problem_preconditioner_fallbacks(const c2b_problem *p, int64_t *n) {
    C2B_API_BEGIN
    if (!p || !n) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_preconditioner_fallbacks: NULL argument");
    *n = p->precond_fallbacks;
    return C2B_OK;
    C2B_API_END("problem_preconditioner_fallbacks")
}

// ---- how the step applies S ---------------------------------------------------------------------------------
int c2b_problem_set_schur(c2b_problem *p, int kind) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_schur: problem is NULL");
    if (kind != C2B_SCHUR_IMPLICIT && kind != C2B_SCHUR_EXPLICIT)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_schur: kind must be 0 (implicit) or 1 (explicit), not %d", kind);
    p->schur_kind = kind;
    return C2B_OK;
    C2B_API_END("problem_set_schur")
}

int c2b_problem_get_schur(const c2b_problem *p, int *kind) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_schur: problem is NULL");
    if (kind) *kind = p->schur_kind;
    return C2B_OK;
    C2B_API_END("problem_get_schur")
}

// ---- how the step solves S dc = b -----------------------------------------------------------------------------
int c2b_problem_set_linear_solver(c2b_problem *p, int kind) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_linear_solver: problem is NULL");
    if (kind != C2B_LINEAR_PCG && kind != C2B_LINEAR_CHOLESKY)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_linear_solver: kind must be 0 (pcg) or 1 (cholesky), not %d", kind);
    p->linear_kind = kind;
    return C2B_OK;
    C2B_API_END("problem_set_linear_solver")
}

int c2b_problem_get_linear_solver(const c2b_problem *p, int *kind) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_linear_solver: problem is NULL");
    if (kind) *kind = p->linear_kind;
    return C2B_OK;
    C2B_API_END("problem_get_linear_solver")
}

// sum over the observations of rho(s) (weighted_sq: of w s) under the problem's loss into out[0] (device), asynchronous;
// one partial per workgroup of 256 observations: the workspace holds one per 4 tiles of 64 (block_part_slots)
static int robust_sum(c2b_problem *p, bool weighted_sq, double *out) {
    const int rc = ensure_camblk(p);
    if (rc) return rc;
    launch_robust_cost(p->stream, weighted_sq, p->camblk, p->pts4, p->cam_idx, nullptr, 0, p->pt_idx, p->uv, p->n_obs, p->loss_kind,
                       p->loss_scale, reinterpret_cast<double *>(p->ws.ptr) + kWsBlockPart, out);
    HIP_TRY(launch_error());
    return C2B_OK;
}

int c2b_problem_robust_cost(c2b_problem *p, double *cost) {
    C2B_API_BEGIN
    if (!p || !cost) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_robust_cost: NULL argument");
    NEED_UPLOADED(p, "problem_robust_cost");
    double s = 0.0;
    if (p->n_obs) {
        int rc = robust_sum(p, false, p->scalar);
        if (!rc) rc = scalars_to_host(p->stream, p->scalar, 1, &s);
        if (rc) return rc;
    }
    *cost = s;
    return C2B_OK;
    C2B_API_END("problem_robust_cost")
}

// ---- the stacked system: a kind's observation pass (zeros without a list), then stack_cameras / stack_points ----
// The camera side: U and gc (both NULL: the cost alone).  want_cost: the observations' sum of squares (weighted under a
// loss) into p->scalar and the camera priors' cost into its scalar (prior_cost_queue).  After ensure_camblk and ensure_rows.
static int assemble_cameras(c2b_problem *p, double *U, double *gc, double diag, bool want_cost) {
    hipStream_t st = S(p->stream);
    if (!U && !want_cost) return C2B_OK;
    if (!p->n_obs) {                                         // no list: every camera's block is empty
        if (U && p->n_cam) {
            HIP_TRY(hipMemsetAsync(U, 0, sizeof(double) * 81 * (size_t)p->n_cam, st));
            HIP_TRY(hipMemsetAsync(gc, 0, sizeof(double) * 9 * (size_t)p->n_cam, st));
        }
        if (want_cost) HIP_TRY(hipMemsetAsync(p->scalar, 0, sizeof(double), st));
    } else if (U) {
        launch_normal_cameras(st, p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->pt_idx, p->uv, p->n_obs, U, gc, p->ws,
                              want_cost ? p->scalar.ptr : nullptr, p->loss_kind, p->loss_scale);
        LAUNCH_CHECK();
    } else {                                                 // the (weighted) sum of squares without the blocks
        const int rc = p->loss_kind != kLossSquared
                           ? robust_sum(p, true, p->scalar)
                           : c2b_reprojection_error_sum_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv,
                                                             p->n_obs, 2.0, p->ws, p->scalar, st);
        if (rc) return rc;
    }
    return stack_cameras(p, U, gc, diag, want_cost);
}

// The point side: V and gp (both NULL: the cost alone, of the point priors)
static int assemble_points(c2b_problem *p, double *V, double *gp, double diag, bool want_cost) {
    hipStream_t st = S(p->stream);
    if (!p->n_pts || (!V && !want_cost)) return C2B_OK;
    if (V && p->n_obs) {
        if (const int rc = ensure_transpose(p)) return rc;
        launch_normal_points(st, p->camblk, p->pts4, p->n_pts, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, V, gp, p->loss_kind, p->loss_scale);
        LAUNCH_CHECK();
    } else if (V) {
        HIP_TRY(hipMemsetAsync(V, 0, sizeof(double) * 9 * (size_t)p->n_pts, st));
        HIP_TRY(hipMemsetAsync(gp, 0, sizeof(double) * 3 * (size_t)p->n_pts, st));
    }
    return stack_points(p, V, gp, diag, want_cost);
}

int c2b_problem_normal_equations(c2b_problem *p, double *U, double *gc, double *V, double *gp, double *sum_sq) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_normal_equations: problem is NULL");
    if (!U != !gc || !V != !gp) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_normal_equations: U / gc and V / gp go in pairs (both or neither)");
    for (const void *q : {(const void *)U, (const void *)gc, (const void *)V, (const void *)gp, (const void *)sum_sq})
        if (reinterpret_cast<uintptr_t>(q) & 7) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_normal_equations: misaligned pointer");
    NEED_UPLOADED(p, "problem_normal_equations");
    const bool want_sum = sum_sq != nullptr, pri = has_priors(p);
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (!rc) rc = assemble_cameras(p, U, gc, 0.0, want_sum);
    if (!rc) rc = assemble_points(p, V, gp, 0.0, want_sum);
    double s = 0.0, hp[2] = {0.0, 0.0};                      // the priors' cost joins sum_sq
    if (!rc && pri && want_sum) rc = prior_cost_queue(p, hp);
    if (!rc) rc = scalars_to_host(p->stream, p->scalar, want_sum ? 1 : 0, &s);
    if (rc) return rc;
    if (want_sum) *sum_sq = pri ? s + (hp[0] + hp[1]) : s;
    return C2B_OK;
    C2B_API_END("problem_normal_equations")
}

// ---- damped Gauss-Newton step (schur_kernels.hpp) ------------------------------------------------------------------
// c2b_problem::sv, carved: U [n_cam][81], gc [n_cam][9], V [n_pts][9], gp [n_pts][3], Lf [n_cam][45], t [n_pts][3],
// r / z / p / q [n_cam][9], two partial arrays [n_part], the device scalars [kScSlots]; under the Schur-Jacobi
// preconditioner its blocks M [n_cam][81] after them (the rest lies where it lies without); under the explicit Schur
// complement its blocks Sd [n_cam][81], So [sp_edges][81] and Y [n_obs][27] after those, and the partial arrays
// also cover k_schur_spmv's grid; under the direct solve those whatever `schur` says, and after Y the dense image
// A [Np][Np] and two vectors [Np], Np = 64 ceil(9 n_cam / 64).  With none of the options nothing moves.
struct SolveBufs {
    double *U, *gc, *V, *gp, *Lf, *t, *r, *z, *pv, *q, *pa, *pb, *sc, *M, *Sd, *So, *Y, *A, *dx, *dw;
    int64_t n_part;
};

static bool schur_explicit(const c2b_problem *p) { return p->schur_kind == C2B_SCHUR_EXPLICIT; }
static bool linear_cholesky(const c2b_problem *p) { return p->linear_kind == C2B_LINEAR_CHOLESKY; }
// the solve buffers hold S's blocks and Y
static bool explicit_bufs(const c2b_problem *p) { return schur_explicit(p) || linear_cholesky(p); }
// the doubles the direct solve adds behind them: the dense image and its two vectors
static int64_t dense_doubles(const c2b_problem *p) {
    const int64_t np = dense_padded(9 * p->n_cam);
    return np * np + 2 * np;
}

static int64_t solve_parts(const c2b_problem *p) {
    const int64_t a = (int64_t)schur_cameras_grid(p->n_cam) * (kNormBlock / 64);
    const int64_t e = explicit_bufs(p) ? schur_spmv_parts(p->n_cam) : 0;
    return std::max<int64_t>({a, e, (int64_t)blocks_for(p->n_cam, kSchurBlock), (int64_t)blocks_for(p->n_obs, kSchurBlock), 1});
}

// the doubles the explicit Schur complement adds: its blocks and Y (the pattern is built before this is asked)
static int64_t schur_explicit_doubles(const c2b_problem *p) { return 81 * (p->n_cam + p->sp_edges) + 27 * p->n_obs; }

static int64_t solve_doubles(const c2b_problem *p) {
    return p->n_cam * (81 + 9 + kCholPacked + 4 * 9) + p->n_pts * (9 + 3 + 3) + 2 * solve_parts(p) + kScSlots +
           (p->precond_kind == C2B_PRECOND_SCHUR_JACOBI ? 81 * p->n_cam : 0) + (explicit_bufs(p) ? schur_explicit_doubles(p) : 0) +
           (linear_cholesky(p) ? dense_doubles(p) : 0);
}

static SolveBufs solve_bufs(c2b_problem *p) {
    SolveBufs b;
    const int64_t nc = p->n_cam, np = p->n_pts;
    double *q = p->sv;
    auto take = [&](int64_t n) { double *r = q; q += n; return r; };
    b.U = take(81 * nc); b.gc = take(9 * nc); b.V = take(9 * np); b.gp = take(3 * np); b.Lf = take(kCholPacked * nc);
    b.t = take(3 * np); b.r = take(9 * nc); b.z = take(9 * nc); b.pv = take(9 * nc); b.q = take(9 * nc);
    b.n_part = solve_parts(p);
    b.pa = take(b.n_part); b.pb = take(b.n_part); b.sc = take(kScSlots);
    b.M = p->precond_kind == C2B_PRECOND_SCHUR_JACOBI ? take(81 * nc) : nullptr;
    const bool ex = explicit_bufs(p), dn = linear_cholesky(p);
    const int64_t dnp = dense_padded(9 * nc);
    b.Sd = ex ? take(81 * nc) : nullptr;
    b.So = ex ? take(81 * p->sp_edges) : nullptr;
    b.Y = ex ? take(27 * p->n_obs) : nullptr;
    b.A = dn ? take(dnp * dnp) : nullptr;
    b.dx = dn ? take(dnp) : nullptr;
    b.dw = dn ? take(dnp) : nullptr;
    return b;
}

static int ensure_solver(c2b_problem *p) {
    const int64_t n = solve_doubles(p);
    if (p->sv && p->sv_doubles >= n) return C2B_OK;
    p->sv_doubles = 0;
    const hipError_t e = p->sv.alloc((size_t)n);                  // (the smaller one is freed first)
    if (e != hipSuccess && linear_cholesky(p))                   // no fallback: the caller sets C2B_LINEAR_PCG, the handle is usable
        return fail(hip_code(e), "problem_solve_step: allocation of %lld bytes for the direct solve (%lld of them the explicit blocks, Y and the dense image): %s",
                    (long long)(8 * n), (long long)(8 * (schur_explicit_doubles(p) + dense_doubles(p))), hipGetErrorString(e));
    if (e != hipSuccess && schur_explicit(p))                    // no fallback: the caller sets C2B_SCHUR_IMPLICIT, the handle is usable
        return fail(hip_code(e), "problem_solve_step: allocation of %lld bytes for the explicit Schur complement (%lld of them its blocks and Y): %s",
                    (long long)(8 * n), (long long)(8 * schur_explicit_doubles(p)), hipGetErrorString(e));
    if (e != hipSuccess) return fail(hip_code(e), "problem_solve_step: allocation: %s", hipGetErrorString(e));
    p->sv_doubles = n;
    return C2B_OK;
}

// The covisibility graph of the resident list at min_shared into the caller's buffers (degree pass, its total, fill pass):
// counts[0] = the directed edges, counts[1] = the cameras that took the heavy path.  Synchronous.
static int covisibility_build(c2b_problem *p, int min_shared, DevBuf<uint64_t> &ptr, DevBuf<uint32_t> &nbr, DevBuf<uint32_t> &shared, int64_t counts_out[2]) {
    const int64_t n_cam = p->n_cam;
    hipStream_t st = p->stream;
    DevBuf<char> temp;
    DevBuf<int64_t> counts;
    counts_out[0] = counts_out[1] = 0;
    struct SyncOnExit { hipStream_t s; ~SyncOnExit() { (void)hipStreamSynchronize(s); } } sync_on_exit{st};      // before the locals are freed
    HIP_TRY(ptr.alloc((size_t)n_cam + 1));
    HIP_TRY(counts.alloc(2));
    HIP_TRY(temp.alloc((size_t)c2b_covisibility_temp_bytes(n_cam, C2B_COVIS_TEMP_GRAPH)));
    int rc = ensure_rows(p);
    if (!rc && p->n_obs) rc = ensure_transpose(p);
    if (!rc) rc = c2b_covisibility_degree_rows(p->rows_ptr, p->pt_idx, p->nt_ptr, p->nt_obs, p->nt_cam, n_cam, p->n_pts, p->n_obs, min_shared, temp, ptr,
                                               counts, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(counts_out, counts.ptr, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(nbr.alloc((size_t)counts_out[0]));
    HIP_TRY(shared.alloc((size_t)counts_out[0]));
    rc = c2b_covisibility_fill_rows(p->rows_ptr, p->pt_idx, p->nt_ptr, p->nt_obs, p->nt_cam, n_cam, p->n_pts, p->n_obs, min_shared, temp, ptr, nbr, shared, st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return C2B_OK;
}

// The pattern of the explicit S: the graph at threshold 1, the solver's own.  Copied from the cached graph when
// that is at threshold 1, built by the same passes otherwise; kept until the list changes (drop_rows).
static int ensure_schur_pattern(c2b_problem *p) {
    if (p->sp_ptr) return C2B_OK;
    DevBuf<uint64_t> ptr;
    DevBuf<uint32_t> nbr, shared;
    int64_t h[2] = {0, 0};
    if (p->cv_ptr && p->cv_min_shared == 1) {
        h[0] = p->cv_edges;
        HIP_TRY(ptr.alloc((size_t)p->n_cam + 1));
        HIP_TRY(nbr.alloc((size_t)h[0]));
        HIP_TRY(hipMemcpyAsync(ptr, p->cv_ptr, sizeof(uint64_t) * ((size_t)p->n_cam + 1), hipMemcpyDeviceToDevice, p->stream));
        if (h[0]) HIP_TRY(hipMemcpyAsync(nbr, p->cv_nbr, sizeof(uint32_t) * (size_t)h[0], hipMemcpyDeviceToDevice, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    } else if (const int rc = covisibility_build(p, 1, ptr, nbr, shared, h)) {
        return rc;
    }
    p->sp_ptr = std::move(ptr); p->sp_nbr = std::move(nbr);
    p->sp_edges = h[0];
    return C2B_OK;
}

// ---- the phases of c2b_problem_solve_step, in the order it runs them (the set-up is the stacked system above) -----------
// The Schur operator's application, written once: the point pass t = +-V_l^-1 (hp + W^T x) with t = 0 for the constant
// points, then -- y given -- the camera pass over t in the mode its pointers name (launch_schur_cameras) and y's constant
// entries to 0.  Asynchronous; the right-hand side, the iteration and the back-substitution are calls of it.
static int schur_apply(c2b_problem *p, const SolveBufs &B, double lambda, const double *x, const double *hp, double *t, bool neg,
                       const double *hc, double *y, double *part) {
    launch_schur_points(p->stream, p->camblk, p->pts4, p->n_pts, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, B.V, lambda, x, hp, t, neg,
                        p->loss_kind, p->loss_scale);
    const int rc = constant_points(p, nullptr, 0.0, t);
    if (rc || !y) return rc;
    launch_schur_cameras(p->stream, p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->pt_idx, p->uv, B.U, lambda, x, hc, t, y, part,
                         p->loss_kind, p->loss_scale);
    return constant_cameras(p, nullptr, 0.0, y);
}

// The preconditioner's factors Lf: of U_l's blocks, or (B.M) of the Schur-Jacobi blocks M with the fallbacks' count queued.
// k_schur_jacobi sums M from the observations, not from U, so the camera priors and the constant zeros follow it as they
// follow the camera pass (stack_cameras).  It sees the constant points' V as kConstPointV, under which their observations
// add Jc^T Jc as they do with Jp = 0; from here on that V is 0.
static int step_preconditioner(c2b_problem *p, const SolveBufs &B, double lambda) {
    hipStream_t st = p->stream;
    const int64_t nc = p->n_cam;
    const unsigned nbc = blocks_for(nc, kSchurBlock);
    if (!B.M) {
        hipLaunchKernelGGL(k_schur_factor, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.U, lambda, B.Lf);
        return C2B_OK;
    }
    launch_schur_jacobi(st, p->camblk, p->pts4, p->rows_ptr, nc, p->pt_idx, p->uv, B.U, B.V, lambda, B.M, p->loss_kind, p->loss_scale);
    int rc = stack_cameras(p, B.M, nullptr, lambda * 1e-6, false);
    if (!rc) rc = constant_points(p, B.V, 0.0, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_schur_factor_blocks, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.M, (const double *)B.U, lambda,
                       B.Lf, B.pa);
    fold_sum(st, B.pa, (int)nbc, B.sc + kScFallback);
    return C2B_OK;
}

// The set-up under the explicit Schur complement, in place of step_preconditioner: S into B.Sd / B.So on the
// handle's pattern, then -- want_factors -- the same preconditioner's factors.  V comes in as step_preconditioner's Schur-Jacobi
// branch takes it (the constant points' at kConstPointV: their Y is 0) and leaves as it leaves there.
//   Sd = M of k_schur_jacobi (it does not cancel at small lambda), the priors and the constant zeros as they follow M; M is a
//   copy of it at that point, its definition unchanged; then k_schur_blocks adds the cross terms of duplicated pairs, which
//   are S's and not M's, and the constant zeros follow once more, now also on the off-diagonal blocks.
static int schur_explicit_setup(c2b_problem *p, const SolveBufs &B, double lambda, bool want_factors) {
    hipStream_t st = p->stream;
    const int64_t nc = p->n_cam;
    const unsigned nbc = blocks_for(nc, kSchurBlock);
    launch_schur_jacobi(st, p->camblk, p->pts4, p->rows_ptr, nc, p->pt_idx, p->uv, B.U, B.V, lambda, B.Sd, p->loss_kind, p->loss_scale);
    int rc = stack_cameras(p, B.Sd, nullptr, lambda * 1e-6, false);
    if (rc) return rc;
    if (B.M && want_factors) HIP_TRY(hipMemcpyAsync(B.M, B.Sd, sizeof(double) * 81 * (size_t)nc, hipMemcpyDeviceToDevice, st));
    launch_schur_y(st, p->camblk, p->pts4, p->cam_idx, p->pt_idx, p->uv, p->n_obs, B.V, lambda, B.Y, p->loss_kind, p->loss_scale);
    if ((rc = constant_points(p, B.V, 0.0, nullptr))) return rc;
    launch_schur_blocks(st, p->rows_ptr, p->pt_idx, p->nt_ptr, p->nt_obs, p->nt_cam, nc, p->sp_ptr, p->sp_nbr, B.Y, B.Sd, B.So);
    if (p->cmask) {
        if ((rc = constant_cameras(p, B.Sd, lambda * 1e-6, nullptr))) return rc;
        hipLaunchKernelGGL(k_const_offdiag, dim3(blocks_for(nc, 4)), dim3(256), 0, st, (const uint64_t *)p->sp_ptr, (const uint32_t *)p->sp_nbr, nc,
                           (const uint16_t *)p->cmask, B.So);
    }
    LAUNCH_CHECK();
    if (!want_factors) return C2B_OK;
    if (!B.M) {
        hipLaunchKernelGGL(k_schur_factor, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.U, lambda, B.Lf);
        return C2B_OK;
    }
    hipLaunchKernelGGL(k_schur_factor_blocks, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.M, (const double *)B.U, lambda,
                       B.Lf, B.pa);
    fold_sum(st, B.pa, (int)nbc, B.sc + kScFallback);
    return C2B_OK;
}

// PCG on the reduced system from x = 0 (x is dc), its right-hand side b in B.r: the iterations run, the status (0 converged,
// 1 max_iters reached, 2 a breakdown or a non-finite number), |b|^2 and the last |r|.  One read-back per iteration.
struct PcgResult {
    int iterations, status;
    double bb, rnorm;
};
static int schur_pcg(c2b_problem *p, const SolveBufs &B, double lambda, int max_iters, double rel_tol, double *dc, PcgResult *res) {
    hipStream_t st = p->stream;
    const int64_t nc = p->n_cam;
    const unsigned nbc = blocks_for(nc, kSchurBlock);
    double h[kScSlots];                                      // what each read-back brings: the scalars up to kScRz1, after all queued work
    int rc;
    hipLaunchKernelGGL(k_pcg_update<true>, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.Lf, (const double *)B.sc, 0, dc,
                       B.r, B.pv, (const double *)nullptr, B.z, B.pa, B.pb);
    fold_sum(st, B.pa, (int)nbc, B.sc + kScRr);
    fold_sum(st, B.pb, (int)nbc, B.sc + kScRz0);
    HIP_TRY(launch_error());
    if ((rc = scalars_to_host(st, B.sc, kScRz1 + 1, h))) return rc;
    const double bb = h[kScRr], bnorm = std::sqrt(bb);
    double rnorm = bnorm;
    int it = 0, status = 1;
    if (!std::isfinite(bb) || !std::isfinite(h[kScRz0])) {
        status = 2;
    } else if (rnorm <= rel_tol * bnorm) {                   // b = 0 (or rel_tol >= 1)
        status = 0;
    } else {
        while (it < max_iters) {
            const int cur = (it & 1) ? kScRz1 : kScRz0, nxt = (it & 1) ? kScRz0 : kScRz1;
            // q = S p and the p.q partials (p's constant entries are 0: they need no correction)
            // (explicit: one product with the stored blocks, whose constant rows are 0 already)
            if (B.So) {
                launch_schur_spmv(st, p->sp_ptr, p->sp_nbr, nc, B.Sd, B.So, B.pv, B.q, B.pa);
                fold_sum(st, B.pa, (int)schur_spmv_parts(nc), B.sc + kScPq);
            } else {
                if ((rc = schur_apply(p, B, lambda, B.pv, nullptr, B.t, false, nullptr, B.q, B.pa))) return rc;
                fold_sum(st, B.pa, (int)(schur_cameras_grid(nc) * (kNormBlock / 64)), B.sc + kScPq);
            }
            hipLaunchKernelGGL(k_pcg_update<false>, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.Lf, (const double *)B.sc,
                               cur, dc, B.r, B.pv, (const double *)B.q, B.z, B.pa, B.pb);
            fold_sum(st, B.pa, (int)nbc, B.sc + kScRr);
            fold_sum(st, B.pb, (int)nbc, B.sc + nxt);
            HIP_TRY(launch_error());
            if ((rc = scalars_to_host(st, B.sc, kScRz1 + 1, h))) return rc;
            const double pq = h[kScPq], rz = h[cur], alpha = rz / pq;
            if (!(pq > 0.0) || !std::isfinite(alpha)) { status = 2; break; }     // k_pcg_update left x as it was
            ++it;
            const double rr = h[kScRr], rzn = h[nxt];
            if (!std::isfinite(rr) || !std::isfinite(rzn)) { status = 2; break; }
            rnorm = std::sqrt(rr);
            if (rnorm <= rel_tol * bnorm) { status = 0; break; }
            if (it == max_iters) break;
            hipLaunchKernelGGL(k_pcg_direction, dim3(blocks_for(9 * nc, kSchurBlock)), dim3(kSchurBlock), 0, st, 9 * nc, rzn / rz,
                               (const double *)B.z, B.pv);
        }
    }
    *res = PcgResult{it, status, bb, rnorm};
    return C2B_OK;
}

// The direct solve of the reduced system, in place of schur_pcg: S's lower triangle into the dense image, its
// Cholesky factor, the two substitutions on b (in B.r) into dc, then the true residual from one product with the stored blocks.
// res: 0 iterations; status 0, or 2 when a pivot was not finite or not > 0 (dc is then garbage: the caller zeroes the step).
static int dense_solve(c2b_problem *p, const SolveBufs &B, double *dc, PcgResult *res) {
    hipStream_t st = p->stream;
    const int64_t nc = p->n_cam, n = 9 * nc, np = dense_padded(n);
    const unsigned nb = blocks_for(n, kSchurBlock);
    if (!p->dense_info) HIP_TRY(p->dense_info.alloc(1));
    launch_dense_scatter(st, p->sp_ptr, p->sp_nbr, nc, B.Sd, B.So, B.A, np);
    HIP_TRY(hipMemsetAsync(p->dense_info, 0, sizeof(int32_t), st));
    launch_dense_cholesky(st, B.A, np, np, p->dense_info);
    HIP_TRY(hipMemsetAsync(B.dx, 0, sizeof(double) * (size_t)np, st));
    HIP_TRY(hipMemcpyAsync(B.dx, B.r, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    launch_dense_solve(st, B.A, np, np, B.dx);
    HIP_TRY(hipMemcpyAsync(dc, B.dx, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    launch_schur_spmv(st, p->sp_ptr, p->sp_nbr, nc, B.Sd, B.So, dc, B.dw, nullptr);
    hipLaunchKernelGGL(k_dense_residual, dim3(nb), dim3(kSchurBlock), 0, st, n, (const double *)B.r, (const double *)B.dw, B.pa, B.pb);
    fold_sum(st, B.pa, (int)nb, B.sc + kScRz0);
    fold_sum(st, B.pb, (int)nb, B.sc + kScRr);
    HIP_TRY(launch_error());
    int32_t bad = 0;
    double h[kScSlots];
    HIP_TRY(hipMemcpyAsync(&bad, p->dense_info, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (const int rc = scalars_to_host(st, B.sc, kScRz1 + 1, h)) return rc;
    *res = PcgResult{0, bad ? 2 : 0, h[kScRr], std::sqrt(h[kScRz0])};
    return C2B_OK;
}

// dp = -V_l^-1 (gp + W^T dc); then |r|^2 and the model decrease from J, per observation, and the priors' share of the two
// sums beside k_schur_model's; the step's last read-back, which also brings the Schur-Jacobi fallbacks' count
static int step_model(c2b_problem *p, const SolveBufs &B, double lambda, const double *dc, double *dp, double *sum_sq, double *model) {
    hipStream_t st = p->stream;
    const bool pri = has_priors(p);
    int rc = schur_apply(p, B, lambda, dc, B.gp, dp, true, nullptr, nullptr, nullptr);
    if (rc) return rc;
    launch_schur_model(st, p->camblk, p->pts4, p->cam_idx, p->pt_idx, p->uv, p->n_obs, dc, dp, B.pa, B.pb, B.sc + kScSumSq,
                       p->loss_kind, p->loss_scale);
    static_assert(kScModel == kScSumSq + 1, "launch_schur_model folds into two neighbouring scalars");
    double h[kScSlots], hpr[2] = {0.0, 0.0};
    if (pri) {
        const PriorBufs P = prior_bufs(p);
        if ((rc = c2b_prior_model_rows(p->camblk, p->n_cam, p->pc0, p->pcw, p->pi0, p->piw, p->pts4, p->n_pts, p->px0, p->pxw, dc, dp, P.pa,
                                        P.pb, P.sc + kPrSumSq, st)))
            return rc;
        HIP_TRY(hipMemcpyAsync(hpr, P.sc + kPrSumSq, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(launch_error());
    const bool fb = B.M && !linear_cholesky(p);                      // (the direct solve builds no preconditioner)
    if ((rc = scalars_to_host(st, B.sc, fb ? kScFallback + 1 : kScModel + 1, h))) return rc;
    if (fb) p->precond_fallbacks = (int64_t)h[kScFallback];
    *sum_sq = pri ? h[kScSumSq] + hpr[0] : h[kScSumSq];
    *model = pri ? h[kScModel] + hpr[1] : h[kScModel];
    return C2B_OK;
}

int c2b_problem_solve_step(c2b_problem *p, double lambda, int max_iters, double rel_tol, double *dc, double *dp, c2b_step_info *info) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: problem is NULL");
    if (!good_lambda(lambda)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: lambda must lie in [1e-20, 1e32]");
    if (max_iters < 0 || !(rel_tol >= 0.0) || !std::isfinite(rel_tol))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: max_iters must be >= 0 and rel_tol finite and >= 0");
    NEED_UPLOADED(p, "problem_solve_step");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: a shard cannot be solved alone (the point-side sums span every rank)");
    const int64_t nc = p->n_cam, np = p->n_pts, no = p->n_obs;
    if ((nc && !dc) || (np && !dp)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: dc / dp is NULL");
    if (!aligned8(dc) || !aligned8(dp)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: misaligned pointer");
    hipStream_t st = p->stream;
    c2b_step_info out{0, 0, 0.0, 0.0, 0.0};
    p->precond_fallbacks = 0;
    if (!no && has_priors(p)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: priors without a single observation are not solved (DESIGN 4.13)");
    if (!no) {                                               // no observation: g = 0, the step is 0
        if (nc) HIP_TRY(hipMemsetAsync(dc, 0, sizeof(double) * 9 * (size_t)nc, st));
        if (np) HIP_TRY(hipMemsetAsync(dp, 0, sizeof(double) * 3 * (size_t)np, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (info) *info = out;
        return C2B_OK;
    }
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (!rc) rc = ensure_transpose(p);
    const bool dn = linear_cholesky(p), ex = schur_explicit(p) && !dn;
    if (dn && nc > C2B_DENSE_MAX_CAMERAS)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_solve_step: %lld cameras exceed C2B_DENSE_MAX_CAMERAS = %d of the direct solve (set C2B_LINEAR_PCG)",
                    (long long)nc, C2B_DENSE_MAX_CAMERAS);
    if (!rc && (ex || dn)) rc = ensure_schur_pattern(p);
    if (!rc) rc = ensure_solver(p);
    if (rc) return rc;
    const SolveBufs B = solve_bufs(p);
    // U, gc, V, gp of the stacked system: with priors and constant parameters they are those of J~
    // from here on, and so is the damping's diagonal.  The constant points' V: see step_preconditioner
    PcgResult pcg{0, 1, 0.0, 0.0};
    rc = assemble_cameras(p, B.U, B.gc, 0.0, false);
    if (!rc) rc = assemble_points(p, B.V, B.gp, B.M || ex || dn ? kConstPointV : 0.0, false);
    if (!rc) rc = dn ? schur_explicit_setup(p, B, lambda, false) : ex ? schur_explicit_setup(p, B, lambda, true) : step_preconditioner(p, B, lambda);
    if (!rc) rc = schur_apply(p, B, lambda, nullptr, B.gp, B.t, false, B.gc, B.r, nullptr);      // b = -gc + W V_l^-1 gp into r
    if (!rc) rc = dn ? dense_solve(p, B, dc, &pcg) : schur_pcg(p, B, lambda, max_iters, rel_tol, dc, &pcg);
    if (!rc) rc = step_model(p, B, lambda, dc, dp, &out.sum_sq, &out.model_decrease);
    if (rc) return rc;
    out.iterations = pcg.iterations;
    out.status = pcg.status;
    out.rel_residual = pcg.bb == 0.0 ? 0.0 : pcg.rnorm / std::sqrt(pcg.bb);
    if (!std::isfinite(out.sum_sq) || !std::isfinite(out.model_decrease) || !std::isfinite(out.rel_residual) || (dn && pcg.status == 2)) {
        // a factorisation failed (a pivot <= 0 at the damping's low end) and a NaN reached the step: no step at all
        HIP_TRY(hipMemsetAsync(dc, 0, sizeof(double) * 9 * (size_t)nc, st));
        if (np) HIP_TRY(hipMemsetAsync(dp, 0, sizeof(double) * 3 * (size_t)np, st));
        HIP_TRY(hipStreamSynchronize(st));
        out.status = 2;
        out.rel_residual = 1.0;
        out.model_decrease = 0.0;
    }
    if (info) *info = out;
    return C2B_OK;
    C2B_API_END("problem_solve_step")
}

// ---- the reduced camera system as a product ------------------------------------------------------------------
int c2b_problem_schur_bytes(c2b_problem *p, int64_t *bytes) {
    C2B_API_BEGIN
    if (!p || !bytes) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_bytes: NULL argument");
    NEED_UPLOADED(p, "problem_schur_bytes");
    if (p->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_bytes: a shard cannot be solved alone");
    if (const int rc = ensure_schur_pattern(p)) return rc;
    *bytes = 8 * schur_explicit_doubles(p);
    return C2B_OK;
    C2B_API_END("problem_schur_bytes")
}

int c2b_problem_linear_solver_bytes(c2b_problem *p, int64_t *bytes) {
    C2B_API_BEGIN
    if (!p || !bytes) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_linear_solver_bytes: NULL argument");
    NEED_UPLOADED(p, "problem_linear_solver_bytes");
    if (p->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_linear_solver_bytes: a shard cannot be solved alone");
    if (p->n_cam > C2B_DENSE_MAX_CAMERAS)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_linear_solver_bytes: %lld cameras exceed C2B_DENSE_MAX_CAMERAS = %d of the direct solve",
                    (long long)p->n_cam, C2B_DENSE_MAX_CAMERAS);
    if (const int rc = ensure_schur_pattern(p)) return rc;
    *bytes = 8 * (schur_explicit_doubles(p) + dense_doubles(p));
    return C2B_OK;
    C2B_API_END("problem_linear_solver_bytes")
}

int c2b_problem_get_schur_pattern(c2b_problem *p, uint64_t *nbr_ptr, uint32_t *nbr) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_get_schur_pattern");
    if (p->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_schur_pattern: a shard cannot be solved alone");
    if (const int rc = ensure_schur_pattern(p)) return rc;
    const size_t ne = (size_t)p->sp_edges;
    if (nbr_ptr) HIP_TRY(hipMemcpyAsync(nbr_ptr, p->sp_ptr, sizeof(uint64_t) * ((size_t)p->n_cam + 1), hipMemcpyDeviceToHost, p->stream));
    if (nbr && ne) HIP_TRY(hipMemcpyAsync(nbr, p->sp_nbr, sizeof(uint32_t) * ne, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_get_schur_pattern")
}

int c2b_problem_schur_complement(c2b_problem *p, double lambda, double *S_diag, double *S_off, double *b, int64_t *n_edges) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_complement: problem is NULL");
    if (!S_diag || !b || !n_edges) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_complement: NULL argument (S_diag, b, n_edges)");
    if (!aligned8(S_diag) || !aligned8(S_off) || !aligned8(b)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_complement: misaligned pointer");
    if (!good_lambda(lambda)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_complement: lambda must lie in [1e-20, 1e32]");
    NEED_UPLOADED(p, "problem_schur_complement");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_complement: a shard has no reduced system of its own (the point-side sums span every rank)");
    const int64_t nc = p->n_cam, no = p->n_obs;
    hipStream_t st = p->stream;
    if (!no && has_priors(p))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_complement: priors without a single observation are not solved (DESIGN 4.13)");
    int rc = ensure_schur_pattern(p);
    if (rc) return rc;
    if (p->sp_edges && !S_off) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_schur_complement: S_off is NULL and the pattern has %lld edges", (long long)p->sp_edges);
    *n_edges = p->sp_edges;
    if (!no) {                                               // no observation: U = 0, its damped diagonal alone; b = 0
        std::vector<double> h(81 * (size_t)nc, 0.0);
        for (int64_t c = 0; c < nc; ++c)
            for (int k = 0; k < 9; ++k) h[(size_t)c * 81 + k * 10] = lambda * 1e-6;
        if (nc) HIP_TRY(hipMemcpyAsync(S_diag, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st));
        if (nc) HIP_TRY(hipMemsetAsync(b, 0, sizeof(double) * 9 * (size_t)nc, st));
        HIP_TRY(hipStreamSynchronize(st));
        return C2B_OK;
    }
    rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (!rc) rc = ensure_transpose(p);
    if (rc) return rc;
    // the buffers in the explicit layout, whatever the handle's setting is (it is put back at once).  Under an implicit handle
    // they are freed again before returning: S and Y are gigabytes at scale, and an implicit solve has no use for them
    const int keep = p->schur_kind;
    p->schur_kind = C2B_SCHUR_EXPLICIT;
    rc = ensure_solver(p);
    const SolveBufs B = solve_bufs(p);
    p->schur_kind = keep;
    if (rc) return rc;
    rc = assemble_cameras(p, B.U, B.gc, 0.0, false);
    if (!rc) rc = assemble_points(p, B.V, B.gp, kConstPointV, false);
    if (!rc) rc = schur_explicit_setup(p, B, lambda, false);
    if (!rc) rc = schur_apply(p, B, lambda, nullptr, B.gp, B.t, false, B.gc, B.r, nullptr);      // b, as the step forms it
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(S_diag, B.Sd, sizeof(double) * 81 * (size_t)nc, hipMemcpyDeviceToDevice, st));
    if (p->sp_edges) HIP_TRY(hipMemcpyAsync(S_off, B.So, sizeof(double) * 81 * (size_t)p->sp_edges, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(b, B.r, sizeof(double) * 9 * (size_t)nc, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (keep != C2B_SCHUR_EXPLICIT) {                        // (the next solve allocates its own, smaller, buffers)
        p->sv.reset();
        p->sv_doubles = 0;
    }
    return C2B_OK;
    C2B_API_END("problem_schur_complement")
}

// ---- bal9 made the truth (the apply_step / rollback / resect rows of the table above cameras_mutated) -------------------
// Before bal9 is edited in place: in state mode it becomes to_vec of the cameras, unless it already is (bal9_fresh) ...
static int bal9_edit_begin(c2b_problem *p) {
    return p->bal_valid || p->bal9_fresh ? C2B_OK : c2b_cameras_to_bal(p->cam15, p->n_cam, p->bal9, p->stream);
}

// ... and after the edit returned rc: the cameras from bal9 by the kernel that builds them at upload_bal (the same bits),
// every cache of the cameras dropped (cameras_mutated), bal9 the truth
static int bal9_edit_end(c2b_problem *p, int rc) {
    if (!rc) rc = c2b_cameras_from_bal(p->bal9, p->n_cam, p->cam15, p->stream);
    cameras_mutated(p);
    p->bal_valid = true;
    return rc;
}

int c2b_problem_apply_step(c2b_problem *p, const double *dc, const double *dp) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_apply_step");
    if (!aligned8(dc) || !aligned8(dp)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_apply_step: misaligned pointer");
    const int64_t nc = p->n_cam, np = p->n_pts;
    hipStream_t st = p->stream;
    int rc = bal9_edit_begin(p);                             // state mode: the columns of dc refer to to_vec(cam15)
    if (rc) return rc;
    if (dc && nc && p->cmask)                                // a constant entry keeps its bits
        hipLaunchKernelGGL(k_add_free, dim3(blocks_for(9 * nc, kSchurBlock)), dim3(kSchurBlock), 0, st, 9 * nc, dc,
                           (const uint16_t *)p->cmask, p->bal9);
    else if (dc && nc) hipLaunchKernelGGL(k_add_f64, dim3(blocks_for(9 * nc, kSchurBlock)), dim3(kSchurBlock), 0, st, 9 * nc, dc, p->bal9);
    LAUNCH_CHECK();
    if ((rc = bal9_edit_end(p, C2B_OK))) return rc;
    if (dp && np) {
        if (p->pmask)
            hipLaunchKernelGGL(k_points_add_free, dim3(blocks_for(np, kSchurBlock)), dim3(kSchurBlock), 0, st, np, dp,
                               (const uint8_t *)p->pmask, reinterpret_cast<double4 *>(p->pts4.ptr));
        else
            hipLaunchKernelGGL(k_points_add, dim3(blocks_for(np, kSchurBlock)), dim3(kSchurBlock), 0, st, np, dp, reinterpret_cast<double4 *>(p->pts4.ptr));
        LAUNCH_CHECK();
    }
    HIP_TRY(hipStreamSynchronize(st));
    return C2B_OK;
    C2B_API_END("problem_apply_step")
}

// ---- what the start-up passes report ------------------------------------------------------------------------------------
// One status byte per entity and a count per kind of status: on the device while the pass runs (the Level 0 entries write
// them there), then copied to the caller.  Triangulation, resection and consensus triangulation report through it.
struct StatusReport {
    static constexpr int kMostKinds = 8;
    const int kinds;
    DevBuf<uint8_t> d_status;
    DevBuf<int64_t> d_counts;

    explicit StatusReport(int kinds_) : kinds(kinds_) {}

    hipError_t alloc(int64_t n) {
        const hipError_t e = d_status.alloc((size_t)n);
        return e == hipSuccess ? d_counts.alloc((size_t)kinds) : e;
    }
    // no observation: every one of the n entities has `kind` (too few), nothing is read or written on the device
    int all_have(int kind, int64_t n, uint8_t *status, int64_t *counts) {
        if (status && n) std::fill(status, status + n, (uint8_t)kind);
        if (counts) {
            std::fill(counts, counts + kinds, (int64_t)0);
            counts[kind] = n;
        }
        return C2B_OK;
    }
    // After the pass returned rc and the caller's own copies e: queue status and counts back, synchronise (the temporaries
    // are freed when the caller returns), and fold the three into the entry's result.
    int read_back(const char *who, hipStream_t st, int rc, hipError_t e, int64_t n, uint8_t *status, int64_t *counts) {
        int64_t got[kMostKinds];
        if (!rc && e == hipSuccess && status) e = hipMemcpyAsync(status, d_status, (size_t)n, hipMemcpyDeviceToHost, st);
        if (!rc && e == hipSuccess) e = hipMemcpyAsync(got, d_counts, sizeof(int64_t) * (size_t)kinds, hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (rc) return rc;
        if (e != hipSuccess || es != hipSuccess) return fail(C2B_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
        if (counts) std::copy(got, got + kinds, counts);
        return C2B_OK;
    }
};

// ---- linear midpoint triangulation -------------------------------------------------------------------------
// The resident points from the resident cameras and observations: c2b_triangulate_rows over the cached transpose (built as
// c2b_problem_solve_step builds it), the cameras read in the mode the problem is in.  Only pts4 changes, and nothing the
// problem caches is derived from the points (c2b_problem_apply_step drops nothing for a moved point either): the list, the
// row structure, the transpose, the solve buffers, the masks, the loss, the preconditioner and a checkpoint all stay.
int c2b_problem_triangulate_points(c2b_problem *p, double min_angle, uint8_t *status, int64_t *counts) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_triangulate_points");
    if (!good_min_angle(min_angle)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_points: min_angle must lie in [0, pi/2] radians");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_triangulate_points: a shard is not triangulated alone (a point's observations span every rank)");
    const int64_t np = p->n_pts;
    StatusReport rep(kTriKinds);
    if (!p->n_obs) return rep.all_have(kTriTooFew, np, status, counts);
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (!rc) rc = ensure_transpose(p);
    if (rc) return rc;
    const hipError_t e = rep.alloc(np);
    if (e != hipSuccess) return fail(hip_code(e), "problem_triangulate_points: allocation: %s", hipGetErrorString(e));
    rc = c2b_triangulate_rows(p->camblk, p->pts4, np, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, min_angle, p->pmask, rep.d_status, rep.d_counts, p->stream);
    return rep.read_back("problem_triangulate_points", p->stream, rc, hipSuccess, np, status, counts);
    C2B_API_END("problem_triangulate_points")
}

// ---- per-point Levenberg-Marquardt --------------------------------------------------------------------
// The resident points re-minimised one by one against the resident cameras: c2b_refine_points_rows over the cached transpose,
// under the handle's loss, point mask and point priors.  Only pts4 changes, so the handle is left as triangulation leaves
// it: the list, the row structure, the transpose, the solve buffers, the masks, the loss, the preconditioner, the priors
// and a checkpoint all stay.  Without a single observation a point has its prior alone: an empty transpose stands in.
// the launch over the resident buffers, which the entry below and lm_loop's inner iterations share: status and counts stay on
// the device (asynchronous); `ptr` is the transpose's row pointer (an all-zero one when the problem has no observation)
static int refine_resident(c2b_problem *p, const c2b_refine_options *opt, const uint64_t *ptr, uint8_t *d_status, int64_t *d_counts) {
    const bool obs = p->n_obs > 0;
    return c2b_refine_points_rows(p->camblk, p->pts4, p->n_pts, ptr, obs ? p->nt_obs.ptr : nullptr, obs ? p->nt_cam.ptr : nullptr, p->uv,
                                  p->loss_kind, p->loss_scale * p->loss_scale, p->pxw ? p->px0.ptr : nullptr, p->pxw ? p->pxw.ptr : nullptr, opt,
                                  p->pmask, d_status, d_counts, p->stream);
}

int c2b_problem_refine_points(c2b_problem *p, const c2b_refine_options *opt, uint8_t *status, int64_t *counts) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_refine_points");
    if (const int bad = check_refine_options("problem_refine_points", opt)) return bad;
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_refine_points: a shard is not refined alone (a point's observations span every rank)");
    const int64_t np = p->n_pts;
    StatusReport rep(kRefCounts);
    if (!np) return rep.all_have(kRefUnobserved, 0, status, counts);
    DevBuf<uint64_t> empty_ptr;
    int rc = ensure_camblk(p);
    if (!rc && p->n_obs) rc = ensure_rows(p);
    if (!rc && p->n_obs) rc = ensure_transpose(p);
    if (rc) return rc;
    hipError_t e = rep.alloc(np);
    if (e == hipSuccess && !p->n_obs) {
        e = empty_ptr.alloc((size_t)np + 1);
        if (e == hipSuccess) e = hipMemsetAsync(empty_ptr, 0, sizeof(uint64_t) * ((size_t)np + 1), p->stream);
    }
    if (e != hipSuccess) return fail(hip_code(e), "problem_refine_points: allocation: %s", hipGetErrorString(e));
    rc = refine_resident(p, opt, p->n_obs ? p->nt_ptr.ptr : empty_ptr.ptr, rep.d_status, rep.d_counts);
    return rep.read_back("problem_refine_points", p->stream, rc, hipSuccess, np, status, counts);
    C2B_API_END("problem_refine_points")
}

// inner iterations of the LM loop: the handle's state, like the loss (it survives uploads and reads)
int c2b_problem_set_inner_iterations(c2b_problem *p, int rounds) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_inner_iterations: problem is NULL");
    if (rounds < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_inner_iterations: rounds must be >= 0, not %d", rounds);
    p->inner_rounds = rounds;
    return C2B_OK;
    C2B_API_END("problem_set_inner_iterations")
}

int c2b_problem_get_inner_iterations(c2b_problem *p, int *rounds) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_inner_iterations: problem is NULL");
    if (rounds) *rounds = p->inner_rounds;
    return C2B_OK;
    C2B_API_END("problem_get_inner_iterations")
}

// ---- camera resection ---------------------------------------------------------------------------------
// The resident cameras' poses from the resident points and observations: c2b_resect_rows over the row structure, in place
// on bal9, which is made the truth first as c2b_problem_apply_step makes it (state mode: to_vec of the cameras) and stays
// the truth: the cameras moved, so their caches go (cameras_mutated) exactly as after a camera step.  The list, the row
// structure, the transpose, the solve buffers, the masks, the loss, the preconditioner and a checkpoint all stay.
int c2b_problem_resect_cameras(c2b_problem *p, int min_points, double min_gap, uint8_t *status, int64_t *counts) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_resect_cameras");
    if (min_points < kResMinPoints) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_cameras: min_points must be at least %d", kResMinPoints);
    if (!good_min_gap(min_gap)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_cameras: min_gap must lie in [0, 1)");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_resect_cameras: a shard is not resected alone");
    const int64_t nc = p->n_cam;
    StatusReport rep(kResKinds);
    if (!p->n_obs) return rep.all_have(kResTooFew, nc, status, counts);
    int rc = ensure_rows(p);
    if (rc) return rc;
    const hipError_t e = rep.alloc(nc);
    if (e != hipSuccess) return fail(hip_code(e), "problem_resect_cameras: allocation: %s", hipGetErrorString(e));
    hipStream_t st = p->stream;
    if ((rc = bal9_edit_begin(p))) return rc;                // state mode: the pass works on to_vec(cam15)
    rc = c2b_resect_rows(p->bal9, p->pts4, p->rows_ptr, nc, p->pt_idx, p->uv, min_points, min_gap, p->cmask, rep.d_status, rep.d_counts, st);
    rc = bal9_edit_end(p, rc);
    return rep.read_back("problem_resect_cameras", st, rc, hipSuccess, nc, status, counts);
    C2B_API_END("problem_resect_cameras")
}

// ---- per-camera Levenberg-Marquardt -------------------------------------------------------------------
// The resident cameras re-minimised one by one against the resident points: c2b_refine_cameras_rows over the row structure, in
// place on bal9, which is made the truth first and stays the truth exactly as in c2b_problem_resect_cameras, under the handle's
// loss, camera mask, centre priors and intrinsics priors.  The list, the row structure, the transpose, the solve buffers, the
// masks, the loss, the preconditioner, the priors and a checkpoint all stay.  Without a single observation a camera has its
// priors alone: an all-zero row pointer stands in.
int c2b_problem_refine_cameras(c2b_problem *p, const c2b_refine_options *opt, uint8_t *status, int64_t *counts) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_refine_cameras");
    if (const int bad = check_refine_options("problem_refine_cameras", opt)) return bad;
    if (p->shard_n_cam_global >= 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_refine_cameras: a shard is not refined alone");
    const int64_t nc = p->n_cam;
    StatusReport rep(kRefCounts);
    if (!nc) return rep.all_have(kRefUnobserved, 0, status, counts);
    DevBuf<uint64_t> empty_ptr;
    int rc = ensure_rows(p);
    if (rc) return rc;
    hipStream_t st = p->stream;
    hipError_t e = rep.alloc(nc);
    if (e == hipSuccess && !p->n_obs) {
        e = empty_ptr.alloc((size_t)nc + 1);
        if (e == hipSuccess) e = hipMemsetAsync(empty_ptr, 0, sizeof(uint64_t) * ((size_t)nc + 1), st);
    }
    if (e != hipSuccess) return fail(hip_code(e), "problem_refine_cameras: allocation: %s", hipGetErrorString(e));
    if ((rc = bal9_edit_begin(p))) return rc;                // state mode: the pass works on to_vec(cam15)
    rc = c2b_refine_cameras_rows(p->bal9, p->pts4, nc, p->n_obs ? p->rows_ptr.ptr : empty_ptr.ptr, p->pt_idx, p->uv, p->loss_kind,
                                 p->loss_scale * p->loss_scale, p->pcw ? p->pc0.ptr : nullptr, p->pcw ? p->pcw.ptr : nullptr,
                                 p->piw ? p->pi0.ptr : nullptr, p->piw ? p->piw.ptr : nullptr, opt, p->cmask, rep.d_status, rep.d_counts, st);
    rc = bal9_edit_end(p, rc);
    return rep.read_back("problem_refine_cameras", st, rc, hipSuccess, nc, status, counts);
    C2B_API_END("problem_refine_cameras")
}

// ---- Levenberg-Marquardt on the device -----------------------------------------------------------------
int c2b_problem_checkpoint(c2b_problem *p) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_checkpoint");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_checkpoint: a shard cannot be solved alone, so it takes no checkpoint");
    p->ck_valid = false;
    const int rc = c2b_problem_apply_step(p, nullptr, nullptr);          // bal mode: bal9 and pts4 are then the whole state
    if (rc) return rc;
    if (!p->ck_bal9 || !p->ck_pts4) {
        hipError_t e = p->ck_bal9.alloc(9 * (size_t)p->n_cam);
        if (e == hipSuccess) e = p->ck_pts4.alloc(4 * (size_t)p->n_pts);
        if (e != hipSuccess) { drop_lm_state(p); return fail(hip_code(e), "problem_checkpoint: allocation: %s", hipGetErrorString(e)); }
    }
    if (p->n_cam) HIP_TRY(hipMemcpyAsync(p->ck_bal9, p->bal9, sizeof(double) * 9 * (size_t)p->n_cam, hipMemcpyDeviceToDevice, p->stream));
    if (p->n_pts) HIP_TRY(hipMemcpyAsync(p->ck_pts4, p->pts4, sizeof(double) * 4 * (size_t)p->n_pts, hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->ck_valid = true;
    return C2B_OK;
    C2B_API_END("problem_checkpoint")
}

int c2b_problem_rollback(c2b_problem *p) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_rollback");
    if (!p->ck_valid) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_rollback: the problem holds no checkpoint");
    hipStream_t st = p->stream;
    if (p->n_cam) HIP_TRY(hipMemcpyAsync(p->bal9, p->ck_bal9, sizeof(double) * 9 * (size_t)p->n_cam, hipMemcpyDeviceToDevice, st));
    const int rc = bal9_edit_end(p, C2B_OK);                 // the cameras' caches only: rows, transpose, solve buffers, masks stay
    if (rc) return rc;
    if (p->n_pts) HIP_TRY(hipMemcpyAsync(p->pts4, p->ck_pts4, sizeof(double) * 4 * (size_t)p->n_pts, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return C2B_OK;
    C2B_API_END("problem_rollback")
}

int c2b_problem_drop_checkpoint(c2b_problem *p) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_drop_checkpoint: problem is NULL");
    p->ck_valid = false;                                     // (the buffers stay for the next checkpoint of these counts)
    return C2B_OK;
    C2B_API_END("problem_drop_checkpoint")
}

// c2b_problem::lm, carved: dc [n_cam][9], dp [n_pts][3], the partials of k_lm_norms (kLmSums x grid; k_lm_gradient_max
// uses the first 2 x grid of them after those were summed), the device scalars: the four sums, then the two maxima; then what
// the inner iterations' refinement reports and nobody reads: its six counts and a status byte per point
struct LmBufs {
    double *dc, *dp, *part, *sc;
    int64_t *inner_counts;
    uint8_t *inner_status;
    unsigned grid;
};
enum { kLmScGradCam = kLmSums, kLmScGradPts = kLmSums + 1, kLmScSlots = 8 };

static LmBufs lm_bufs(c2b_problem *p) {
    LmBufs b;
    b.grid = lm_grid(std::max<int64_t>(9 * p->n_cam, 3 * p->n_pts));
    b.dc = p->lm;
    b.dp = b.dc + 9 * p->n_cam;
    b.part = b.dp + 3 * p->n_pts;
    b.sc = b.part + (int64_t)kLmSums * b.grid;
    b.inner_counts = reinterpret_cast<int64_t *>(b.sc + kLmScSlots);
    b.inner_status = reinterpret_cast<uint8_t *>(b.inner_counts + kRefCounts);
    return b;
}

static int ensure_lm(c2b_problem *p) {
    if (p->lm) return C2B_OK;                                // (dropped whenever a count changes)
    const int64_t n = 9 * p->n_cam + 3 * p->n_pts + (int64_t)kLmSums * lm_grid(std::max<int64_t>(9 * p->n_cam, 3 * p->n_pts)) + kLmScSlots +
                      kRefCounts + (p->n_pts + 7) / 8;
    const hipError_t e = p->lm.alloc((size_t)n);
    if (e != hipSuccess) return fail(hip_code(e), "problem_levenberg_marquardt: allocation: %s", hipGetErrorString(e));
    return C2B_OK;
}

// x^y by libm's pow, as CPython's ** evaluates it: the exponent is kept from the compiler, which would otherwise turn a
// constant 2 or 3 into multiplications (the last bit can differ)
static double libm_pow(double x, double y) {
    volatile double e = y;
    return std::pow(x, e);
}

// the cost the loop compares: sum rho(|r|^2) under a loss, else the square of the root total_reprojection_error returns
// (the numbers of city2ba_amd/solve.py's loop)
static int lm_cost_observations(c2b_problem *p, double *cost) {
    if (p->loss_kind != kLossSquared) return c2b_problem_robust_cost(p, cost);
    double e = 0.0;
    const int rc = c2b_problem_total_reprojection_error(p, 2.0, &e);
    if (rc) return rc;
    *cost = libm_pow(e, 2.0);
    return C2B_OK;
}

// ... plus the priors' cost when any is in force, added in that order
static int lm_cost(c2b_problem *p, double *cost) {
    int rc = lm_cost_observations(p, cost);
    if (rc || !has_priors(p)) return rc;
    double pc = 0.0;
    if ((rc = c2b_problem_prior_cost(p, &pc))) return rc;
    *cost = *cost + pc;
    return C2B_OK;
}

static int lm_loop(c2b_problem *p, const c2b_lm_options &o, c2b_lm_iteration *history, c2b_lm_summary *summary) {
    const int64_t nc = p->n_cam, np = p->n_pts;
    hipStream_t st = p->stream;
    auto clamp = [](double l) { return std::min(std::max(l, C2B_STEP_LAMBDA_MIN), C2B_STEP_LAMBDA_MAX); };
    int rc = ensure_lm(p);
    if (!rc) rc = c2b_problem_checkpoint(p);                 // bal mode; the state every rejected step returns to
    if (rc) return rc;
    const LmBufs L = lm_bufs(p);
    double lam = clamp(o.lambda0), nu = 2.0, e0 = 0.0;
    if ((rc = lm_cost(p, &e0))) return rc;
    c2b_lm_summary sum{0, 0, e0, e0, lam};
    if (!std::isfinite(e0)) sum.termination = 4;
    while (!sum.termination && sum.iterations < o.max_iterations) {
        c2b_step_info info;
        if ((rc = c2b_problem_solve_step(p, lam, o.pcg_max_iters, o.pcg_rel_tol, L.dc, L.dp, &info))) return rc;
        // the gradient the solve kept (no observation: it has none and g = 0) and the norms of its step and of the state
        const bool have_g = p->n_obs > 0;
        hipLaunchKernelGGL(k_lm_norms, dim3(L.grid), dim3(kSchurBlock), 0, st, 9 * nc, np, (const double *)p->bal9,
                           reinterpret_cast<const double4 *>(p->pts4.ptr), (const double *)L.dc, (const double *)L.dp, L.part);
        for (int k = 0; k < kLmSums; ++k)
            fold_sum(st, L.part + (int64_t)k * L.grid, (int)L.grid, L.sc + k);
        if (have_g) {
            const SolveBufs B = solve_bufs(p);
            hipLaunchKernelGGL(k_lm_gradient_max, dim3(L.grid), dim3(kSchurBlock), 0, st, 9 * nc, 3 * np, (const double *)B.gc,
                               (const double *)B.gp, L.part);
            hipLaunchKernelGGL(k_lm_max_fold, dim3(1), dim3(kSchurBlock), 0, st, (const double *)L.part, (int)L.grid, L.sc + kLmScGradCam);
        }
        HIP_TRY(launch_error());
        double h[kLmScSlots] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if ((rc = scalars_to_host(st, L.sc, have_g ? kLmScGradPts + 1 : kLmSums, h))) return rc;
        c2b_lm_iteration it{};
        it.cost = it.cost_trial = e0;
        it.lambda = lam;
        it.model_decrease = info.model_decrease;
        it.gradient_max = (h[kLmScGradCam] > h[kLmScGradPts] || h[kLmScGradCam] != h[kLmScGradCam]) ? h[kLmScGradCam] : h[kLmScGradPts];
        it.step_norm = std::sqrt(h[kLmStepCam] + h[kLmStepPts]);
        it.x_norm = std::sqrt(h[kLmXCam] + h[kLmXPts]);
        it.pcg_rel_residual = info.rel_residual;
        it.pcg_iterations = info.iterations;
        it.status = info.status;
        c2b_lm_iteration *slot = history ? history + sum.iterations : nullptr;
        ++sum.iterations;
        if (!std::isfinite(it.gradient_max)) sum.termination = 4;                 // (the step was not applied: nothing to roll back)
        else if (o.gradient_tol > 0.0 && it.gradient_max <= o.gradient_tol) sum.termination = 2;
        else if (o.parameter_tol > 0.0 && it.step_norm <= o.parameter_tol * (it.x_norm + o.parameter_tol)) sum.termination = 3;
        if (sum.termination) {
            if (slot) *slot = it;
            break;
        }
        if ((rc = c2b_problem_apply_step(p, L.dc, L.dp))) return rc;
        if (p->inner_rounds && p->n_obs) {                   // inner iterations: the points against the moved cameras,
            const c2b_refine_options inner{p->inner_rounds, 0, 1e-4, 0.0, 0.0, 0.0};       // queued like any pass: no allocation, no read-back
            if ((rc = ensure_camblk(p))) return rc;          // (the rows and the transpose are the solve's)
            if ((rc = refine_resident(p, &inner, p->nt_ptr, L.inner_status, L.inner_counts))) return rc;
        }
        double e1 = 0.0;
        if ((rc = lm_cost(p, &e1))) return rc;
        it.cost_trial = e1;
        const double md = info.model_decrease;
        const double rho = md > 0.0 ? (e0 - e1) / md : -1.0;
        it.accepted = rho > 0.0 && e1 < e0;
        if (slot) *slot = it;
        if (it.accepted) {
            lam = clamp(lam * std::max(1.0 / 3.0, 1.0 - libm_pow(2.0 * rho - 1.0, 3.0)));
            nu = 2.0;
            if ((rc = c2b_problem_checkpoint(p))) return rc;
            if (o.function_tol > 0.0 && e0 - e1 <= o.function_tol * e0) sum.termination = 1;
            e0 = e1;
        } else {
            if ((rc = c2b_problem_rollback(p))) return rc;
            lam = clamp(lam * nu);
            nu *= 2.0;
            if (!std::isfinite(e1)) sum.termination = 4;
        }
    }
    sum.final_cost = e0;
    sum.lambda_next = lam;
    if (summary) *summary = sum;
    return C2B_OK;
}

int c2b_problem_levenberg_marquardt(c2b_problem *p, const c2b_lm_options *opt, c2b_lm_iteration *history, int capacity,
                                    c2b_lm_summary *summary) {
    C2B_API_BEGIN
    if (!p || !opt) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_levenberg_marquardt: NULL argument");
    if (opt->max_iterations < 0 || opt->pcg_max_iters < 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_levenberg_marquardt: max_iterations and pcg_max_iters must be >= 0");
    if (!good_lambda(opt->lambda0)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_levenberg_marquardt: lambda0 must lie in [1e-20, 1e32]");
    for (const double t : {opt->pcg_rel_tol, opt->function_tol, opt->gradient_tol, opt->parameter_tol})
        if (!(t >= 0.0) || !std::isfinite(t))
            return fail(C2B_ERR_INVALID_ARGUMENT, "problem_levenberg_marquardt: tolerances must be finite and >= 0");
    if (history && capacity < opt->max_iterations)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_levenberg_marquardt: history holds %d entries, max_iterations is %d", capacity,
                    (int)opt->max_iterations);
    NEED_UPLOADED(p, "problem_levenberg_marquardt");
    if (p->shard_n_cam_global >= 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_levenberg_marquardt: a shard cannot be solved alone (the point-side sums span every rank)");
    if (!p->n_obs && has_priors(p))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_levenberg_marquardt: priors without a single observation are not solved (DESIGN 4.13)");
    const int rc = lm_loop(p, *opt, history, summary);
    p->ck_valid = false;                                     // the checkpoint was the loop's
    return rc;
    C2B_API_END("problem_levenberg_marquardt")
}
