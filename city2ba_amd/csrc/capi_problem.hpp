// capi_problem.hpp -- Level 1 of include/city2ba_hip.h: a BAProblem resident on one device (c2b_problem_*), its device-side generators, cull, file images, noise functions, and the *_sharded forms
// Part of the one translation unit of the C ABI: included by capi.hip (inside its extern "C" block, after its helpers and
// launchers), never compiled or included on its own.

/* ------------------------------- level 1 --------------------------------------------- */

struct c2b_problem {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n_cam = 0, n_pts = 0, n_obs = 0;
    // every device array below is a DevBuf (capi.hip): the problem owns its memory through that one type, and the four
    // functions under this struct say which group of them goes when
    DevBuf<double> cam15, bal9, camblk, cen4, pts4, uv;
    // cen4[n_cam][4]: the cameras' centres as 32-byte rows (derived with camblk, valid when blk_valid): what the statistics
    // and the centre-keyed cell lists read -- a 128-byte line of camblk per camera otherwise
    DevBuf<uint32_t> cam_idx, pt_idx;
    DevBuf<char> ws;
    DevBuf<double> stats, scalar;
    // this problem as ONE SHARD of a larger one (c2b_problem_set_shard): its cameras are [shard_cam_base, + n_cam) of
    // shard_n_cam_global (< 0: not a shard), its first observation is observation shard_obs_base of the whole list
    int64_t shard_cam_base = 0, shard_n_cam_global = -1, shard_obs_base = 0;
    c2b_problem_options opt{0, 0, 0, 0, 0, 0, -1};   // c2b_problem_set_options; survives uploads / reads (it is the handle's, not the data's)
    // c2b_problem_set_loss: the robust loss of normal_equations / solve_step / robust_cost (0 squared, 1 Huber, 2 Cauchy,
    // 3 soft-L1) and its scale; the handle's too
    int loss_kind = 0;
    double loss_scale = 1.0;
    // c2b_problem_set_preconditioner: what c2b_problem_solve_step's PCG is preconditioned with (0 block-Jacobi on U,
    // 1 Schur-Jacobi), the handle's too; and how many cameras' Schur-Jacobi factors fell back in the last solve
    int precond_kind = 0;
    int64_t precond_fallbacks = 0;
    // c2b_problem_set_constant: the camera parameters (bit k of a camera's word, to_vec order) and the points
    // (0 / 1) that normal_equations / solve_step / apply_step hold constant; the handle's, kept while both counts stay
    // what they were set for (const_n_cam, const_n_pts).  A kind with nothing set has no array: no launch changes for it.
    DevBuf<uint16_t> cmask;
    DevBuf<uint8_t> pmask;
    std::vector<uint16_t> h_cmask;
    std::vector<uint8_t> h_pmask;
    int64_t const_n_cam = -1, const_n_pts = -1, const_params = 0, const_pts = 0;
    bool bal_valid = false;     // bal9 still describes the cameras (no mutation since upload_bal)
    bool blk_valid = false;     // camblk matches cam15 (and bal_valid mode)
    bool bal9_fresh = false;    // !bal_valid, but bal9 holds to_vec of the current cameras (the last write / download_bal computed it)
    // the row structure of the observation list for the *_rows launchers, rebuilt on demand after the list changed
    DevBuf<uint64_t> rows_ptr;
    DevBuf<char> rows_tiles;
    bool rows_valid = false;
    // its point-major transpose for c2b_problem_normal_equations (pt_row_ptr [n_pts + 1], obs_of / cam_of [n_obs]), dropped with it
    DevBuf<uint64_t> nt_ptr;
    DevBuf<uint32_t> nt_obs, nt_cam;
    // c2b_problem_solve_step's buffers (U, gc, V, gp, the preconditioner's factors, the PCG vectors, partials, scalars):
    // one allocation, sized by the list, dropped with it
    DevBuf<double> sv;
    int64_t sv_doubles = 0;
    // c2b_problem_checkpoint: bal9 and pts4 as they were when it was taken, what c2b_problem_rollback copies
    // back.  Allocated on first use and reused while the counts stay; ck_valid says whether they hold a checkpoint.
    // lm: the scratch of c2b_problem_levenberg_marquardt (its step, the partials and scalars of k_lm_norms /
    // k_lm_gradient_max), sized by the counts.  Both go with the entities (drop_lm_state).
    DevBuf<double> ck_bal9, ck_pts4, lm;
    bool ck_valid = false;
    DevBuf<uint32_t> dense_pt;      // survivors of the last dense visibility sweep
    DevBuf<double> dense_uv;
    DevBuf<uint64_t> dense_row;     // its CSR row pointer [n_cam + 1], kept for the occlusion filter
    int64_t dense_n = 0;
    // residual + Jacobian to host buffers: a ring of chunk-sized device buffers, a copy stream, per-slot events
    static constexpr int kJacSlots = 3;
    static constexpr int64_t kJacChunk = 256 * 1024;       // observations per chunk (53 MB of results)
    DevBuf<double> jac_ring;                               // kJacSlots x kJacChunk x 26 doubles
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_done[kJacSlots] = {nullptr, nullptr, nullptr}, ev_free[kJacSlots] = {nullptr, nullptr, nullptr};
};

static void cameras_mutated(c2b_problem *p);

// the pending visibility result goes (a new sweep, a cull, new points)
static void free_dense(c2b_problem *p) {
    p->dense_pt.reset(); p->dense_uv.reset(); p->dense_row.reset();
    p->dense_n = 0;
}

// the observation list changed (upload, cull, adopted visibility): its row structure is rebuilt by the next user
static void drop_rows(c2b_problem *p) {
    p->rows_ptr.reset(); p->rows_tiles.reset();
    p->rows_valid = false;
    p->nt_ptr.reset(); p->nt_obs.reset(); p->nt_cam.reset();
    p->sv.reset();
    p->sv_doubles = 0;
}

// the entities were renumbered or their counts changed: nothing is constant any more
static void drop_constant(c2b_problem *p) {
    p->cmask.reset(); p->pmask.reset();
    p->h_cmask.clear(); p->h_pmask.clear();
    p->const_n_cam = p->const_n_pts = -1;
    p->const_params = p->const_pts = 0;
}

// the entities were replaced, renumbered or their counts changed: no checkpoint describes them any more
static void drop_lm_state(c2b_problem *p) {
    p->ck_bal9.reset(); p->ck_pts4.reset(); p->lm.reset();
    p->ck_valid = false;
}

// everything but the constant masks goes: "nothing uploaded"
static void free_buffers(c2b_problem *p) {
    drop_lm_state(p);
    p->cam15.reset(); p->bal9.reset(); p->camblk.reset(); p->cen4.reset(); p->pts4.reset(); p->uv.reset();
    p->cam_idx.reset(); p->pt_idx.reset();
    p->ws.reset(); p->stats.reset(); p->scalar.reset(); p->jac_ring.reset();
    free_dense(p);
    drop_rows(p);
    p->n_cam = p->n_pts = p->n_obs = 0;
    p->bal_valid = p->blk_valid = p->bal9_fresh = false;
}

void c2b_problem_options_init(c2b_problem_options *o) {
    if (o) *o = c2b_problem_options{0, 0, 0, 0, 0, 0, -1};
}
int c2b_problem_set_options(c2b_problem *p, const c2b_problem_options *o) {
    if (!p || !o) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_options: NULL argument");
    if (o->read_threads < 0 || o->read_threads > 64 || o->io_threads < 0 || o->io_threads > 64 || o->rank_sort_max_row < 0 || o->reserved != 0)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_options: thread counts must be in [0, 64], rank_sort_max_row >= 0, reserved 0");
    p->opt = *o;
    return C2B_OK;
}
int c2b_problem_get_options(const c2b_problem *p, c2b_problem_options *o) {
    if (!p || !o) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_get_options: NULL argument");
    *o = p->opt;
    return C2B_OK;
}
void c2b_host_set_io_threads(int n) { c2b_host::io_threads_setting().store(n < 1 ? 0 : (n > 64 ? 64 : n), std::memory_order_relaxed); }

int c2b_problem_create(int device, c2b_problem **out) {
    C2B_API_BEGIN
    if (!out) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(C2B_ERR_NO_DEVICE, "problem_create: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_create: device %d out of range [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    c2b_problem *p = new (std::nothrow) c2b_problem();
    if (!p) return fail(C2B_ERR_OOM, "problem_create: host allocation failed");
    p->device = device;
    hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete p; return fail(C2B_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    *out = p;
    return C2B_OK;
    C2B_API_END("problem_create")
}

void c2b_problem_destroy(c2b_problem *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    free_buffers(p);
    drop_constant(p);
    for (int k = 0; k < c2b_problem::kJacSlots; ++k) {
        if (p->ev_done[k]) (void)hipEventDestroy(p->ev_done[k]);
        if (p->ev_free[k]) (void)hipEventDestroy(p->ev_free[k]);
    }
    if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

static int ensure_camblk(c2b_problem *p) {
    if (p->blk_valid) return C2B_OK;
    int rc = p->bal_valid ? c2b_camblk_from_bal(p->bal9, p->n_cam, p->camblk, cam_table_doubles(p->n_cam), p->cen4, p->stream)
                          : c2b_camblk_from_state(p->cam15, p->n_cam, p->camblk, cam_table_doubles(p->n_cam), p->cen4, p->stream);
    if (rc) return rc;
    p->blk_valid = true;
    return C2B_OK;
}

// the resident arrays of a problem with these sizes (whatever it held before is freed); contents undefined.  The constant
// masks go too, unless the caller brings the same entities back (an upload) and both counts are those they were set for.
static int alloc_problem(c2b_problem *p, int64_t n_cam, int64_t n_pts, int64_t n_obs, bool same_entities = false) {
    HIP_TRY(hipSetDevice(p->device));
    free_buffers(p);
    if (!same_entities || n_cam != p->const_n_cam || n_pts != p->const_n_pts) drop_constant(p);
    HIP_TRY(p->cam15.alloc(15 * (size_t)n_cam));
    HIP_TRY(p->bal9.alloc(9 * (size_t)n_cam));
    HIP_TRY(p->camblk.alloc((size_t)cam_table_doubles(n_cam)));      // whole groups of 8 cameras
    HIP_TRY(p->cen4.alloc(4 * (size_t)n_cam));
    HIP_TRY(p->pts4.alloc(4 * (size_t)n_pts));
    HIP_TRY(p->uv.alloc(2 * (size_t)n_obs));
    HIP_TRY(p->cam_idx.alloc((size_t)n_obs));
    HIP_TRY(p->pt_idx.alloc((size_t)n_obs));
    HIP_TRY(p->ws.alloc((size_t)c2b_workspace_bytes(n_obs)));
    if (int rc = c2b_workspace_init(p->ws, p->stream)) return rc;
    HIP_TRY(p->stats.alloc(C2B_STATS_DOUBLES));
    HIP_TRY(p->scalar.alloc(2));
    p->n_cam = n_cam; p->n_pts = n_pts; p->n_obs = n_obs;
    return C2B_OK;
}

static int upload_common(c2b_problem *p, int64_t n_cam, const double *cams, bool is_bal, int64_t n_pts,
                         const double *pts3, const uint64_t *row_ptr, const uint64_t *pt_idx, const double *uv) {
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_upload: problem is NULL");
    if (n_cam < 0 || n_pts < 0 || (n_cam && !cams) || (n_pts && !pts3) || !row_ptr)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_upload: bad arguments");
    if (n_cam >= ((int64_t)1 << 32) || n_pts >= ((int64_t)1 << 32))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_upload: device indices are 32-bit");
    // assert!(cams.len() == obs.len()) is structural here; row_ptr must be a monotone prefix
    if (row_ptr[0] != 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_upload: row_ptr[0] != 0");
    for (int64_t c = 0; c < n_cam; ++c)
        if (row_ptr[c + 1] < row_ptr[c]) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_upload: row_ptr not monotone at camera %lld", (long long)c);
    const int64_t n_obs = (int64_t)row_ptr[n_cam];
    if (n_obs && (!pt_idx || !uv)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_upload: NULL observations");
    std::vector<uint32_t> pi32((size_t)n_obs);
    for (int64_t o = 0; o < n_obs; ++o) {
        // assert!(ci < &points.len()), src/baproblem.rs:368
        if (pt_idx[o] >= (uint64_t)n_pts)
            return fail(C2B_ERR_INDEX_OUT_OF_RANGE, "problem_upload: observation %lld refers to point %llu >= %lld",
                        (long long)o, (unsigned long long)pt_idx[o], (long long)n_pts);
        pi32[(size_t)o] = (uint32_t)pt_idx[o];
    }
    if (int rc = alloc_problem(p, n_cam, n_pts, n_obs, true)) return rc;
    // staging through temporary device buffers (row_ptr, packed points)
    DevBuf<uint64_t> d_row;
    DevBuf<double> d_p3;
    HIP_TRY(d_row.alloc((size_t)n_cam + 1));
    const hipError_t e = d_p3.alloc(3 * (size_t)n_pts);
    if (e != hipSuccess) return fail(C2B_ERR_OOM, "problem_upload: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(d_row, row_ptr, sizeof(uint64_t) * (n_cam + 1), hipMemcpyHostToDevice, p->stream));
    if (n_pts) HIP_TRY(hipMemcpyAsync(d_p3, pts3, sizeof(double) * 3 * n_pts, hipMemcpyHostToDevice, p->stream));
    if (n_obs) {
        HIP_TRY(hipMemcpyAsync(p->pt_idx, pi32.data(), sizeof(uint32_t) * n_obs, hipMemcpyHostToDevice, p->stream));
        HIP_TRY(hipMemcpyAsync(p->uv, uv, sizeof(double) * 2 * n_obs, hipMemcpyHostToDevice, p->stream));
    }
    int rc = C2B_OK;
    if (is_bal) {
        if (n_cam) HIP_TRY(hipMemcpyAsync(p->bal9, cams, sizeof(double) * 9 * n_cam, hipMemcpyHostToDevice, p->stream));
        if ((rc = c2b_cameras_from_bal(p->bal9, n_cam, p->cam15, p->stream))) return rc;
    } else {
        if (n_cam) HIP_TRY(hipMemcpyAsync(p->cam15, cams, sizeof(double) * 15 * n_cam, hipMemcpyHostToDevice, p->stream));
    }
    if ((rc = c2b_points_pad(d_p3, n_pts, p->pts4, p->stream))) return rc;
    if ((rc = c2b_expand_rows(d_row, n_cam, 0, n_obs, p->cam_idx, p->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->bal_valid = is_bal;
    p->blk_valid = false;
    return C2B_OK;
}

int c2b_problem_upload(c2b_problem *p, int64_t n_cam, const double *cams15, int64_t n_pts, const double *pts3,
                       const uint64_t *row_ptr, const uint64_t *pt_idx, const double *uv) {
    C2B_API_BEGIN
    return upload_common(p, n_cam, cams15, false, n_pts, pts3, row_ptr, pt_idx, uv);
    C2B_API_END("problem_upload")
}

int c2b_problem_upload_bal(c2b_problem *p, int64_t n_cam, const double *bal9, int64_t n_pts, const double *pts3,
                           const uint64_t *row_ptr, const uint64_t *pt_idx, const double *uv) {
    C2B_API_BEGIN
    return upload_common(p, n_cam, bal9, true, n_pts, pts3, row_ptr, pt_idx, uv);
    C2B_API_END("problem_upload_bal")
}

// synthetic_grid's / synthetic_line's layout loops (src/synthetic.rs:178-258, :323-344) straight into the resident problem:
// cameras by Camera::from_position_direction, points, no observations yet (the visibility loop adds them).  Entity for
// entity and bit for bit what c2b_synthetic_grid_layout + c2b_problem_from_position_direction + c2b_problem_upload give,
// without 2 x 112 MB crossing PCIe.  The orientations' sines and cosines come from the host's libm like the host
// layout's (Basis3::from_angle_y(Deg(..)), :191-205).
static GridDirs layout_dirs() {
    GridDirs d;
    c2b_host::basis_from_angle_y_deg(-90.0, d.m[0]);
    c2b_host::basis_from_angle_y_deg(90.0, d.m[1]);
    c2b_host::basis_from_angle_y_deg(180.0, d.m[2]);
    const double one[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::copy(one, one + 9, d.m[3]);
    return d;
}

int c2b_problem_synthetic_grid_layout(c2b_problem *p, int64_t cpb, int64_t ppb, int64_t blocks, double block_length,
                                      double block_inset, double camera_height, double point_height) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_synthetic_grid_layout: problem is NULL");
    if (cpb < 0 || ppb < 0 || blocks < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_synthetic_grid_layout: bad arguments");
    // assert!(block_inset * 2. < block_length, ...), src/synthetic.rs:177
    if (!(block_inset * 2.0 < block_length))
        return fail(C2B_ERR_INVALID_ARGUMENT,
                    "Block inset (%g) must be less than half the block length (%g), to not violate physical constraints.",
                    block_inset, block_length);
    int64_t n_cam = 0, n_pts = 0;
    c2b_host::grid_sizes(cpb, ppb, blocks, &n_cam, &n_pts);
    if (n_cam >= ((int64_t)1 << 32) || n_pts >= ((int64_t)1 << 32))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_synthetic_grid_layout: device indices are 32-bit");
    int rc = alloc_problem(p, n_cam, n_pts, 0);
    if (rc) return rc;
    if (n_cam) hipLaunchKernelGGL(k_grid_cameras, dim3(blocks_for(n_cam, 256)), dim3(256), 0, p->stream, n_cam, cpb, blocks, block_length,
                                  camera_height, layout_dirs(), p->cam15);
    if (n_pts) hipLaunchKernelGGL(k_grid_points, dim3(blocks_for(n_pts, 256)), dim3(256), 0, p->stream, n_pts, ppb, blocks, block_length,
                                  block_inset, point_height, reinterpret_cast<double4 *>(p->pts4.ptr));
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->bal_valid = false; p->blk_valid = false;
    return C2B_OK;
    C2B_API_END("problem_synthetic_grid_layout")
}

int c2b_problem_synthetic_line_layout(c2b_problem *p, int64_t n_cam, int64_t n_pts, double length, double point_offset,
                                      double camera_height, double point_height) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_synthetic_line_layout: problem is NULL");
    if (n_cam < 0 || n_pts < 0 || n_cam >= ((int64_t)1 << 32) || n_pts >= ((int64_t)1 << 32))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_synthetic_line_layout: bad arguments");
    int rc = alloc_problem(p, n_cam, n_pts, 0);
    if (rc) return rc;
    const int64_t n = std::max(n_cam, n_pts);
    if (n) hipLaunchKernelGGL(k_line_layout, dim3(blocks_for(n, 256)), dim3(256), 0, p->stream, n_cam, n_pts, length, point_offset,
                              camera_height, point_height, layout_dirs(), p->cam15, reinterpret_cast<double4 *>(p->pts4.ptr));
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->bal_valid = false; p->blk_valid = false;
    return C2B_OK;
    C2B_API_END("problem_synthetic_line_layout")
}

int c2b_problem_sizes(const c2b_problem *p, int64_t *n_cam, int64_t *n_pts, int64_t *n_obs) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_sizes: problem is NULL");
    if (n_cam) *n_cam = p->n_cam;
    if (n_pts) *n_pts = p->n_pts;
    if (n_obs) *n_obs = p->n_obs;
    return C2B_OK;
    C2B_API_END("problem_sizes")
}

#define NEED_UPLOADED(p, who)                                                              \
    if (!(p)) return fail(C2B_ERR_INVALID_ARGUMENT, who ": problem is NULL");              \
    if (!(p)->ws) return fail(C2B_ERR_INVALID_ARGUMENT, who ": nothing uploaded");         \
    HIP_TRY(hipSetDevice((p)->device));

int c2b_problem_download(c2b_problem *p, double *cams15, double *pts3, double *uv) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_download");
    if (cams15 && p->n_cam)
        HIP_TRY(hipMemcpyAsync(cams15, p->cam15, sizeof(double) * 15 * p->n_cam, hipMemcpyDeviceToHost, p->stream));
    if (uv && p->n_obs)
        HIP_TRY(hipMemcpyAsync(uv, p->uv, sizeof(double) * 2 * p->n_obs, hipMemcpyDeviceToHost, p->stream));
    DevBuf<double> d_p3;
    if (pts3 && p->n_pts) {
        HIP_TRY(d_p3.alloc(3 * (size_t)p->n_pts));
        int rc = c2b_points_unpad(p->pts4, p->n_pts, d_p3, p->stream);
        if (rc) return rc;
        hipError_t e = hipMemcpyAsync(pts3, d_p3, sizeof(double) * 3 * p->n_pts, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) return fail(C2B_ERR_HIP, "download points: %s", hipGetErrorString(e));
    }
    hipError_t e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return fail(C2B_ERR_HIP, "problem_download: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_download")
}

int c2b_problem_download_bal(c2b_problem *p, double *bal9) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_download_bal");
    if (!bal9) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_download_bal: bal9 is NULL");
    if (!p->n_cam) return C2B_OK;
    if (!p->bal_valid && !p->bal9_fresh) {
        // to_vec (src/baproblem.rs:189-202) of the current state
        int rc = c2b_cameras_to_bal(p->cam15, p->n_cam, p->bal9, p->stream);
        if (rc) return rc;
        p->bal9_fresh = true;
    }
    HIP_TRY(hipMemcpyAsync(bal9, p->bal9, sizeof(double) * 9 * p->n_cam, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_download_bal")
}

int c2b_problem_from_position_direction(c2b_problem *p, int64_t n_cam, const double *pos3, const double *dir9,
                                        double *cams15) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_from_position_direction: problem is NULL");
    if (n_cam < 0 || (n_cam && (!pos3 || !dir9 || !cams15)))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_from_position_direction: bad arguments");
    if (!n_cam) return C2B_OK;
    HIP_TRY(hipSetDevice(p->device));
    DevBuf<double> d_pos, d_dir, d_cam;
    int rc = C2B_OK;
    hipError_t e = d_pos.alloc(3 * (size_t)n_cam);
    if (e == hipSuccess) e = d_dir.alloc(9 * (size_t)n_cam);
    if (e == hipSuccess) e = d_cam.alloc(15 * (size_t)n_cam);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pos, pos3, sizeof(double) * 3 * n_cam, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_dir, dir9, sizeof(double) * 9 * n_cam, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) {
        rc = c2b_cameras_from_position_direction(d_pos, d_dir, n_cam, d_cam, p->stream);
        if (!rc) e = hipMemcpyAsync(cams15, d_cam, sizeof(double) * 15 * n_cam, hipMemcpyDeviceToHost, p->stream);
        hipError_t e2 = hipStreamSynchronize(p->stream);
        if (e == hipSuccess) e = e2;
    }
    if (rc) return rc;
    if (e != hipSuccess)
        return fail(hip_code(e), "problem_from_position_direction: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_from_position_direction")
}

int c2b_problem_centers(c2b_problem *p, double *centers3) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_centers");
    if (!p->n_cam) return C2B_OK;
    if (!centers3) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_centers: centers3 is NULL");
    int rc = ensure_camblk(p);
    if (rc) return rc;
    // the compact centre table: 32-byte rows, the centre in the first three doubles
    HIP_TRY(hipMemcpy2DAsync(centers3, 3 * sizeof(double), p->cen4, 4 * sizeof(double),
                             3 * sizeof(double), (size_t)p->n_cam, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_centers")
}

// row_ptr (from the camera-major cam_idx) and the tile records of the current observation list
static int ensure_rows(c2b_problem *p) {
    if (p->rows_valid || !p->n_obs) return C2B_OK;
    drop_rows(p);
    HIP_TRY(p->rows_ptr.alloc((size_t)p->n_cam + 1));
    HIP_TRY(p->rows_tiles.alloc((size_t)c2b_rows_tiles_bytes(p->n_obs)));
    hipLaunchKernelGGL(k_rows_from_sorted, dim3(blocks_for(p->n_obs + 1)), dim3(kBlock), 0, p->stream, (const uint32_t *)p->cam_idx,
                       p->n_obs, p->n_cam, p->rows_ptr);
    LAUNCH_CHECK();
    const int rc = c2b_rows_pack(p->rows_ptr, p->n_cam, p->n_obs, p->rows_tiles, p->stream);
    if (rc) return rc;
    p->rows_valid = true;
    return C2B_OK;
}

int c2b_problem_project(c2b_problem *p, double *uv_out) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_project");
    if (!p->n_obs) return C2B_OK;
    if (!uv_out) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_project: uv_out is NULL");
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    DevBuf<double> d_uv;
    HIP_TRY(d_uv.alloc(2 * (size_t)p->n_obs));
    rc = c2b_project_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->n_obs, d_uv, p->stream);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(uv_out, d_uv, sizeof(double) * 2 * p->n_obs, hipMemcpyDeviceToHost, p->stream);
    hipError_t e2 = hipStreamSynchronize(p->stream);
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(C2B_ERR_HIP, "problem_project: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return C2B_OK;
    C2B_API_END("problem_project")
}

int c2b_problem_total_reprojection_error(c2b_problem *p, double norm, double *out) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_total_reprojection_error");
    if (!out) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_error: out is NULL");
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    rc = c2b_reprojection_error_sum_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv, p->n_obs,
                                         norm, p->ws, p->scalar, p->stream);
    if (rc) return rc;
    double sum = 0.0;
    HIP_TRY(hipMemcpyAsync(&sum, p->scalar, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    *out = std::pow(sum, 1.0 / norm);          // .powf(1. / norm), src/baproblem.rs:278
    return C2B_OK;
    C2B_API_END("problem_total_reprojection_error")
}

// The same for a problem that is one SHARD (a contiguous camera range) of a larger one: the local sum, one 8-byte
// all-reduce through the communicator on the problem's stream, then .powf(1/norm) -- every rank returns the global
// error (src/baproblem.rs:265-279 over all shards).  Collective: every rank of the communicator must call it.
int c2b_problem_total_reprojection_error_sharded(c2b_problem *p, c2b_comm *comm, double norm, double *out) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_total_reprojection_error_sharded");
    if (!out || !comm) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_error_sharded: NULL argument");
    if (comm->device != p->device) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_error_sharded: communicator and problem live on different devices");
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    if (p->n_obs > 0)
        rc = c2b_reprojection_error_sum_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv, p->n_obs,
                                             norm, p->ws, p->scalar, p->stream);
    else
        HIP_TRY(hipMemsetAsync(p->scalar, 0, sizeof(double), p->stream));          // an empty shard still takes part
    if (!rc) rc = c2b_comm_all_reduce_sum_f64(comm, p->scalar, 1, p->stream);
    if (rc) return rc;
    double sum = 0.0;
    HIP_TRY(hipMemcpyAsync(&sum, p->scalar, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    *out = std::pow(sum, 1.0 / norm);
    return C2B_OK;
    C2B_API_END("problem_total_reprojection_error_sharded")
}

// Both norms run_noise prints (src/bin/city2ba.rs:283-287, 350-354) from ONE pass over the observations.
static int errors_l1_l2_impl(c2b_problem *p, c2b_comm *comm, double *l1, double *l2) {
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    if (p->n_obs > 0)
        rc = c2b_reprojection_error_sums2_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv, p->n_obs,
                                               p->ws, p->scalar, p->stream);
    else
        HIP_TRY(hipMemsetAsync(p->scalar, 0, 2 * sizeof(double), p->stream));      // an empty shard still takes part
    if (!rc && comm) rc = c2b_comm_all_reduce_sum_f64(comm, p->scalar, 2, p->stream);   // ONE 2-element all-reduce
    if (rc) return rc;
    double sums[2] = {0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(sums, p->scalar, 2 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    *l1 = std::pow(sums[0], 1.0 / 1.0);        // .powf(1. / norm), src/baproblem.rs:278
    *l2 = std::pow(sums[1], 1.0 / 2.0);
    return C2B_OK;
}

int c2b_problem_total_reprojection_errors_l1_l2(c2b_problem *p, double *l1, double *l2) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_total_reprojection_errors_l1_l2");
    if (!l1 || !l2) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_errors_l1_l2: NULL output");
    return errors_l1_l2_impl(p, nullptr, l1, l2);
    C2B_API_END("problem_total_reprojection_errors_l1_l2")
}

int c2b_problem_total_reprojection_errors_l1_l2_sharded(c2b_problem *p, c2b_comm *comm, double *l1, double *l2) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_total_reprojection_errors_l1_l2_sharded");
    if (!l1 || !l2 || !comm) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_errors_l1_l2_sharded: NULL argument");
    if (comm->device != p->device) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_errors_l1_l2_sharded: communicator and problem live on different devices");
    return errors_l1_l2_impl(p, comm, l1, l2);
    C2B_API_END("problem_total_reprojection_errors_l1_l2_sharded")
}

// the point-major transpose of the current observation list (after ensure_rows; pt_idx does not change without drop_rows)
static int ensure_transpose(c2b_problem *p) {
    if (p->nt_ptr) return C2B_OK;
    DevBuf<uint64_t> ptr;
    DevBuf<uint32_t> obs, cam;
    DevBuf<char> temp;
    const size_t n_obs = (size_t)p->n_obs;
    hipError_t e = ptr.alloc((size_t)p->n_pts + 1);
    if (e == hipSuccess) e = obs.alloc(n_obs);
    if (e == hipSuccess) e = cam.alloc(n_obs);
    if (e == hipSuccess) e = temp.alloc((size_t)c2b_normal_transpose_temp_bytes(p->n_obs, p->n_pts));
    if (e != hipSuccess) return fail(hip_code(e), "normal_equations: transpose allocation: %s", hipGetErrorString(e));
    int rc = c2b_normal_transpose(p->rows_ptr, p->n_cam, p->pt_idx, p->n_obs, p->n_pts, ptr, obs, cam, temp, p->stream);
    if (!rc) {
        e = hipStreamSynchronize(p->stream);                 // temp is freed below
        if (e != hipSuccess) rc = fail(C2B_ERR_HIP, "normal_equations: transpose: %s", hipGetErrorString(e));
    }
    temp.reset();
    if (rc) return rc;
    p->nt_ptr = std::move(ptr); p->nt_obs = std::move(obs); p->nt_cam = std::move(cam);
    return C2B_OK;
}

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

// sum over the observations of rho(s) (weighted_sq: of w s) under the problem's loss into out[0] (device), asynchronous;
// one partial per workgroup of 256 observations: the workspace holds one per 4 tiles of 64 (block_part_slots)
static int robust_sum(c2b_problem *p, bool weighted_sq, double *out) {
    const int rc = ensure_camblk(p);
    if (rc) return rc;
    static_assert(kNormBlock == 256, "k_robust_cost's partials are sized by block_part_slots");
    const unsigned nb = blocks_for(p->n_obs, kNormBlock);
    double *part = reinterpret_cast<double *>(p->ws.ptr) + kWsBlockPart;
    const double4 *p4 = reinterpret_cast<const double4 *>(p->pts4.ptr);
    const double2 *uv = reinterpret_cast<const double2 *>(p->uv.ptr);
    const double a2 = p->loss_scale * p->loss_scale;
    if (weighted_sq)
        hipLaunchKernelGGL(k_robust_cost<true>, dim3(nb), dim3(kNormBlock), 0, p->stream, p->camblk, p4, (const uint32_t *)p->cam_idx,
                           (const uint64_t *)nullptr, 0, (const uint32_t *)p->pt_idx, uv, p->n_obs, p->loss_kind, a2, part);
    else
        hipLaunchKernelGGL(k_robust_cost<false>, dim3(nb), dim3(kNormBlock), 0, p->stream, p->camblk, p4, (const uint32_t *)p->cam_idx,
                           (const uint64_t *)nullptr, 0, (const uint32_t *)p->pt_idx, uv, p->n_obs, p->loss_kind, a2, part);
    hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, p->stream, (const double *)part, (int)nb, out);
    HIP_TRY(launch_error());
    return C2B_OK;
}

int c2b_problem_robust_cost(c2b_problem *p, double *cost) {
    C2B_API_BEGIN
    if (!p || !cost) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_robust_cost: NULL argument");
    NEED_UPLOADED(p, "problem_robust_cost");
    double s = 0.0;
    if (p->n_obs) {
        const int rc = robust_sum(p, false, p->scalar);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(&s, p->scalar, sizeof(double), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    *cost = s;
    return C2B_OK;
    C2B_API_END("problem_robust_cost")
}

int c2b_problem_normal_equations(c2b_problem *p, double *U, double *gc, double *V, double *gp, double *sum_sq) {
    C2B_API_BEGIN
    if (!p) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_normal_equations: problem is NULL");
    if (!U != !gc || !V != !gp) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_normal_equations: U / gc and V / gp go in pairs (both or neither)");
    for (const void *q : {(const void *)U, (const void *)gc, (const void *)V, (const void *)gp, (const void *)sum_sq})
        if (reinterpret_cast<uintptr_t>(q) & 7) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_normal_equations: misaligned pointer");
    NEED_UPLOADED(p, "problem_normal_equations");
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    const bool want_sum = sum_sq != nullptr;
    if (U) {
        rc = normal_cameras_rows_impl(p->camblk, p->pts4, p->n_obs ? p->rows_ptr : nullptr, p->n_obs ? p->n_cam : 0, p->pt_idx, p->uv,
                                      p->n_obs, U, gc, want_sum ? p->ws : nullptr, want_sum ? p->scalar : nullptr, p->loss_kind,
                                      p->loss_scale, p->stream);
        if (!rc && !p->n_obs && p->n_cam) {                   // no list: every camera's block is empty
            HIP_TRY(hipMemsetAsync(U, 0, sizeof(double) * 81 * (size_t)p->n_cam, p->stream));
            HIP_TRY(hipMemsetAsync(gc, 0, sizeof(double) * 9 * (size_t)p->n_cam, p->stream));
        }
        if (!rc && p->n_obs) rc = constant_cameras(p, U, 0.0, gc);
    } else if (want_sum && p->loss_kind != kLossSquared && p->n_obs) {
        rc = robust_sum(p, true, p->scalar);                 // the weighted sum of squares without the blocks
    } else if (want_sum) {
        rc = p->n_obs ? c2b_reprojection_error_sum_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv,
                                                        p->n_obs, 2.0, p->ws, p->scalar, p->stream)
                      : (hipMemsetAsync(p->scalar, 0, sizeof(double), p->stream) == hipSuccess ? C2B_OK
                                                                                             : fail(C2B_ERR_HIP, "problem_normal_equations: memset"));
    }
    if (rc) return rc;
    if (V && p->n_pts) {
        if (p->n_obs) {
            rc = ensure_transpose(p);
            if (!rc) rc = normal_points_rows_impl(p->camblk, p->pts4, p->n_pts, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, V, gp, p->loss_kind,
                                                  p->loss_scale, p->stream);
            if (!rc) rc = constant_points(p, V, 0.0, gp);
            if (rc) return rc;
        } else {
            HIP_TRY(hipMemsetAsync(V, 0, sizeof(double) * 9 * (size_t)p->n_pts, p->stream));
            HIP_TRY(hipMemsetAsync(gp, 0, sizeof(double) * 3 * (size_t)p->n_pts, p->stream));
        }
    }
    double s = 0.0;
    if (want_sum) HIP_TRY(hipMemcpyAsync(&s, p->scalar, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (want_sum) *sum_sq = s;
    return C2B_OK;
    C2B_API_END("problem_normal_equations")
}

// ---- damped Gauss-Newton step (schur_kernels.hpp) ------------------------------------------------------------------
// c2b_problem::sv, carved: U [n_cam][81], gc [n_cam][9], V [n_pts][9], gp [n_pts][3], Lf [n_cam][45], t [n_pts][3],
// r / z / p / q [n_cam][9], two partial arrays [n_part], the device scalars [kScSlots]; under the Schur-Jacobi
// preconditioner its blocks M [n_cam][81] after them (the rest lies where it lies without)
struct SolveBufs {
    double *U, *gc, *V, *gp, *Lf, *t, *r, *z, *pv, *q, *pa, *pb, *sc, *M;
    int64_t n_part;
};

static int64_t solve_parts(const c2b_problem *p) {
    const int64_t a = (int64_t)schur_cameras_grid(p->n_cam) * (kNormBlock / 64);
    return std::max<int64_t>({a, (int64_t)blocks_for(p->n_cam, kSchurBlock), (int64_t)blocks_for(p->n_obs, kSchurBlock), 1});
}

static int64_t solve_doubles(const c2b_problem *p) {
    return p->n_cam * (81 + 9 + kCholPacked + 4 * 9) + p->n_pts * (9 + 3 + 3) + 2 * solve_parts(p) + kScSlots +
           (p->precond_kind == C2B_PRECOND_SCHUR_JACOBI ? 81 * p->n_cam : 0);
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
    return b;
}

static int ensure_solver(c2b_problem *p) {
    const int64_t n = solve_doubles(p);
    if (p->sv && p->sv_doubles >= n) return C2B_OK;
    p->sv_doubles = 0;
    const hipError_t e = p->sv.alloc((size_t)n);                  // (the smaller one is freed first)
    if (e != hipSuccess) return fail(hip_code(e), "problem_solve_step: allocation: %s", hipGetErrorString(e));
    p->sv_doubles = n;
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
    if (!rc) rc = ensure_solver(p);
    if (rc) return rc;
    const SolveBufs B = solve_bufs(p);
    const double4 *p4 = reinterpret_cast<const double4 *>(p->pts4.ptr);
    const double2 *uv = reinterpret_cast<const double2 *>(p->uv.ptr);
    const unsigned cgrid = schur_cameras_grid(nc), nbc = blocks_for(nc, kSchurBlock), nbo = blocks_for(no, kSchurBlock);
    const int n_cpart = (int)(cgrid * (kNormBlock / 64));
    const int kind = p->loss_kind;                           // 0: every launch below is the squared-loss kernel it always was
    const double a2 = p->loss_scale * p->loss_scale;
    auto points = [&](const double *x, const double *h, double *t, bool neg) {
        with_loss(kind, a2, [&](auto... loss) {
            if (neg)
                hipLaunchKernelGGL((k_schur_points<true, decltype(loss)...>), dim3(blocks_for(np, kSchurBlock)), dim3(kSchurBlock), 0, st,
                                   p->camblk, p4, np, p->nt_ptr, p->nt_obs, p->nt_cam, uv, B.V, lambda, x, h, t, loss...);
            else
                hipLaunchKernelGGL((k_schur_points<false, decltype(loss)...>), dim3(blocks_for(np, kSchurBlock)), dim3(kSchurBlock), 0, st,
                                   p->camblk, p4, np, p->nt_ptr, p->nt_obs, p->nt_cam, uv, B.V, lambda, x, h, t, loss...);
        });
        if (p->pmask) (void)constant_points(p, nullptr, 0.0, t);        // t = 0 for the constant points (fetch sees a launch error)
    };
    auto mask_y = [&](double *y) {                           // after a camera pass: y's constant entries to 0
        if (p->cmask) (void)constant_cameras(p, nullptr, 0.0, y);
    };
    double h[kScSlots];
    auto fetch = [&](int slots) -> int {                     // the first `slots` scalars to the host, after all queued work
        HIP_TRY(launch_error());
        HIP_TRY(hipMemcpyAsync(h, B.sc, sizeof(double) * slots, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return C2B_OK;
    };

    // U, gc, V, gp; the preconditioner; b = -gc + W V_l^-1 gp into r
    rc = normal_cameras_rows_impl(p->camblk, p->pts4, p->rows_ptr, nc, p->pt_idx, p->uv, no, B.U, B.gc, nullptr, nullptr, kind,
                                  p->loss_scale, st);
    if (!rc) rc = normal_points_rows_impl(p->camblk, p->pts4, np, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, B.V, B.gp, kind, p->loss_scale, st);
    if (rc) return rc;
    const bool schur_jacobi = p->precond_kind == C2B_PRECOND_SCHUR_JACOBI;
    // constant parameters: from here on U, gc, V, gp are those of J~.  k_schur_jacobi first sees the constant
    // points' V as kConstPointV, under which their observations add Jc^T Jc as they do with Jp = 0
    rc = constant_cameras(p, B.U, 0.0, B.gc);
    if (!rc) rc = constant_points(p, B.V, schur_jacobi ? kConstPointV : 0.0, B.gp);
    if (rc) return rc;
    if (schur_jacobi) {                                      // M from U's diagonal and V, its factors, the fallbacks' count
        rc = schur_jacobi_rows_impl(p->camblk, p->pts4, p->rows_ptr, nc, p->pt_idx, p->uv, no, B.U, B.V, lambda, B.M, kind, p->loss_scale, st);
        if (!rc) rc = constant_cameras(p, B.M, lambda * 1e-6, nullptr);
        if (!rc) rc = constant_points(p, B.V, 0.0, nullptr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_schur_factor_blocks, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.M, (const double *)B.U,
                           lambda, B.Lf, B.pa);
        hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pa, (int)nbc, B.sc + kScFallback);
    } else {
        hipLaunchKernelGGL(k_schur_factor, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.U, lambda, B.Lf);
    }
    points(nullptr, B.gp, B.t, false);
    with_loss(kind, a2, [&](auto... loss) {
        hipLaunchKernelGGL((k_schur_cameras<kSchurRhs, decltype(loss)...>), dim3(cgrid), dim3(kNormBlock), 0, st, p->camblk, p4, p->rows_ptr,
                           (int)nc, p->pt_idx, uv, (const double *)B.U, lambda, (const double *)nullptr, (const double *)B.gc,
                           (const double *)B.t, B.r, (double *)nullptr, loss...);
    });
    mask_y(B.r);
    hipLaunchKernelGGL(k_pcg_update<true>, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.Lf, (const double *)B.sc, 0, dc,
                       B.r, B.pv, (const double *)nullptr, B.z, B.pa, B.pb);
    hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pa, (int)nbc, B.sc + kScRr);
    hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pb, (int)nbc, B.sc + kScRz0);
    if ((rc = fetch(kScRz1 + 1))) return rc;

    // PCG from x = 0 (x is dc)
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
            points(B.pv, nullptr, B.t, false);
            with_loss(kind, a2, [&](auto... loss) {
                hipLaunchKernelGGL((k_schur_cameras<kSchurDot, decltype(loss)...>), dim3(cgrid), dim3(kNormBlock), 0, st, p->camblk, p4,
                                   p->rows_ptr, (int)nc, p->pt_idx, uv, (const double *)B.U, lambda, (const double *)B.pv,
                                   (const double *)nullptr, (const double *)B.t, B.q, B.pa, loss...);
            });
            mask_y(B.q);                                     // p's constant entries are 0: the p.q partials need no correction
            hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pa, n_cpart, B.sc + kScPq);
            hipLaunchKernelGGL(k_pcg_update<false>, dim3(nbc), dim3(kSchurBlock), 0, st, nc, (const double *)B.Lf, (const double *)B.sc,
                               cur, dc, B.r, B.pv, (const double *)B.q, B.z, B.pa, B.pb);
            hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pa, (int)nbc, B.sc + kScRr);
            hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pb, (int)nbc, B.sc + nxt);
            if ((rc = fetch(kScRz1 + 1))) return rc;
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

    // dp = -V_l^-1 (gp + W^T dc); then |r|^2 and the model decrease from J, per observation
    points(dc, B.gp, dp, true);
    with_loss(kind, a2, [&](auto... loss) {
        hipLaunchKernelGGL(k_schur_model<decltype(loss)...>, dim3(nbo), dim3(kSchurBlock), 0, st, p->camblk, p4, (const uint32_t *)p->cam_idx,
                           (const uint32_t *)p->pt_idx, uv, no, (const double *)dc, (const double *)dp, B.pa, B.pb, loss...);
    });
    hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pa, (int)nbo, B.sc + kScSumSq);
    hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)B.pb, (int)nbo, B.sc + kScModel);
    if ((rc = fetch(schur_jacobi ? kScFallback + 1 : kScModel + 1))) return rc;
    if (schur_jacobi) p->precond_fallbacks = (int64_t)h[kScFallback];
    out.iterations = it;
    out.status = status;
    out.rel_residual = bb == 0.0 ? 0.0 : rnorm / bnorm;
    out.sum_sq = h[kScSumSq];
    out.model_decrease = h[kScModel];
    if (!std::isfinite(out.sum_sq) || !std::isfinite(out.model_decrease) || !std::isfinite(out.rel_residual)) {
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

int c2b_problem_apply_step(c2b_problem *p, const double *dc, const double *dp) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_apply_step");
    if (!aligned8(dc) || !aligned8(dp)) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_apply_step: misaligned pointer");
    const int64_t nc = p->n_cam, np = p->n_pts;
    hipStream_t st = p->stream;
    if (nc) {
        if (!p->bal_valid && !p->bal9_fresh) {               // state mode: the columns of dc refer to to_vec(cam15)
            const int rc = c2b_cameras_to_bal(p->cam15, nc, p->bal9, st);
            if (rc) return rc;
        }
        if (dc && p->cmask)                                  // a constant entry keeps its bits
            hipLaunchKernelGGL(k_add_free, dim3(blocks_for(9 * nc, kSchurBlock)), dim3(kSchurBlock), 0, st, 9 * nc, dc,
                               (const uint16_t *)p->cmask, p->bal9);
        else if (dc) hipLaunchKernelGGL(k_add_f64, dim3(blocks_for(9 * nc, kSchurBlock)), dim3(kSchurBlock), 0, st, 9 * nc, dc, p->bal9);
        LAUNCH_CHECK();
        const int rc = c2b_cameras_from_bal(p->bal9, nc, p->cam15, st);
        if (rc) return rc;
    }
    if (dp && np) {
        if (p->pmask)
            hipLaunchKernelGGL(k_points_add_free, dim3(blocks_for(np, kSchurBlock)), dim3(kSchurBlock), 0, st, np, dp,
                               (const uint8_t *)p->pmask, reinterpret_cast<double4 *>(p->pts4.ptr));
        else
            hipLaunchKernelGGL(k_points_add, dim3(blocks_for(np, kSchurBlock)), dim3(kSchurBlock), 0, st, np, dp, reinterpret_cast<double4 *>(p->pts4.ptr));
        LAUNCH_CHECK();
    }
    cameras_mutated(p);                                      // every cache of the cameras; then bal9 is the truth
    p->bal_valid = true;
    HIP_TRY(hipStreamSynchronize(st));
    return C2B_OK;
    C2B_API_END("problem_apply_step")
}

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
    int64_t got[kTriKinds] = {0, 0, 0, 0, 0};
    if (!p->n_obs) {                                         // no observation: every point has too few, nothing is read or written
        got[kTriTooFew] = np;
        if (status && np) std::fill(status, status + np, (uint8_t)kTriTooFew);
        if (counts) std::copy(got, got + kTriKinds, counts);
        return C2B_OK;
    }
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (!rc) rc = ensure_transpose(p);
    if (rc) return rc;
    DevBuf<uint8_t> d_status;
    DevBuf<int64_t> d_counts;
    hipError_t e = d_status.alloc((size_t)np);
    if (e == hipSuccess) e = d_counts.alloc(kTriKinds);
    if (e != hipSuccess) return fail(hip_code(e), "problem_triangulate_points: allocation: %s", hipGetErrorString(e));
    rc = c2b_triangulate_rows(p->camblk, p->pts4, np, p->nt_ptr, p->nt_obs, p->nt_cam, p->uv, min_angle, p->pmask, d_status, d_counts, p->stream);
    if (!rc && status) e = hipMemcpyAsync(status, d_status, (size_t)np, hipMemcpyDeviceToHost, p->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(got, d_counts, sizeof(got), hipMemcpyDeviceToHost, p->stream);
    const hipError_t es = hipStreamSynchronize(p->stream);   // the temporaries are freed below
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(C2B_ERR_HIP, "problem_triangulate_points: %s", hipGetErrorString(e != hipSuccess ? e : es));
    if (counts) std::copy(got, got + kTriKinds, counts);
    return C2B_OK;
    C2B_API_END("problem_triangulate_points")
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
    if (p->n_cam) {
        HIP_TRY(hipMemcpyAsync(p->bal9, p->ck_bal9, sizeof(double) * 9 * (size_t)p->n_cam, hipMemcpyDeviceToDevice, st));
        const int rc = c2b_cameras_from_bal(p->bal9, p->n_cam, p->cam15, st);      // the kernel that built cam15: the same bits
        if (rc) return rc;
    }
    if (p->n_pts) HIP_TRY(hipMemcpyAsync(p->pts4, p->ck_pts4, sizeof(double) * 4 * (size_t)p->n_pts, hipMemcpyDeviceToDevice, st));
    cameras_mutated(p);                                      // the cameras' caches only: rows, transpose, solve buffers, masks stay
    p->bal_valid = true;
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
// uses the first 2 x grid of them after those were summed), the device scalars: the four sums, then the two maxima
struct LmBufs {
    double *dc, *dp, *part, *sc;
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
    return b;
}

static int ensure_lm(c2b_problem *p) {
    if (p->lm) return C2B_OK;                                // (dropped whenever a count changes)
    const int64_t n = 9 * p->n_cam + 3 * p->n_pts + (int64_t)kLmSums * lm_grid(std::max<int64_t>(9 * p->n_cam, 3 * p->n_pts)) + kLmScSlots;
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
static int lm_cost(c2b_problem *p, double *cost) {
    if (p->loss_kind != kLossSquared) return c2b_problem_robust_cost(p, cost);
    double e = 0.0;
    const int rc = c2b_problem_total_reprojection_error(p, 2.0, &e);
    if (rc) return rc;
    *cost = libm_pow(e, 2.0);
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
            hipLaunchKernelGGL(k_normal_sum, dim3(1), dim3(256), 0, st, (const double *)(L.part + (int64_t)k * L.grid), (int)L.grid, L.sc + k);
        if (have_g) {
            const SolveBufs B = solve_bufs(p);
            hipLaunchKernelGGL(k_lm_gradient_max, dim3(L.grid), dim3(kSchurBlock), 0, st, 9 * nc, 3 * np, (const double *)B.gc,
                               (const double *)B.gp, L.part);
            hipLaunchKernelGGL(k_lm_max_fold, dim3(1), dim3(kSchurBlock), 0, st, (const double *)L.part, (int)L.grid, L.sc + kLmScGradCam);
        }
        HIP_TRY(launch_error());
        double h[kLmScSlots] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        HIP_TRY(hipMemcpyAsync(h, L.sc, sizeof(double) * (have_g ? kLmScGradPts + 1 : kLmSums), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
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
    const int rc = lm_loop(p, *opt, history, summary);
    p->ck_valid = false;                                     // the checkpoint was the loop's
    return rc;
    C2B_API_END("problem_levenberg_marquardt")
}

// Results leave in chunks of kJacChunk observations through a ring of kJacSlots device buffers: the kernel of chunk
// k + 1 is queued before the copies of chunk k start, copies run on their own stream, so PCIe and the kernel overlap
// and the device never holds more than the ring (159 MB) whatever the problem size.  Host buffers from
// c2b_host_alloc (pinned) take the copies at link speed; ordinary pageable memory works too, at the runtime's staged
// rate.  The ring, the copy stream and the events are created on first use and live as long as the problem.
int c2b_problem_residual_jacobian(c2b_problem *p, double *r, double *Jc, double *Jp) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_residual_jacobian");
    if (!p->n_obs) return C2B_OK;
    if (!r || !Jc || !Jp) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_residual_jacobian: NULL output");
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    constexpr int kSlots = c2b_problem::kJacSlots;
    constexpr int64_t kChunk = c2b_problem::kJacChunk;
    if (!p->jac_ring) HIP_TRY(p->jac_ring.alloc(26 * (size_t)kChunk * kSlots));
    if (!p->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
    for (int k = 0; k < kSlots; ++k) {
        if (!p->ev_done[k]) HIP_TRY(hipEventCreateWithFlags(&p->ev_done[k], hipEventDisableTiming));
        if (!p->ev_free[k]) HIP_TRY(hipEventCreateWithFlags(&p->ev_free[k], hipEventDisableTiming));
    }
    const int64_t n = p->n_obs, n_chunks = (n + kChunk - 1) / kChunk;
    auto slot_r = [&](int s) { return p->jac_ring + (size_t)s * 26 * kChunk; };
    auto slot_Jc = [&](int s) { return slot_r(s) + 2 * kChunk; };
    auto slot_Jp = [&](int s) { return slot_r(s) + 20 * kChunk; };
    auto launch = [&](int64_t k) -> int {
        const int s = (int)(k % kSlots);
        const int64_t o0 = k * kChunk, m = (n - o0 < kChunk) ? n - o0 : kChunk;
        if (k >= kSlots) { HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_free[s], 0)); }      // its previous copies are out
        // kJacChunk is a multiple of 64: every chunk starts on a tile record
        // (n_pts = 0: a chunk's working set is small and this path is bound by the PCIe copies; loads stay cached)
        int rc2 = c2b_residual_jacobian_rows(p->camblk, p->pts4, 0, p->rows_ptr, p->n_cam, (const char *)p->rows_tiles + (o0 >> 6) * 16, o0,
                                             p->pt_idx + o0, p->uv + 2 * o0, m, slot_r(s), slot_Jc(s), slot_Jp(s), 2.0, nullptr,
                                             nullptr, p->stream);
        if (rc2) return rc2;
        HIP_TRY(hipEventRecord(p->ev_done[s], p->stream));
        return C2B_OK;
    };
    hipError_t e = hipSuccess;
    rc = launch(0);
    for (int64_t k = 0; k < n_chunks && !rc && e == hipSuccess; ++k) {
        if (k + 1 < n_chunks) rc = launch(k + 1);            // queued BEFORE chunk k's copies: they overlap
        if (rc) break;
        const int s = (int)(k % kSlots);
        const int64_t o0 = k * kChunk, m = (n - o0 < kChunk) ? n - o0 : kChunk;
        e = hipStreamWaitEvent(p->copy_stream, p->ev_done[s], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(r + 2 * o0, slot_r(s), sizeof(double) * 2 * m, hipMemcpyDeviceToHost, p->copy_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(Jc + 18 * o0, slot_Jc(s), sizeof(double) * 18 * m, hipMemcpyDeviceToHost, p->copy_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(Jp + 6 * o0, slot_Jp(s), sizeof(double) * 6 * m, hipMemcpyDeviceToHost, p->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(p->ev_free[s], p->copy_stream);
    }
    const hipError_t e1 = hipStreamSynchronize(p->copy_stream), e2 = hipStreamSynchronize(p->stream);
    if (e == hipSuccess) e = e1 != hipSuccess ? e1 : e2;
    if (rc) return rc;
    if (e != hipSuccess) return fail(hip_code(e), "problem_residual_jacobian: %s", hipGetErrorString(e));
    return C2B_OK;
    C2B_API_END("problem_residual_jacobian")
}

// The same launch with the results left ON THE DEVICE, in output arrays placed for streaming stores: what a
// BAProblem-level caller that consumes the Jacobian on the GPU (a solver's normal equations) calls in its loop.  The
// whole list in ONE launch -- residual, both blocks and the folded sum of squared residuals -- at the Level-0 headline
// rate; nothing crosses PCIe but the 8-byte sum.  *outputs == NULL: a set is allocated by c2b_jacobian_outputs_alloc
// (max_attempts placements tried, as there) and handed to the caller, who passes it back on later calls (it is reused as
// long as the observation count matches) and frees it with c2b_jacobian_outputs_free.
int c2b_problem_residual_jacobian_device(c2b_problem *p, int max_attempts, c2b_jacobian_outputs **outputs, double *sum_sq) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_residual_jacobian_device");
    if (!outputs) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_residual_jacobian_device: outputs is NULL");
    if (*outputs && ((*outputs)->n_obs != p->n_obs || (*outputs)->device != p->device))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_residual_jacobian_device: the output set holds %lld observations on device %d, the problem %lld on device %d",
                    (long long)(*outputs)->n_obs, (*outputs)->device, (long long)p->n_obs, p->device);
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    const bool mine = *outputs == nullptr;
    if (mine) {
        rc = c2b_jacobian_outputs_alloc(p->n_obs, max_attempts, 0.0, p->stream, outputs);
        if (rc) return rc;
    }
    c2b_jacobian_outputs *h = *outputs;
    // into the placed set: the workgroup shape follows the store rate measured for it
    rc = c2b_residual_jacobian_rows_placed(p->camblk, p->pts4, p->n_pts, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv, p->n_obs,
                                           h, 2.0, p->ws, p->scalar, p->stream);
    double sum = 0.0;
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(&sum, p->scalar, sizeof(double), hipMemcpyDeviceToHost, p->stream);
    const hipError_t e2 = hipStreamSynchronize(p->stream);
    if (rc || e != hipSuccess || e2 != hipSuccess) {
        if (mine) { c2b_jacobian_outputs_free(h); *outputs = nullptr; }
        if (rc) return rc;
        return fail(C2B_ERR_HIP, "problem_residual_jacobian_device: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    if (sum_sq) *sum_sq = sum;
    return C2B_OK;
    C2B_API_END("problem_residual_jacobian_device")
}

int c2b_host_alloc(void **ptr, int64_t bytes) {
    C2B_API_BEGIN
    if (!ptr || bytes < 0) return fail(C2B_ERR_INVALID_ARGUMENT, "host_alloc: bad arguments");
    *ptr = nullptr;
    if (!bytes) return C2B_OK;
    HIP_TRY(hipHostMalloc(ptr, (size_t)bytes, hipHostMallocDefault));
    return C2B_OK;
    C2B_API_END("host_alloc")
}

void c2b_host_free(void *ptr) {
    if (ptr) (void)hipHostFree(ptr);
}

static int compute_stats(c2b_problem *p) {
    // The statistics read the centre table only.  When the camera table is stale because the in-memory cameras MOVED (drift, noise:
    // bal_valid is off then), the centres alone are derived from the state -- k_cameras_centers, the bits k_cameras_prepare would write
    // -- instead of the whole table: run_noise's add_noise asks for std() right after add_drift (src/noise.rs:133) and its entity
    // pass invalidates a camera table again before any pass reads it (38.6 -> ~20 us of that flow, r06).  camblk stays stale.
    if (!p->blk_valid && !p->bal_valid && p->n_cam > 0) {
        hipLaunchKernelGGL(k_cameras_centers, dim3(blocks_for(p->n_cam)), dim3(kBlock), 0, p->stream, p->cam15, p->n_cam, p->cen4);
        LAUNCH_CHECK();
    } else {
        int rc = ensure_camblk(p);
        if (rc) return rc;
    }
    return c2b_stats(p->camblk, p->cen4, p->n_cam, p->pts4, p->n_pts, p->ws, p->stats, p->stream);
}

int c2b_problem_stats(c2b_problem *p, double *stats) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_stats");
    if (!stats) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_stats: stats is NULL");
    int rc = compute_stats(p);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stats, p->stats, sizeof(double) * C2B_STATS_DOUBLES, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_stats")
}

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

// exclusive scan of n 0/1 flags into pos; *total_host = number of set flags.  Synchronises.
hipError_t scan_flags(hipStream_t st, const uint32_t *flags, int64_t n, uint32_t *pos, uint32_t *tile_scratch, uint32_t *d_total,
                      uint32_t *total_host) {
    const int64_t tiles = (n + kScanTile - 1) / kScanTile;
    if (n > 0) hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)tiles), dim3(kScanBlock), 0, st, flags, n, pos, tile_scratch);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(kScanBlock), 0, st, tile_scratch, tiles, d_total);
    if (n > 0) hipLaunchKernelGGL(k_scan_add, dim3((unsigned)tiles), dim3(kScanBlock), 0, st, pos, n, (const uint32_t *)tile_scratch);
    hipError_t e = launch_error();
    if (e == hipSuccess) e = hipMemcpyAsync(total_host, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

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
        each(tiles, (size_t)(big0 / kScanTile + 2)); each(best, (size_t)1); each(total, (size_t)1); each(deg, (size_t)nc0); each(cnt, (size_t)np0);
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
    DevBuf<char> n_ws;
    if (e == hipSuccess) e = n_cam15.alloc(15 * (size_t)nc);
    if (e == hipSuccess) e = n_bal9.alloc(9 * (size_t)nc);
    if (e == hipSuccess) e = n_camblk.alloc((size_t)cam_table_doubles(nc));
    if (e == hipSuccess) e = n_cen4.alloc(4 * (size_t)nc);
    if (e == hipSuccess) e = n_pts4.alloc(4 * (size_t)np);
    if (e == hipSuccess) e = n_uv.alloc(2 * (size_t)no);
    if (e == hipSuccess) e = n_ws.alloc((size_t)c2b_workspace_bytes(no));
    if (e == hipSuccess && c2b_workspace_init(n_ws, st) != C2B_OK) e = hipErrorUnknown;
    if (e == hipSuccess) {
        auto gather = [&](const double *in, const uint32_t *orig, int64_t n, int width, double *out) {
            if (n) hipLaunchKernelGGL(k_gather_rows, dim3(blocks_of(n * width, kBlock)), dim3(kBlock), 0, st, in, orig, n, width, out);
        };
        gather(p->cam15, corig[cur], nc, 15, n_cam15);
        if (p->bal_valid) gather(p->bal9, corig[cur], nc, 9, n_bal9);
        gather(p->pts4, porig[cur], np, 4, n_pts4);
        gather(p->uv, eorig[cur], no, 2, n_uv);
        e = launch_error();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(hip_code(e), "problem_cull: %s", hipGetErrorString(e));
    }
    p->cam15 = std::move(n_cam15); p->bal9 = std::move(n_bal9); p->camblk = std::move(n_camblk); p->cen4 = std::move(n_cen4);
    p->pts4 = std::move(n_pts4); p->uv = std::move(n_uv);
    p->cam_idx = std::move(cam[cur]); p->pt_idx = std::move(pt[cur]); p->ws = std::move(n_ws);
    drop_rows(p);
    drop_constant(p);                                         // the survivors are renumbered
    drop_lm_state(p);
    p->n_cam = nc; p->n_pts = np; p->n_obs = no;
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
    DevBuf<uint32_t> cam_idx;
    DevBuf<char> ws;
    hipError_t e = cam_idx.alloc((size_t)n);
    if (e == hipSuccess) e = ws.alloc((size_t)c2b_workspace_bytes(n));
    if (e != hipSuccess) return fail(hip_code(e), "problem_adopt_visibility: %s", hipGetErrorString(e));
    int rc = c2b_expand_rows(p->dense_row, p->n_cam, 0, n, cam_idx, p->stream);
    if (!rc) rc = c2b_workspace_init(ws, p->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->uv = std::move(p->dense_uv); p->cam_idx = std::move(cam_idx); p->pt_idx = std::move(p->dense_pt); p->ws = std::move(ws);
    p->n_obs = n;
    free_dense(p);                                            // (the row pointer; the lists were moved out)
    drop_rows(p);
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
    if (n_cam) hipLaunchKernelGGL(k_keep_row_counts, dim3(row_blocks), dim3(256), 0, p->stream, d_row_old, d_keep, n_cam, d_tot);
    hipLaunchKernelGGL(k_dense_cam_scan, dim3(1), dim3(256), 0, p->stream, (const uint64_t *)d_tot, n_cam, row_new);
    e = hipMemcpyAsync(row_ptr_host, row_new, sizeof(uint64_t) * (size_t)(n_cam + 1), hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return e;
    *w = (int64_t)row_ptr_host[n_cam];
    if (*w == stop_at) return hipSuccess;
    e = pt_new.alloc((size_t)*w);
    if (e == hipSuccess) e = uv_new.alloc(2 * (size_t)*w);
    if (e == hipSuccess && n_cam) {
        hipLaunchKernelGGL(k_keep_row_scatter, dim3(row_blocks), dim3(256), 0, p->stream, d_row_old, (const uint64_t *)row_new, d_keep,
                           d_pt, reinterpret_cast<const double2 *>(d_uv), n_cam, pt_new, reinterpret_cast<double2 *>(uv_new.ptr));
        e = launch_error();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    return e;
}

// The outlier filter: the residual predicate over the resident list, a stable compaction of (pt_idx, uv) by its
// mask, cam_idx from the new row pointer, a workspace for the new count -- swapped in only once the stream has synchronised
// without error, as cull_impl does.  The entities do not move: cameras, points, both counts, the masks, the loss, the
// preconditioner, the checkpoint and the LM scratch stay; what was derived from the list (drop_rows) goes.
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
    const int64_t n_cam = p->n_cam, n_old = p->n_obs;
    DevBuf<uint8_t> keep;
    DevBuf<uint64_t> row_new;
    DevBuf<uint32_t> pt_new, cam_new;
    DevBuf<double> uv_new;
    DevBuf<char> ws_new;
    std::vector<uint64_t> row_host((size_t)n_cam + 1);
    int64_t w = 0;
    hipError_t e = keep.alloc((size_t)n_old);
    if (e != hipSuccess) return fail(hip_code(e), "problem_filter_observations: %s", hipGetErrorString(e));
    rc = c2b_residual_keep_rows(p->camblk, p->pts4, p->rows_ptr, n_cam, p->rows_tiles, p->pt_idx, p->uv, n_old, max_error, flags, keep, p->stream);
    if (!rc) e = compact_rows_on_device(p, p->rows_ptr, keep, p->pt_idx, p->uv, n_cam, row_host.data(), row_new, pt_new, uv_new, &w, n_old);
    if (!rc && e == hipSuccess && w == n_old) return C2B_OK;       // nothing removed: nothing changes, no cache is dropped
    if (!rc && e == hipSuccess) e = cam_new.alloc((size_t)w);
    if (!rc && e == hipSuccess) e = ws_new.alloc((size_t)c2b_workspace_bytes(w));
    if (!rc && e == hipSuccess) rc = c2b_expand_rows(row_new, n_cam, 0, w, cam_new, p->stream);
    if (!rc && e == hipSuccess) rc = c2b_workspace_init(ws_new, p->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (rc || e != hipSuccess) {
        (void)hipStreamSynchronize(p->stream);
        return rc ? rc : fail(hip_code(e), "problem_filter_observations: %s", hipGetErrorString(e));
    }
    p->uv = std::move(uv_new); p->pt_idx = std::move(pt_new); p->cam_idx = std::move(cam_new); p->ws = std::move(ws_new);
    p->n_obs = w;
    drop_rows(p);
    if (n_removed) *n_removed = n_old - w;
    return C2B_OK;
    C2B_API_END("problem_filter_observations")
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
    // extent of cameras and points -> the cell grid.  Cells are a hair wider than max_dist so that rounding in the cell
    // arithmetic can never separate a camera from a point within max_dist by more than one cell.
    double stats[C2B_STATS_DOUBLES];
    rc = compute_stats(p);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stats, p->stats, sizeof stats, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    CellGrid g;
    g.x0 = stats[6]; g.z0 = stats[8];
    const double ex = stats[9] - stats[6], ez = stats[11] - stats[8];
    double cs = (max_dist > 0.0 ? max_dist : 1.0) * (1.0 + 0x1.0p-20);
    if (!(ex >= 0.0) || !(ez >= 0.0) || !std::isfinite(ex) || !std::isfinite(ez) || !std::isfinite(cs))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_visibility_within_distance: non-finite coordinates");
    auto cells = [&](double c) { return (std::floor(ex / c) + 1.0) * (std::floor(ez / c) + 1.0); };
    while (cells(cs) > (double)(1 << 24)) cs *= 2.0;                     // wider cells stay correct, only slower
    g.inv_cs = 1.0 / cs;
    g.ncx = (int)std::floor(ex / cs) + 1; g.ncz = (int)std::floor(ez / cs) + 1;
    const int64_t n_cells = (int64_t)g.ncx * g.ncz;

    DevArena arena;
    DevBuf<uint32_t> cell_of, counts, cursor, sorted, tiles, total, cam_count, pos, max32;
    DevBuf<unsigned long long> sum64;
    DevBuf<uint64_t> row64;
    const int64_t big = std::max(n_cells + 1, n_cam + 1);
    auto temporaries = [&](auto &&each) {
        each(cell_of, (size_t)n_pts); each(counts, (size_t)(n_cells + 1)); each(cursor, (size_t)(n_cells + 1));
        each(sorted, (size_t)n_pts); each(tiles, (size_t)(big / kScanTile + 2)); each(total, (size_t)1);
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
    if (n_pts) hipLaunchKernelGGL(k_cells_assign, dim3(blocks_of(n_pts, 256)), dim3(256), 0, st, reinterpret_cast<const double4 *>(p->pts4.ptr), n_pts,
                                  g, cell_of, counts);
    uint32_t n_sorted = 0, n_kept32 = 0;
    uint32_t *start = cursor;                             // scanned counts; the fill's cursors live in `counts` afterwards
    e = scan_flags(st, counts, n_cells + 1, start, tiles, total, &n_sorted);
    if (e == hipSuccess && (int64_t)n_sorted != n_pts) return fail(C2B_ERR_HIP, "problem_visibility_within_distance: cell counts do not add up");
    if (e == hipSuccess) e = hipMemsetAsync(counts.ptr, 0, 4 * (size_t)(n_cells + 1), st);
    if (e == hipSuccess && n_pts)
        hipLaunchKernelGGL(k_cells_fill, dim3(blocks_of(n_pts, 256)), dim3(256), 0, st, cell_of, n_pts,
                           (const uint32_t *)start, counts, sorted);
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
    rc = c2b_stats(p->camblk, p->cen4, n_cam, p->pts4, 0, p->ws, p->stats, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stats, p->stats, sizeof stats, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    CellGrid g;
    g.x0 = stats[6]; g.z0 = stats[8];
    const double ex = stats[9] - stats[6], ez = stats[11] - stats[8];
    double cs = (max_dist > 0.0 ? max_dist : 1.0) * (1.0 + 0x1.0p-20);
    if (!(ex >= 0.0) || !(ez >= 0.0) || !std::isfinite(ex) || !std::isfinite(ez) || !std::isfinite(cs))
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_generate_world_points: non-finite coordinates");
    auto cells = [&](double c) { return (std::floor(ex / c) + 1.0) * (std::floor(ez / c) + 1.0); };
    while (cells(cs) > (double)(1 << 24)) cs *= 2.0;
    g.inv_cs = 1.0 / cs;
    g.ncx = (int)std::floor(ex / cs) + 1; g.ncz = (int)std::floor(ez / cs) + 1;
    const int64_t n_cells = (int64_t)g.ncx * g.ncz;
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
    if (e == hipSuccess) e = tiles.alloc((size_t)(big / kScanTile + 2));
    if (e == hipSuccess) e = total.alloc(1);
    if (e == hipSuccess) e = cand.alloc((size_t)chunk);
    if (e == hipSuccess) e = ok.alloc((size_t)chunk);
    if (e == hipSuccess) e = pos.alloc((size_t)chunk);
    if (e == hipSuccess) e = cutoff.alloc(1);
    if (e == hipSuccess) e = out.alloc(4 * (size_t)std::max<int64_t>(num_points, 1));
    if (e == hipSuccess) e = hipMemsetAsync(counts.ptr, 0, 4 * (size_t)(n_cells + 1), st);
    if (e != hipSuccess) return fail(hip_code(e), "problem_generate_world_points: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_cells_assign, dim3(blocks_of(n_cam, 256)), dim3(256), 0, st, centres, n_cam, g, cell_of, counts);
    uint32_t n_sorted = 0;
    e = scan_flags(st, counts, n_cells + 1, startb, tiles, total, &n_sorted);
    if (e == hipSuccess && (int64_t)n_sorted != n_cam) return fail(C2B_ERR_HIP, "problem_generate_world_points: cell counts do not add up");
    if (e == hipSuccess) e = hipMemsetAsync(counts.ptr, 0, 4 * (size_t)(n_cells + 1), st);
    if (e == hipSuccess)
        hipLaunchKernelGGL(k_cells_fill, dim3(blocks_of(n_cam, 256)), dim3(256), 0, st, cell_of, n_cam, startb, counts, sorted);
    if (e == hipSuccess) e = launch_error();
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
    drop_lm_state(p);
    p->pts4 = std::move(out);
    p->n_pts = accepted;
    *n_out = accepted;
    return C2B_OK;
    C2B_API_END("problem_generate_world_points")
}

#include "capi_files.hpp"        // c2b_problem_write / c2b_problem_read: both file forms assembled / taken apart on the device

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

static void cameras_mutated(c2b_problem *p) { p->bal_valid = false; p->blk_valid = false; p->bal9_fresh = false; }

int c2b_problem_add_drift(c2b_problem *p, double strength, double angle_strength, double std, const double dir[3],
                          uint64_t seed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_drift");
    if (!dir) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_drift: dir is NULL");
    int rc = compute_stats(p);
    if (rc) return rc;
    rc = c2b_add_drift(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats + 15, strength, angle_strength, std, dir[0],
                       dir[1], dir[2], seed, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_add_drift")
}

int c2b_problem_add_drift_normalized(c2b_problem *p, double strength, double angle_strength, double std,
                                     uint64_t seed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_drift_normalized");
    int rc = compute_stats(p);
    if (rc) return rc;
    rc = c2b_add_drift_normalized(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, strength, angle_strength, std, seed,
                                  p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_add_drift_normalized")
}

int c2b_problem_add_noise(c2b_problem *p, double translation_std, double rotation_std, double point_std,
                          double observations_std, uint64_t seed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_noise");
    int rc = compute_stats(p);
    if (rc) return rc;
    rc = c2b_add_noise_entities(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, translation_std, rotation_std,
                                point_std, seed, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    rc = c2b_add_noise_observations(p->uv, p->n_obs, 0, observations_std, seed, p->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_add_noise")
}

// add_noise followed by the L1 / L2 errors of the result -- run_noise's tail (src/bin/city2ba.rs:334-354) -- with the
// observation pass and both error sums in one launch.  comm != NULL: the problem is a shard (statistics and the
// 2-element sum go through the communicator).
static int sharded_stats(c2b_problem *p, c2b_comm *comm);
static int add_noise_errors_impl(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std, double point_std,
                                 double observations_std, uint64_t seed, double *l1, double *l2) {
    int rc = comm ? sharded_stats(p, comm) : compute_stats(p);
    if (rc) return rc;
    rc = comm ? c2b_add_noise_entities_sharded(p->cam15, p->n_cam, p->shard_cam_base, p->pts4, p->n_pts, p->stats, translation_std,
                                               rotation_std, point_std, seed, p->stream)
              : c2b_add_noise_entities(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, translation_std, rotation_std, point_std,
                                       seed, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    rc = ensure_camblk(p);                                 // the perturbed cameras' records
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    if (p->n_obs > 0)
        rc = c2b_add_noise_observations_error_sums2_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv,
                                                         p->n_obs, comm ? p->shard_obs_base : 0, observations_std, seed, p->ws,
                                                         p->scalar, p->stream);
    else
        HIP_TRY(hipMemsetAsync(p->scalar, 0, 2 * sizeof(double), p->stream));
    if (!rc && comm) rc = c2b_comm_all_reduce_sum_f64(comm, p->scalar, 2, p->stream);
    if (rc) return rc;
    double sums[2] = {0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(sums, p->scalar, 2 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    *l1 = std::pow(sums[0], 1.0 / 1.0);
    *l2 = std::pow(sums[1], 1.0 / 2.0);
    return C2B_OK;
}

int c2b_problem_add_noise_errors_l1_l2(c2b_problem *p, double translation_std, double rotation_std, double point_std,
                                       double observations_std, uint64_t seed, double *l1, double *l2) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_noise_errors_l1_l2");
    if (!l1 || !l2) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_noise_errors_l1_l2: NULL output");
    return add_noise_errors_impl(p, nullptr, translation_std, rotation_std, point_std, observations_std, seed, l1, l2);
    C2B_API_END("problem_add_noise_errors_l1_l2")
}

int c2b_problem_add_sin_noise(c2b_problem *p, const double dir[3], const double noise_dir[3], double strength,
                              double frequency) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_sin_noise");
    if (!dir || !noise_dir) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_sin_noise: NULL direction");
    int rc = compute_stats(p);
    if (rc) return rc;
    rc = c2b_add_sin_noise(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, dir[0], dir[1], dir[2], noise_dir[0],
                           noise_dir[1], noise_dir[2], strength, frequency, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_add_sin_noise")
}

// ---- Level 1 for a problem that is ONE SHARD of a larger one -------------------------------
// One c2b_problem per GPU holds a contiguous camera range (c2b_partition_cameras), its slice of the observation list
// and the WHOLE point table.  After c2b_problem_set_shard the *_sharded entries below give, shard by shard, exactly what
// the unsharded calls give on the whole problem: draws are keyed by global indices, the statistics go through the
// communicator (c2b_stats_sharded), every rank perturbs the replicated points identically.  All are collective (every
// rank of the communicator calls them in the same order) and synchronous.
int c2b_problem_set_shard(c2b_problem *p, int64_t cam_base, int64_t n_cam_global, int64_t obs_base) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_set_shard");
    if (cam_base < 0 || obs_base < 0 || n_cam_global < cam_base + p->n_cam)
        return fail(C2B_ERR_INVALID_ARGUMENT, "problem_set_shard: the shard [%lld, %lld) does not fit %lld cameras",
                    (long long)cam_base, (long long)(cam_base + p->n_cam), (long long)n_cam_global);
    p->shard_cam_base = cam_base; p->shard_n_cam_global = n_cam_global; p->shard_obs_base = obs_base;
    return C2B_OK;
    C2B_API_END("problem_set_shard")
}

#define NEED_SHARD(p, comm, who)                                                                          \
    NEED_UPLOADED(p, who);                                                                                \
    if (!(comm)) return fail(C2B_ERR_INVALID_ARGUMENT, who ": communicator is NULL");                     \
    if ((p)->shard_n_cam_global < 0) return fail(C2B_ERR_INVALID_ARGUMENT, who ": c2b_problem_set_shard first"); \
    if ((comm)->device != (p)->device) return fail(C2B_ERR_INVALID_ARGUMENT, who ": communicator and problem live on different devices")

static int sharded_stats(c2b_problem *p, c2b_comm *comm) {
    int rc = ensure_camblk(p);
    if (rc) return rc;
    return c2b_stats_sharded(comm, p->camblk, p->cen4, p->n_cam, p->shard_cam_base, p->shard_n_cam_global, p->pts4, p->n_pts, p->ws,
                             p->stats, p->stream);
}

int c2b_problem_stats_sharded(c2b_problem *p, c2b_comm *comm, double *stats) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_stats_sharded");
    if (!stats) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_stats_sharded: stats is NULL");
    const int rc = sharded_stats(p, comm);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stats, p->stats, sizeof(double) * C2B_STATS_DOUBLES, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_stats_sharded")
}

// dir == NULL: add_drift_normalized (direction and scale from the global std, src/noise.rs:47-56)
int c2b_problem_add_drift_sharded(c2b_problem *p, c2b_comm *comm, double strength, double angle_strength, double std,
                                  const double *dir, uint64_t seed) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_drift_sharded");
    int rc = sharded_stats(p, comm);
    if (rc) return rc;
    rc = c2b_add_drift_sharded(p->cam15, p->n_cam, p->shard_cam_base, p->pts4, p->n_pts, p->stats, dir ? 0 : 1, strength,
                               angle_strength, std, dir ? dir[0] : 0.0, dir ? dir[1] : 0.0, dir ? dir[2] : 0.0, seed, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_add_drift_sharded")
}

int c2b_problem_add_noise_sharded(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std,
                                  double point_std, double observations_std, uint64_t seed) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_noise_sharded");
    int rc = sharded_stats(p, comm);
    if (rc) return rc;
    rc = c2b_add_noise_entities_sharded(p->cam15, p->n_cam, p->shard_cam_base, p->pts4, p->n_pts, p->stats, translation_std,
                                        rotation_std, point_std, seed, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    rc = c2b_add_noise_observations(p->uv, p->n_obs, p->shard_obs_base, observations_std, seed, p->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_add_noise_sharded")
}

int c2b_problem_add_noise_errors_l1_l2_sharded(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std,
                                               double point_std, double observations_std, uint64_t seed, double *l1, double *l2) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_noise_errors_l1_l2_sharded");
    if (!l1 || !l2) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_noise_errors_l1_l2_sharded: NULL output");
    return add_noise_errors_impl(p, comm, translation_std, rotation_std, point_std, observations_std, seed, l1, l2);
    C2B_API_END("problem_add_noise_errors_l1_l2_sharded")
}

int c2b_problem_add_sin_noise_sharded(c2b_problem *p, c2b_comm *comm, const double dir[3], const double noise_dir[3],
                                      double strength, double frequency) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_sin_noise_sharded");
    if (!dir || !noise_dir) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_sin_noise_sharded: NULL direction");
    int rc = sharded_stats(p, comm);                        // the extent of the WHOLE problem scales the phase
    if (rc) return rc;
    rc = c2b_add_sin_noise(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, dir[0], dir[1], dir[2], noise_dir[0],
                           noise_dir[1], noise_dir[2], strength, frequency, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
    C2B_API_END("problem_add_sin_noise_sharded")
}

