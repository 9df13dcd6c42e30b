// capi_problem.hpp -- Level 1 of include/city2ba_hip.h: a BAProblem resident on one device (c2b_problem_*): the handle and what it caches, upload / download, layouts,
// error sums, residual + Jacobian, statistics, the noise functions and the *_sharded forms; capi_solve.hpp, capi_graph.hpp and capi_files.hpp are included where their text sat
// Part of the one translation unit of the C ABI: included by capi.hip (inside its extern "C" block, after its helpers and
// launchers), never compiled or included on its own.

struct c2b_problem {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n_cam = 0, n_pts = 0, n_obs = 0;
    // every device array below is a DevBuf (capi.hip): the problem owns its memory through that one type, and the table
    // under this struct says which group of them goes when
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
    // c2b_problem_set_inner_iterations: rounds of c2b_problem_refine_points after every step the LM loop applies (0 = off); the handle's too
    int inner_rounds = 0;
    // c2b_problem_set_preconditioner: what c2b_problem_solve_step's PCG is preconditioned with (0 block-Jacobi on U,
    // 1 Schur-Jacobi), the handle's too; and how many cameras' Schur-Jacobi factors fell back in the last solve
    int precond_kind = 0;
    int64_t precond_fallbacks = 0;
    // c2b_problem_set_schur: how c2b_problem_solve_step applies S (0 implicit, never formed; 1 explicit, block-CSR
    // on the covisibility pattern), the handle's too
    int schur_kind = 0;
    // c2b_problem_set_linear_solver: how c2b_problem_solve_step solves S dc = b (0 PCG; 1 dense Cholesky of the
    // explicit S), the handle's too; and the device word the factorisation reports a failed pivot in (allocated with the first
    // direct solve)
    int linear_kind = 0;
    DevBuf<int32_t> dense_info;
    // c2b_problem_set_constant: the camera parameters (bit k of a camera's word, to_vec order) and the points
    // (0 / 1) that normal_equations / solve_step / apply_step hold constant; the handle's, kept while both counts stay
    // what they were set for (const_n_cam, const_n_pts).  A kind with nothing set has no array: no launch changes for it.
    DevBuf<uint16_t> cmask;
    DevBuf<uint8_t> pmask;
    std::vector<uint16_t> h_cmask;
    std::vector<uint8_t> h_pmask;
    int64_t const_n_cam = -1, const_n_pts = -1, const_params = 0, const_pts = 0;
    // c2b_problem_set_priors: targets and weights [n][3] of the camera centres (pc0, pcw), the intrinsics
    // (pi0, piw) and the points (px0, pxw), and the partials and scalars their sums go through (prior_part); the handle's,
    // kept and dropped as the masks are (prior_n_cam, prior_n_pts: the counts they were set for).  A kind whose weights
    // are all 0 has no array, and with none in force nothing is launched or allocated for priors.
    DevBuf<double> pc0, pcw, pi0, piw, px0, pxw, prior_part;
    std::vector<double> h_pc0, h_pcw, h_pi0, h_piw, h_px0, h_pxw;
    int64_t prior_n_cam = -1, prior_n_pts = -1, prior_rows[3] = {0, 0, 0};
    bool bal_valid = false;    // bal9 still describes the cameras (no mutation since upload_bal)
    bool blk_valid = false;     // camblk matches cam15 (and bal_valid mode)
    bool bal9_fresh = false;    // !bal_valid, but bal9 holds to_vec of the current cameras (the last write / download_bal computed it)
    // the row structure of the observation list for the *_rows launchers, rebuilt on demand after the list changed
    // (ensure_rows; a non-null rows_ptr is its validity, and only drop_rows clears it)
    DevBuf<uint64_t> rows_ptr;
    DevBuf<char> rows_tiles;
    // its point-major transpose for c2b_problem_normal_equations (pt_row_ptr [n_pts + 1], obs_of / cam_of [n_obs]), dropped with it
    DevBuf<uint64_t> nt_ptr;
    DevBuf<uint32_t> nt_obs, nt_cam;
    // c2b_problem_solve_step's buffers (U, gc, V, gp, the preconditioner's factors, the PCG vectors, partials, scalars):
    // one allocation, sized by the list, dropped with it
    DevBuf<double> sv;
    int64_t sv_doubles = 0;
    // c2b_problem_covisibility: the camera covisibility graph of the list at threshold cv_min_shared (nbr_ptr
    // [n_cam + 1], nbr / shared [cv_edges]) and how many cameras took the heavy path; derived from the list, dropped with it
    DevBuf<uint64_t> cv_ptr;
    DevBuf<uint32_t> cv_nbr, cv_shared;
    int cv_min_shared = 0;
    int64_t cv_edges = 0, cv_heavy = 0;
    // the sparsity pattern of the explicit S: the solver's OWN copy of the graph at threshold 1 (sp_ptr [n_cam + 1],
    // sp_nbr [sp_edges]), so that a covisibility call at another threshold does not disturb it; derived from the list, dropped with it
    DevBuf<uint64_t> sp_ptr;
    DevBuf<uint32_t> sp_nbr;
    int64_t sp_edges = 0;
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
    // identity: serial names the handle for the life of the process (set at create); entity_epoch is raised
    // wherever the entities are replaced or renumbered (entities_replaced: the rows of the table below whose masks column says X)
    uint64_t serial = 0, entity_epoch = 0;
    // c2b_problem_subset / c2b_problem_window: where this problem's entities came from -- the parent's identity and counts at
    // the extraction, child index -> parent index and the roles (cameras 0 seed / 1 halo, points 0 / 1 shared), on the host and,
    // for c2b_problem_write_back's scatters, on the device.  Gone as soon as this problem's own entities are replaced.
    bool has_origin = false;
    uint64_t origin_serial = 0, origin_epoch = 0;
    int64_t origin_n_cam = 0, origin_n_pts = 0;
    std::vector<uint32_t> h_cam_of, h_pt_of;
    std::vector<uint8_t> h_cam_role, h_pt_role;
    DevBuf<uint32_t> d_cam_of, d_pt_of;
};

// Which event drops which cache or handle state.  X: dropped (rebuilt by the next user, or gone), -: stays.  The functions
// below and cameras_mutated are the table's implementation; the list's three caches go together (drop_rows), and the
// covisibility graph (c2b_problem_covisibility) goes with them: wherever the transpose column says X, it is dropped.  "S pattern" is the
// solver's own copy of the graph at threshold 1: it goes in drop_rows too, with the blocks it addresses.
//                              camblk/cen4  bal9       rows  transpose  solve  S pattern  pending vis.  masks       checkpoint/LM
//   upload, upload_bal         X            X / truth  X     X          X      X          X             - / X (1)   X
//   layout (grid, line)        X            X          X     X          X      X          X             X           X
//   read (.bal, .bbal)         X            truth      X     X          X      X          X             X           X
//   cull                       X            - (2)      X     X          X      X          X (3)         X           X
//   adopt_visibility           -            -          X     X          X      X          X (spent)     -           -
//   filter (4)                 -            -          X     X          X      X          -             -           -
//   generate_world_points      -            -          X     X          X      X          X             X           X
//   apply_step, rollback (5)   X            truth      -     -          -      -          -             -           -
//   noise (drift, noise, sin)  X            X          -     -          -      -          -             -           -
//   transform (14)             X            X          -     -          -      -          -             -           -
//   triangulate_points         -            -          -     -          -      -          -             -           -
//   refine_points              -            -          -     -          -      -          -             -           -
//   triangulate_consensus (6)  -            -          - / X - / X      - / X  - / X      -             -           -
//   resect_cameras             X            truth      -     -          -      -          -             -           -
//   refine_cameras             X            truth      -     -          -      -          -             -           -
//   resect_consensus (6)       X            truth      - / X - / X      - / X  - / X      -             -           -
//   merge_points (7)           -            -          - / X - / X      - / X  - / X      -             -           -
//   rematch_observations (8)   -            -          - / X - / X      - / X  - / X      -             -           -
//   drop_features (4)          -            -          X     X          X      X          -             -           -
//   mismatch, join (12)        -            -          - / X - / X      - / X  - / X      -             -           -
//   split_landmarks (13)       -            -          X     X          X      X          X             X           X
//   subset, window: src        -            - (9)      -     -          -      -          -             -           -
//   subset, window: dst (10)   X            X / truth  X     X          X      X          X             X / carried X
//   get_origin                 -            -          -     -          -      -          -             -           -
//   write_back: parent         X            truth      -     -          -      -          -             -           -
//   write_back: child (11)     - / X        - / truth  -     -          -      -          -             -           -
// The priors (c2b_problem_set_priors) share the masks' column: kept and dropped with them, by counts of their own.
// (1) kept when both counts are those the masks were set for.  (2) gathered with the cameras while it is the truth; a merely
// fresh bal9 (bal9_fresh: to_vec of the current cameras, filled by download_bal / write / apply_step) is dropped.  (3) on
// entry, so also by a cull that fails later.  (4) one that removes nothing drops nothing.  (5) checkpoint is an apply_step
// of no step, then the copy.  (6) with C2B_TRI_DROP_OUTLIERS / C2B_RES_DROP_OUTLIERS and something removed: as the filter.  (7) after every round that merged: as the filter.
// (8) after a call that reassigned or removed something: as the filter.  A new visibility result
// (pairs_compact, within_distance, dense) replaces the pending one only.  (9) the source is read, never written.  (10) replaced
// as an upload replaces it, in the source's camera mode (bal9 gathered while it is the source's truth); the masks and priors are
// the source's, gathered by the origin lists, with C2B_SUBSET_CARRY (a window: always, OR the roles) and dropped without; the
// origin (above) is recorded by a window, and by a carrying subset of repeat-free lists.  (11) a state-mode child gets to_vec of
// its cameras and is in bal mode afterwards; a child in bal mode is only read.  (12) add_incorrect_correspondences, join_landmarks
// (DESIGN 4.18): after a call that changed a label, as the filter.  (13) the point count grows: cull's policy; a call that selects
// no point drops nothing.  (14) c2b_problem_transform (capi_align.hpp): a similarity of the whole problem, the noise row; the
// priors hold positions in the old frame and are left as they are.  c2b_problem_align writes neither problem (it may build camblk / cen4).
// An X in the masks column is also where the handle's entity_epoch is raised and its origin dropped (entities_replaced).
// the cameras moved: every cache of them (apply_step / rollback then make bal9 the truth)
static void cameras_mutated(c2b_problem *p) { p->bal_valid = false; p->blk_valid = false; p->bal9_fresh = false; }

// the pending visibility result
static void free_dense(c2b_problem *p) {
    p->dense_pt.reset(); p->dense_uv.reset(); p->dense_row.reset();
    p->dense_n = 0;
}

// what is derived from the observation list: row structure, transpose, solve buffers, covisibility graph, the pattern of S
static void drop_rows(c2b_problem *p) {
    p->rows_ptr.reset(); p->rows_tiles.reset();
    p->nt_ptr.reset(); p->nt_obs.reset(); p->nt_cam.reset();
    p->sv.reset();
    p->sv_doubles = 0;
    p->cv_ptr.reset(); p->cv_nbr.reset(); p->cv_shared.reset();
    p->cv_min_shared = 0;
    p->cv_edges = p->cv_heavy = 0;
    p->sp_ptr.reset(); p->sp_nbr.reset();
    p->sp_edges = 0;
}

// the masks: nothing is constant any more
static void drop_constant(c2b_problem *p) {
    p->cmask.reset(); p->pmask.reset();
    p->h_cmask.clear(); p->h_pmask.clear();
    p->const_n_cam = p->const_n_pts = -1;
    p->const_params = p->const_pts = 0;
}

// the priors: no soft constraint any more (dropped wherever the masks are dropped for a count change or a renumbering)
static void drop_priors(c2b_problem *p) {
    p->pc0.reset(); p->pcw.reset(); p->pi0.reset(); p->piw.reset(); p->px0.reset(); p->pxw.reset(); p->prior_part.reset();
    for (auto *v : {&p->h_pc0, &p->h_pcw, &p->h_pi0, &p->h_piw, &p->h_px0, &p->h_pxw}) v->clear();
    p->prior_n_cam = p->prior_n_pts = -1;
    p->prior_rows[0] = p->prior_rows[1] = p->prior_rows[2] = 0;
}
static bool has_priors(const c2b_problem *p) { return p->pcw || p->piw || p->pxw; }

// the checkpoint and the LM scratch: no checkpoint describes the entities any more
static void drop_lm_state(c2b_problem *p) {
    p->ck_bal9.reset(); p->ck_pts4.reset(); p->lm.reset();
    p->ck_valid = false;
}

// the origin of a sub-problem: it no longer describes the entities
static void drop_origin(c2b_problem *p) {
    p->has_origin = false;
    p->h_cam_of.clear(); p->h_pt_of.clear(); p->h_cam_role.clear(); p->h_pt_role.clear();
    p->d_cam_of.reset(); p->d_pt_of.reset();
}

// the entities were replaced or renumbered: no origin taken FROM this problem fits it any more, and its own origin is gone
static void entities_replaced(c2b_problem *p) {
    ++p->entity_epoch;
    drop_origin(p);
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
    static std::atomic<uint64_t> next_serial{1};
    p->serial = next_serial.fetch_add(1, std::memory_order_relaxed);
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
    drop_priors(p);
    drop_origin(p);
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

// a workspace for a list of n_obs observations, its counters zeroed on the stream (asynchronous)
static int new_workspace(DevBuf<char> &ws, int64_t n_obs, hipStream_t st) {
    HIP_TRY(ws.alloc((size_t)c2b_workspace_bytes(n_obs)));
    return c2b_workspace_init(ws, st);
}

// the resident arrays of a problem with these sizes (whatever it held before is freed); contents undefined.  The constant
// masks go too, unless the caller brings the same entities back (an upload) and both counts are those they were set for.
static int alloc_problem(c2b_problem *p, int64_t n_cam, int64_t n_pts, int64_t n_obs, bool same_entities = false) {
    HIP_TRY(hipSetDevice(p->device));
    free_buffers(p);
    entities_replaced(p);
    if (!same_entities || n_cam != p->const_n_cam || n_pts != p->const_n_pts) drop_constant(p);
    if (!same_entities || n_cam != p->prior_n_cam || n_pts != p->prior_n_pts) drop_priors(p);
    HIP_TRY(p->cam15.alloc(15 * (size_t)n_cam));
    HIP_TRY(p->bal9.alloc(9 * (size_t)n_cam));
    HIP_TRY(p->camblk.alloc((size_t)cam_table_doubles(n_cam)));      // whole groups of 8 cameras
    HIP_TRY(p->cen4.alloc(4 * (size_t)n_cam));
    HIP_TRY(p->pts4.alloc(4 * (size_t)n_pts));
    HIP_TRY(p->uv.alloc(2 * (size_t)n_obs));
    HIP_TRY(p->cam_idx.alloc((size_t)n_obs));
    HIP_TRY(p->pt_idx.alloc((size_t)n_obs));
    if (int rc = new_workspace(p->ws, n_obs, p->stream)) return rc;
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
    p->bal_valid = is_bal;                                   // (alloc_problem left the flags off)
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
    return C2B_OK;                                           // (alloc_problem left all three camera flags off: cam15 is the truth)
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
    return C2B_OK;                                           // (alloc_problem left all three camera flags off: cam15 is the truth)
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

// row_ptr (from the camera-major cam_idx) and the tile records of the current observation list: built into locals and
// moved in on success, as ensure_transpose does (a failure leaves the problem without rows, never with half of them)
static int ensure_rows(c2b_problem *p) {
    if (p->rows_ptr || !p->n_obs) return C2B_OK;
    DevBuf<uint64_t> ptr;
    DevBuf<char> tiles;
    HIP_TRY(ptr.alloc((size_t)p->n_cam + 1));
    HIP_TRY(tiles.alloc((size_t)c2b_rows_tiles_bytes(p->n_obs)));
    hipLaunchKernelGGL(k_rows_from_sorted, dim3(blocks_for(p->n_obs + 1)), dim3(kBlock), 0, p->stream, (const uint32_t *)p->cam_idx,
                       p->n_obs, p->n_cam, ptr.ptr);
    LAUNCH_CHECK();
    const int rc = c2b_rows_pack(ptr, p->n_cam, p->n_obs, tiles, p->stream);
    if (rc) return rc;
    p->rows_ptr = std::move(ptr); p->rows_tiles = std::move(tiles);
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

// comm != NULL: the problem is one SHARD (a contiguous camera range) of a larger one: the local sum, one 8-byte all-reduce through
// the communicator on the problem's stream, then .powf(1/norm): every rank returns the global error (src/baproblem.rs:265-279).
static int total_error_impl(c2b_problem *p, c2b_comm *comm, double norm, double *out) {
    int rc = ensure_camblk(p);
    if (!rc) rc = ensure_rows(p);
    if (rc) return rc;
    if (p->n_obs > 0 || !comm)                               // (alone, the launcher itself turns an empty list into 0)
        rc = c2b_reprojection_error_sum_rows(p->camblk, p->pts4, p->rows_ptr, p->n_cam, p->rows_tiles, p->pt_idx, p->uv, p->n_obs,
                                             norm, p->ws, p->scalar, p->stream);
    else
        HIP_TRY(hipMemsetAsync(p->scalar, 0, sizeof(double), p->stream));          // an empty shard still takes part
    if (!rc && comm) rc = c2b_comm_all_reduce_sum_f64(comm, p->scalar, 1, p->stream);
    if (rc) return rc;
    double sum = 0.0;
    if ((rc = scalars_to_host(p->stream, p->scalar, 1, &sum))) return rc;
    *out = std::pow(sum, 1.0 / norm);          // .powf(1. / norm), src/baproblem.rs:278
    return C2B_OK;
}

int c2b_problem_total_reprojection_error(c2b_problem *p, double norm, double *out) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_total_reprojection_error");
    if (!out) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_error: out is NULL");
    return total_error_impl(p, nullptr, norm, out);
    C2B_API_END("problem_total_reprojection_error")
}

// Collective: every rank of the communicator must call it.
int c2b_problem_total_reprojection_error_sharded(c2b_problem *p, c2b_comm *comm, double norm, double *out) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_total_reprojection_error_sharded");
    if (!out || !comm) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_error_sharded: NULL argument");
    if (comm->device != p->device) return fail(C2B_ERR_INVALID_ARGUMENT, "total_reprojection_error_sharded: communicator and problem live on different devices");
    return total_error_impl(p, comm, norm, out);
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
    if ((rc = scalars_to_host(p->stream, p->scalar, 2, sums))) return rc;
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

#include "capi_solve.hpp"        // constant parameters ... Levenberg-Marquardt: everything the solver calls

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
    const int rc = compute_stats(p);
    return rc ? rc : scalars_to_host(p->stream, p->stats, C2B_STATS_DOUBLES, stats);
    C2B_API_END("problem_stats")
}

#include "capi_graph.hpp"        // cull, adopt, filter, the visibility entries, generate_world_points, the dense sweep
#include "capi_subset.hpp"       // subset, window, get_origin, write_back: a sub-problem cut out on the device and put back
#include "capi_index_noise.hpp"  // drop_features, add_incorrect_correspondences, split_landmarks, join_landmarks in place
#include "capi_files.hpp"        // c2b_problem_write / c2b_problem_read: both file forms assembled / taken apart on the device

// ---- the noise functions, alone and for a problem that is ONE SHARD of a larger one ----------
// One c2b_problem per GPU holds a contiguous camera range (c2b_partition_cameras), its slice of the observation list
// and the WHOLE point table.  After c2b_problem_set_shard the *_sharded entries below give, shard by shard, exactly what
// the unsharded calls give on the whole problem: draws are keyed by global indices, the statistics go through the
// communicator (c2b_stats_sharded), every rank perturbs the replicated points identically.  All are collective (every
// rank of the communicator calls them in the same order) and synchronous.  A pair of entries shares one implementation
// whose comm is NULL for the problem alone; that case keeps its own launcher, never the sharded one with base 0.
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

// the statistics of the whole problem into p->stats (compute_stats's centres-only shortcut is the unsharded path's alone)
static int noise_stats(c2b_problem *p, c2b_comm *comm) {
    if (!comm) return compute_stats(p);
    if (const int rc = ensure_camblk(p)) return rc;
    return c2b_stats_sharded(comm, p->camblk, p->cen4, p->n_cam, p->shard_cam_base, p->shard_n_cam_global, p->pts4, p->n_pts, p->ws,
                             p->stats, p->stream);
}

int c2b_problem_stats_sharded(c2b_problem *p, c2b_comm *comm, double *stats) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_stats_sharded");
    if (!stats) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_stats_sharded: stats is NULL");
    const int rc = noise_stats(p, comm);
    return rc ? rc : scalars_to_host(p->stream, p->stats, C2B_STATS_DOUBLES, stats);
    C2B_API_END("problem_stats_sharded")
}

// dir == NULL: add_drift_normalized (direction and scale from the global std, src/noise.rs:47-56)
static int add_drift_impl(c2b_problem *p, c2b_comm *comm, double strength, double angle_strength, double std, const double *dir, uint64_t seed) {
    int rc = noise_stats(p, comm);
    if (rc) return rc;
    if (comm)
        rc = c2b_add_drift_sharded(p->cam15, p->n_cam, p->shard_cam_base, p->pts4, p->n_pts, p->stats, dir ? 0 : 1, strength,
                                   angle_strength, std, dir ? dir[0] : 0.0, dir ? dir[1] : 0.0, dir ? dir[2] : 0.0, seed, p->stream);
    else if (dir)
        rc = c2b_add_drift(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats + 15, strength, angle_strength, std, dir[0], dir[1], dir[2],
                           seed, p->stream);
    else
        rc = c2b_add_drift_normalized(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, strength, angle_strength, std, seed, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
}

int c2b_problem_add_drift(c2b_problem *p, double strength, double angle_strength, double std, const double dir[3], uint64_t seed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_drift");
    if (!dir) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_drift: dir is NULL");
    return add_drift_impl(p, nullptr, strength, angle_strength, std, dir, seed);
    C2B_API_END("problem_add_drift")
}

int c2b_problem_add_drift_normalized(c2b_problem *p, double strength, double angle_strength, double std, uint64_t seed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_drift_normalized");
    return add_drift_impl(p, nullptr, strength, angle_strength, std, nullptr, seed);
    C2B_API_END("problem_add_drift_normalized")
}

int c2b_problem_add_drift_sharded(c2b_problem *p, c2b_comm *comm, double strength, double angle_strength, double std,
                                  const double *dir, uint64_t seed) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_drift_sharded");
    return add_drift_impl(p, comm, strength, angle_strength, std, dir, seed);
    C2B_API_END("problem_add_drift_sharded")
}

// the entity half of add_noise (asynchronous): the statistics, the cameras and points perturbed
static int noise_entities(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std, double point_std, uint64_t seed) {
    int rc = noise_stats(p, comm);
    if (rc) return rc;
    rc = comm ? c2b_add_noise_entities_sharded(p->cam15, p->n_cam, p->shard_cam_base, p->pts4, p->n_pts, p->stats, translation_std,
                                               rotation_std, point_std, seed, p->stream)
              : c2b_add_noise_entities(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, translation_std, rotation_std, point_std,
                                       seed, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    return C2B_OK;
}

static int add_noise_impl(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std, double point_std,
                          double observations_std, uint64_t seed) {
    int rc = noise_entities(p, comm, translation_std, rotation_std, point_std, seed);
    if (!rc) rc = c2b_add_noise_observations(p->uv, p->n_obs, comm ? p->shard_obs_base : 0, observations_std, seed, p->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
}

int c2b_problem_add_noise(c2b_problem *p, double translation_std, double rotation_std, double point_std, double observations_std, uint64_t seed) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_noise");
    return add_noise_impl(p, nullptr, translation_std, rotation_std, point_std, observations_std, seed);
    C2B_API_END("problem_add_noise")
}

int c2b_problem_add_noise_sharded(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std,
                                  double point_std, double observations_std, uint64_t seed) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_noise_sharded");
    return add_noise_impl(p, comm, translation_std, rotation_std, point_std, observations_std, seed);
    C2B_API_END("problem_add_noise_sharded")
}

// add_noise followed by the L1 / L2 errors of the result -- run_noise's tail (src/bin/city2ba.rs:334-354) -- with the
// observation pass and both error sums in one launch (the 2-element sum goes through the communicator of a shard)
static int add_noise_errors_impl(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std, double point_std,
                                 double observations_std, uint64_t seed, double *l1, double *l2) {
    int rc = noise_entities(p, comm, translation_std, rotation_std, point_std, seed);
    if (!rc) rc = ensure_camblk(p);                        // the perturbed cameras' records
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
    if ((rc = scalars_to_host(p->stream, p->scalar, 2, sums))) return rc;
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

int c2b_problem_add_noise_errors_l1_l2_sharded(c2b_problem *p, c2b_comm *comm, double translation_std, double rotation_std,
                                               double point_std, double observations_std, uint64_t seed, double *l1, double *l2) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_noise_errors_l1_l2_sharded");
    if (!l1 || !l2) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_noise_errors_l1_l2_sharded: NULL output");
    return add_noise_errors_impl(p, comm, translation_std, rotation_std, point_std, observations_std, seed, l1, l2);
    C2B_API_END("problem_add_noise_errors_l1_l2_sharded")
}

// (a shard: the extent of the WHOLE problem scales the phase; the launcher is the same)
static int add_sin_noise_impl(c2b_problem *p, c2b_comm *comm, const double dir[3], const double noise_dir[3], double strength, double frequency) {
    int rc = noise_stats(p, comm);
    if (rc) return rc;
    rc = c2b_add_sin_noise(p->cam15, p->n_cam, p->pts4, p->n_pts, p->stats, dir[0], dir[1], dir[2], noise_dir[0],
                           noise_dir[1], noise_dir[2], strength, frequency, p->stream);
    if (rc) return rc;
    cameras_mutated(p);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return C2B_OK;
}

int c2b_problem_add_sin_noise(c2b_problem *p, const double dir[3], const double noise_dir[3], double strength, double frequency) {
    C2B_API_BEGIN
    NEED_UPLOADED(p, "problem_add_sin_noise");
    if (!dir || !noise_dir) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_sin_noise: NULL direction");
    return add_sin_noise_impl(p, nullptr, dir, noise_dir, strength, frequency);
    C2B_API_END("problem_add_sin_noise")
}

int c2b_problem_add_sin_noise_sharded(c2b_problem *p, c2b_comm *comm, const double dir[3], const double noise_dir[3],
                                      double strength, double frequency) {
    C2B_API_BEGIN
    NEED_SHARD(p, comm, "problem_add_sin_noise_sharded");
    if (!dir || !noise_dir) return fail(C2B_ERR_INVALID_ARGUMENT, "problem_add_sin_noise_sharded: NULL direction");
    return add_sin_noise_impl(p, comm, dir, noise_dir, strength, frequency);
    C2B_API_END("problem_add_sin_noise_sharded")
}
