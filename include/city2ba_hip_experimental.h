/*
 * city2ba_hip_experimental.h -- entry points of libcity2ba_hip.so that are NOT part of the stable boundary (city2ba_hip.h):
 * measurement aids the benchmark uses in the same process as the timed run, diagnostics that name the kernel instance a
 * launch takes, and the f32 extension of BASELINE configs[4] (the reference has no f32 path).  They may change between
 * rounds; a drop-in host needs none of them.
 */
#ifndef CITY2BA_HIP_EXPERIMENTAL_H
#define CITY2BA_HIP_EXPERIMENTAL_H
#include "city2ba_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagnostics ---- */
/* Diagnostic: synchronises `stream`, then counts the workspace's non-zero arrival counters.  Zero whenever no launch
 * using it is in flight; anything else means a fold did not complete.  -1: the workspace was never initialised. */
int c2b_workspace_selfcheck(const void *workspace, void *stream, int64_t *nonzero_words);
/* "RCCL 2.x.y (path)" or "unavailable: ..." */
const char *c2b_comm_backend(void);
/* tiles of 64 observations a wave of the residual + Jacobian launch takes: 1 below ~6 M observations, else 2
 * (diagnostic: names the kernel instance a launch of this size runs; results do not depend on it, the rounding of
 * the folded error sum does, like on any other change of the grid) */
int c2b_jacobian_tiles_per_wave(int64_t n_obs);
/* ... and the full shape -- waves of 64 per workgroup, tiles per wave -- of a launch of n_obs observations into an output
 * set that takes streaming stores at store_GBs (GB/s; 0 = unknown): 16 x 1 below ~6 M observations; above, 8 x 2 -- or
 * 4 x 1 when the set is one of the slow-store kind (< 6.3 TB/s) and 16 x 1 when it lies between the classes (< 6.85 TB/s),
 * which only c2b_residual_jacobian_rows_placed knows.  Diagnostic, like the two above: results do not depend on the shape.
 * The shapes named are those of a launch WITH an error sum (workspace != NULL, the bench step).  One exception: a launch
 * without a sum (workspace == NULL) that would take 8 x 2 runs 16 x 1 instead -- the 8 x 2 instance without the sum's
 * fold does not fit its 128 registers without scratch (capi.hip: launch_jac_l). */
int c2b_jacobian_launch_shape(int64_t n_obs, double store_GBs, int *waves_per_workgroup, int *tiles_per_wave);

/* ---- placed output sets: the search's log, overriding the recorded rate ---- */
/* store rate (GB/s) measured for every attempt, how many there were, and which one was kept */
int c2b_jacobian_outputs_log(const c2b_jacobian_outputs *h, double *store_GBs_per_attempt, int capacity, int *attempts,
                             int *chosen);
/* replace it: for a caller that timed the set itself, or wants one particular launch shape (<= 0: "unknown") */
int c2b_jacobian_outputs_set_store_rate(c2b_jacobian_outputs *h, double store_GBs);

/* Calibration (measurement aids, no reference counterpart; used by bench.py in the same process as the timed run so
 * that a slow device can be told from a slow kernel).  _store_pattern writes a fill pattern over r [n][2], Jc [n][18],
 * Jp [n][6] in exactly the residual+Jacobian kernel's store geometry with no loads and no arithmetic -- the time its
 * stores alone take; _copy is a 16-bytes-per-lane streaming copy (bytes % 16 == 0). */
int c2b_calib_store_pattern(int64_t n_obs, double *r, double *Jc, double *Jp, void *stream);
int c2b_calib_copy(const void *src, void *dst, int64_t bytes, void *stream);

/* ---- Gauss-Newton diagonal blocks, Level 0 (c2b_problem_normal_equations is the stable entry) ----
 * The whole observation list in the row-structure form (row_ptr [n_cam + 1] over the camera-major list; pt_idx, uv_obs
 * its observations; camblk, pts4 as for c2b_residual_jacobian_rows, whose Jacobian these passes reduce without storing it).
 * The passes need no tile records: the camera pass walks row_ptr, the point pass the transpose.
 * _transpose: the point-major order of the list -- pt_row_ptr [n_pts + 1] (u64), obs_of [n_obs] the observations of
 * each point in ascending order (= a stable argsort of pt_idx), cam_of [n_obs] the camera of obs_of[j]; temp is
 * c2b_normal_transpose_temp_bytes(n_obs, n_pts) bytes of device memory (16-byte aligned), free once the stream passed
 * the call: the counts / cursors of the points, the fill's slots and the tile sums of the scan over the points (about
 * 8 bytes per 1024 points) -- ask for the size, never compute it.  Every pt_idx must be < n_pts.
 * _cameras_rows: U [n_cam][9][9], gc [n_cam][9] (both required); with a workspace and sum_sq != NULL (device pointer)
 * the same launch folds sum |r|^2 into sum_sq[0].
 * _points_rows: V [n_pts][3][3], gp [n_pts][3] from the transpose.
 * Asynchronous on `stream`; results as c2b_problem_normal_equations describes. */
int64_t c2b_normal_transpose_temp_bytes(int64_t n_obs, int64_t n_pts);
int c2b_normal_transpose(const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx, int64_t n_obs, int64_t n_pts,
                         uint64_t *pt_row_ptr, uint32_t *obs_of, uint32_t *cam_of, void *temp, void *stream);
int c2b_normal_cameras_rows(const double *camblk, const double *pts4, const uint64_t *row_ptr, int64_t n_cam,
                            const uint32_t *pt_idx, const double *uv_obs, int64_t n_obs, double *U, double *gc,
                            void *workspace, double *sum_sq, void *stream);
int c2b_normal_points_rows(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr,
                           const uint32_t *obs_of, const uint32_t *cam_of, const double *uv_obs, double *V, double *gp,
                           void *stream);

/* ---- damped Gauss-Newton (Levenberg-Marquardt) step: implicit Schur complement + PCG ----
 * The damped normal equations (J^T J + lambda D) delta = -g of the Jacobian c2b_problem_residual_jacobian gives (same
 * bal- or state-mode columns, r = projected - observed), solved on the device without storing J, W or S.  H = J^T J has
 * the diagonal blocks U_c (9x9), V_p (3x3) of c2b_problem_normal_equations and W_cp = sum Jc^T Jp; g = (gc, gp).
 * Damping: A_l = A + lambda diag(d) for every diagonal block A, d_i = min(max(A_ii, 1e-6), 1e32); lambda in
 * [C2B_STEP_LAMBDA_MIN, C2B_STEP_LAMBDA_MAX] (inside it lambda * 1e-6 and lambda * 1e32 stay normal doubles), else
 * C2B_ERR_INVALID_ARGUMENT.
 * Reduced camera system S dc = b, S = U_l - W V_l^-1 W^T, b = -gc + W V_l^-1 gp; dp = -V_l^-1 (gp + W^T dc).
 *
 * Level 0, asynchronous on `stream`, the inputs of c2b_normal_points_rows / _cameras_rows plus U or V as those fill them:
 * _points_rows: t_pts [n_pts][3] = V_l,p^-1 (h_p + sum_o Jp_o^T (Jc_o x_c(o))), each point's observations in ascending
 *   index through the transpose; x_cam [n_cam][9] NULL means 0 (no observation is read), h_pts [n_pts][3] NULL means 0.
 * _cameras_rows: y_cam [n_cam][9] = U_l,c x_c - sum_o Jc_o^T (Jp_o t_p(o)) over each camera's list; x_cam NULL drops
 *   the U term.  So S x = cameras(x, points(x, NULL)) and b = -gc - cameras(NULL, points(NULL, gp)).
 * Deterministic: no float atomics; every sum runs in an order fixed by the problem. */
#define C2B_STEP_LAMBDA_MIN 1e-20
#define C2B_STEP_LAMBDA_MAX 1e32
int c2b_schur_points_rows(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr,
                          const uint32_t *obs_of, const uint32_t *cam_of, const double *uv_obs, const double *V, double lambda,
                          const double *x_cam, const double *h_pts, double *t_pts, void *stream);
int c2b_schur_cameras_rows(const double *camblk, const double *pts4, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx,
                           const double *uv_obs, int64_t n_obs, const double *U, double lambda, const double *x_cam,
                           const double *t_pts, double *y_cam, void *stream);
/* Level 1, synchronous; dc [n_cam][9] and dp [n_pts][3] are DEVICE arrays on the problem's device (8-byte aligned).
 * _solve_step: forms U, gc, V, gp (the passes of c2b_problem_normal_equations) into buffers the problem keeps until its
 *   observation list changes, then PCG on S from dc = 0 with the block-Jacobi preconditioner U_l,c (9x9 Cholesky): it
 *   stops when the recurrence residual |b - S x_k| <= rel_tol |b| (status 0), after max_iters iterations (status 1), or
 *   on a breakdown -- p.Sp <= 0 or a non-finite value -- with dc the last good iterate (status 2).  b = 0: a zero step
 *   after 0 iterations.  Then dp by back-substitution.  A step whose model pass is not finite (near the low end of the
 *   damping range a 3x3 factorisation of a point seen once can fail) is returned as dc = dp = 0 with status 2,
 *   rel_residual 1 and model_decrease 0.  info (may be NULL): iterations, status, rel_residual |r_k| / |b|,
 *   sum_sq = |r|^2 at the current state and model_decrease = |r|^2 - |r + Jc dc + Jp dp|^2, both summed per observation
 *   from J.  An empty camera or an unobserved point gets an exact zero.  A problem with a shard set is refused: the
 *   point-side sums span every rank.  Deterministic: the same problem and arguments give the same bits.
 * _apply_step: bal9 = (bal mode ? bal9 : to_vec(cam15)) + dc, cam15 rebuilt from it, points += dp (NULL: no change);
 *   the problem is in bal mode afterwards (apply_step(p, NULL, NULL) takes a state-mode problem there), and every
 *   cache of the cameras and points is dropped. */
typedef struct {
    int32_t iterations, status;
    double rel_residual, sum_sq, model_decrease;
} c2b_step_info;
int c2b_problem_solve_step(c2b_problem *p, double lambda, int max_iters, double rel_tol, double *dc, double *dp, c2b_step_info *info);
int c2b_problem_apply_step(c2b_problem *p, const double *dc, const double *dp);

/* ---- robust losses in the step: iteratively reweighted least squares ----
 * Per observation s = r0^2 + r1^2, a loss rho(s) with scale a > 0 (Ceres' definitions) and the weight w = rho'(s):
 *   kind 0 squared:  rho = s                                              w = 1
 *   kind 1 Huber:    rho = s (s <= a^2), else 2 a sqrt(s) - a^2           w = 1 (s <= a^2), else a / sqrt(s)
 *   kind 2 Cauchy:   rho = a^2 log1p(s / a^2)                             w = 1 / (1 + s / a^2)
 *   kind 3 soft-L1:  rho = 2 a^2 (sqrt(1 + s / a^2) - 1)                  w = 1 / sqrt(1 + s / a^2)
 * Every pass that uses (r, Jc, Jp) of an observation uses sqrt(w) (r, Jc, Jp) instead, w taken at the current state and
 * held for the whole solve: U = sum w Jc^T Jc, gc = sum w Jc^T r, V, gp, W, the damping diagonal, the preconditioner, b,
 * the back-substitution and the model decrease all follow from that one substitution.  No second-order (Triggs) term: H
 * stays positive semi-definite.  w is recomputed per observation from r: there is no weight array.  0 < w <= 1, and
 * s = 0 gives w = 1 in every kind.
 * _set_loss / _get_loss: the loss is the handle's state (default kind 0); it survives uploads, reads and culls.  kind
 *   outside 0..3, or (kind != 0) a scale that is not finite or <= 0: C2B_ERR_INVALID_ARGUMENT; kind 0 ignores the scale.
 *   c2b_problem_normal_equations and c2b_problem_solve_step honour it: under a loss U, gc, V, gp are the reweighted
 *   blocks, and sum_sq (both entries) and c2b_step_info.model_decrease are the weighted sum w |r|^2 and
 *   sum -w (2r + e).e the step modelled.  With kind 0 both entries launch the squared-loss kernels, bit for bit.
 * _robust_cost: sum rho(s) at the current state under the problem's loss (kind 0: sum |r|^2), one projection per
 *   observation, summed in a fixed order -- what a loop under a loss minimises (not sum w s).  Synchronous.
 * The *_rows_loss entries are the Level-0 passes above with (kind, scale) before the stream; kind 0 is the plain entry. */
int c2b_problem_set_loss(c2b_problem *p, int kind, double scale);
int c2b_problem_get_loss(const c2b_problem *p, int *kind, double *scale);
int c2b_problem_robust_cost(c2b_problem *p, double *cost);
int c2b_normal_cameras_rows_loss(const double *camblk, const double *pts4, const uint64_t *row_ptr, int64_t n_cam,
                                 const uint32_t *pt_idx, const double *uv_obs, int64_t n_obs, double *U, double *gc,
                                 void *workspace, double *sum_sq, int kind, double scale, void *stream);
int c2b_normal_points_rows_loss(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr,
                                const uint32_t *obs_of, const uint32_t *cam_of, const double *uv_obs, double *V, double *gp,
                                int kind, double scale, void *stream);
int c2b_schur_points_rows_loss(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr,
                               const uint32_t *obs_of, const uint32_t *cam_of, const double *uv_obs, const double *V, double lambda,
                               const double *x_cam, const double *h_pts, double *t_pts, int kind, double scale, void *stream);
int c2b_schur_cameras_rows_loss(const double *camblk, const double *pts4, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx,
                                const double *uv_obs, int64_t n_obs, const double *U, double lambda, const double *x_cam,
                                const double *t_pts, double *y_cam, int kind, double scale, void *stream);

/* ---- the preconditioner of the step: block-Jacobi on U (default) or Schur-Jacobi ----
 * Schur-Jacobi: per camera, with d_c the damping diagonal of U_c (the clamp rule above) and w_o the loss's weight,
 *   M_c = lambda diag(d_c) + sum_o w_o Jc_o^T (I2 - Jp_o V_l,p(o)^-1 Jp_o^T) Jc_o       over the camera's list,
 * the 9x9 diagonal block of S = U_l - W V_l^-1 W^T whenever no camera sees a point twice.  With a duplicated (camera,
 * point) pair it is not that block, but every term is positive semi-definite, so M_c stays symmetric positive definite;
 * the sum is accumulated in that form (nothing is subtracted from U_l).  M_c replaces U_l,c as the 9x9 block the PCG
 * factors and applies: the iterations are the same kernels, and the solution of S dc = b is the same.
 * _set_preconditioner / _get_preconditioner: the handle's state like the loss (default C2B_PRECOND_BLOCK_JACOBI); it
 *   survives uploads, reads and culls.  Another kind: C2B_ERR_INVALID_ARGUMENT.  c2b_problem_solve_step honours it: with
 *   kind 0 it launches exactly what it launched before this entry existed, bit for bit; with kind 1 the set-up runs one
 *   more pass over the observations (M, in a buffer of n_cam x 81 doubles the problem then keeps with the others) and
 *   factors M_c.  A camera whose M_c has a pivot that is not finite or not > 0 falls back to U_l,c's factor.
 * _preconditioner_fallbacks: how many cameras fell back in the last c2b_problem_solve_step; 0 after a block-Jacobi solve.
 * _schur_jacobi_rows(_loss): the Level-0 pass, asynchronous on `stream`: the inputs of c2b_schur_cameras_rows that it
 *   needs plus V [n_pts][3][3]; U and V are those c2b_normal_*_rows filled (under the same loss).  Output M [n_cam][9][9],
 *   both triangles the same bits.  Deterministic. */
#define C2B_PRECOND_BLOCK_JACOBI 0
#define C2B_PRECOND_SCHUR_JACOBI 1
int c2b_problem_set_preconditioner(c2b_problem *p, int kind);
int c2b_problem_get_preconditioner(const c2b_problem *p, int *kind);
int c2b_problem_preconditioner_fallbacks(const c2b_problem *p, int64_t *n);
int c2b_schur_jacobi_rows(const double *camblk, const double *pts4, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx,
                          const double *uv_obs, int64_t n_obs, const double *U, const double *V, double lambda, double *M,
                          void *stream);
int c2b_schur_jacobi_rows_loss(const double *camblk, const double *pts4, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx,
                               const double *uv_obs, int64_t n_obs, const double *U, const double *V, double lambda, double *M,
                               int kind, double scale, void *stream);

/* ---- constant camera parameters and points in the step ----
 * A camera's mask has bit k set when its parameter k is held constant, k in to_vec order (the columns of Jc):
 * w0 w1 w2 t0 t1 t2 f k1 k2; a point's mask is 1 when the whole point is.  With a mask in force c2b_problem_normal_equations
 * and c2b_problem_solve_step return what they are specified to return, computed from J~ in place of J: J with column k of
 * Jc_o zero for every observation o of a camera with bit k set, and Jp_o zero for every observation of a constant point.
 * So the constant rows and columns of U, and those entries of gc, are 0, V and gp of a constant point are 0, their damped
 * diagonals are lambda 1e-6 (the clamp rule), S, b and both preconditioners are those of J~, and every constant entry of
 * dc and every row of dp of a constant point compares == 0.0 -- at every iterate, for every max_iters, under every
 * status.  The free parameters get the step of the problem in which the constant ones cannot move, which is not the
 * unmasked step with entries overwritten.  sum_sq does not change (the mask does not touch r, nor a loss's weights);
 * model_decrease is summed from J, which equals the sum from J~ on a step with those zeros.  Every camera constant: b = 0,
 * 0 iterations, status 0, dp = -V_l^-1 gp.  Every point constant: S = U_l.  c2b_problem_apply_step adds the step to the
 * free entries only: constant entries of bal9 (state mode: of to_vec(cam15)) and constant points keep their bits.
 * _set_constant: cam_mask [n_cam] (uint16_t words) and pt_mask [n_pts] are HOST arrays; either may be NULL (none of that
 *   kind constant), both NULL clears the masks; an all-zero mask is no mask.  A bit above bit 8, or a pt_mask value other
 *   than 0 or 1: C2B_ERR_INVALID_ARGUMENT, and the masks in force stay.  With none in force both entries launch exactly
 *   what they launch without this entry, bit for bit.  Deterministic with a mask as without.
 * _get_constant: the masks in force (zeros when none) and how many camera parameters / points they hold; any output may
 *   be NULL.
 * Lifetime: the masks are the handle's state.  They survive c2b_problem_apply_step, the noise functions, _set_loss,
 *   _set_preconditioner, _adopt_visibility and an upload that keeps both n_cam and n_pts (the entities are then taken to
 *   be the same ones).  Whatever changes a count or renumbers the entities drops them: a cull (_cull,
 *   _largest_connected_component, _remove_singletons), a read, a generator, an upload of another size. */
#define C2B_CONST_ROTATION 0x007
#define C2B_CONST_TRANSLATION 0x038
#define C2B_CONST_POSE 0x03f
#define C2B_CONST_FOCAL 0x040
#define C2B_CONST_K1 0x080
#define C2B_CONST_K2 0x100
#define C2B_CONST_INTRINSICS 0x1c0
#define C2B_CONST_ALL 0x1ff
typedef uint16_t c2b_camera_mask;      /* a camera's word: an OR of C2B_CONST_* bits */
int c2b_problem_set_constant(c2b_problem *p, const c2b_camera_mask *cam_mask, const uint8_t *pt_mask);
int c2b_problem_get_constant(const c2b_problem *p, c2b_camera_mask *cam_mask, uint8_t *pt_mask, int64_t *n_const_cam_params,
                             int64_t *n_const_pts);

/* ---- priors on camera centres, intrinsics and points in the step ----
 * Optional residual rows beside the observations' (costs are sums of squares without a 1/2, g = J^T r):
 *   camera c:  r_C = w_C o (C - C0), C = -R^T t the world-frame centre (3 rows);  r_I = w_I o ((f, k1, k2) - I0) (3 rows)
 *   point p:   r_X = w_X o (X - X0) (3 rows)
 * Weights are per component, finite and >= 0: 1 / sigma in units of the observations' standard deviation.  A weight of 0
 * switches its row off, and its target is then ignored and may be anything.  No robust loss reweights a prior.  The stacked
 * objective is (sum |r_obs|^2, or sum rho(|r_obs|^2)) + sum |r_prior|^2.  With the left-Jacobian convention of the Jacobian's
 * rotation columns, dC/dw = -R^T [t]x J_l(w) and dC/dt = -R^T, from the camera's camblk record (so the prior refers to the w
 * of the mode the problem is in); A = the 6x9 stack diag(w_C) [dC/dw | -R^T | 0], [0 | 0 | diag(w_I)].
 * With priors in force c2b_problem_normal_equations and c2b_problem_solve_step are those of the stacked system: U_c += A^T A,
 * gc_c += A^T r, V_p += diag(w_X^2), gp_p += w_X o r_X, added after the observations' passes and before the constant
 * parameters' zeros (a constant parameter's prior column is zeroed like any other); the damping's diagonal, S, b, both
 * preconditioners, sum_sq (+ sum |r_prior|^2) and model_decrease (+ sum |r_prior|^2 - |r_prior + A delta|^2) follow.
 * c2b_problem_levenberg_marquardt's cost is the observations' cost + c2b_problem_prior_cost, added in that order.
 * c2b_problem_total_reprojection_error, c2b_problem_robust_cost and c2b_problem_filter_observations stay observation-only.
 * _set_priors: six HOST arrays of [n][3] doubles; a (target, weights) pair may be NULL (no prior of that kind), all NULL
 *   clears the priors; a pair whose weights are all 0 is no prior.  A target without its weights (or the reverse), a negative
 *   or non-finite weight, a non-finite target under a positive weight, or a shard: C2B_ERR_INVALID_ARGUMENT, and the priors
 *   in force stay.  With none in force every entry launches and allocates exactly what it does without this entry.
 * _get_priors: the arrays in force (zeros for a kind with none) and how many cameras / cameras / points have a centre / an
 *   intrinsics / a point row with a positive weight; any output may be NULL.
 * _prior_cost: sum |r_prior|^2 at the current state (the cameras' sum + the points' sum); 0 without priors.
 * _prior_residual_jacobian: HOST out-buffers (any may be NULL), synchronous: r_cam [n_cam][6] = (r_C, r_I), A_cam [n_cam][3][6]
 *   = diag(w_C) [dC/dw | -R^T], r_pt [n_pts][3]; zeros where no prior is in force.
 * Lifetime: as the constant masks -- kept by c2b_problem_apply_step, the noise functions, _set_loss, _set_preconditioner,
 *   _set_constant, checkpoint and rollback and an upload of the same counts; dropped by a cull, a read, a generator, an
 *   upload of another size.
 * Limits: priors in force and no observation at all: c2b_problem_solve_step and c2b_problem_levenberg_marquardt return
 *   C2B_ERR_INVALID_ARGUMENT.  A camera with an empty row and a prior is ordinary: its block is the prior alone.
 * Level 0, asynchronous on `stream`, device pointers, (target, weights) pairs [n][3] NULL together:
 * _prior_cameras_rows: U [n_cam][9][9] += A^T A, gc [n_cam][9] += A^T r (either may be NULL: U may be the Schur-Jacobi M);
 *   r [n_cam][6] and A [n_cam][3][6] (may be NULL) are written for every camera; part (may be NULL) takes one cost partial
 *   per 256 rows of blocks, ceil(9 n_cam / 256) doubles, and cost (may be NULL, needs part) their sum in a fixed order.
 * _prior_points_rows: V [n_pts][3][3] += diag(w_X^2), gp [n_pts][3] += w_X o r_X (both may be NULL), r [n_pts][3], part
 *   [ceil(n_pts / 256)], cost likewise.
 * _prior_model_rows: sums[0] = sum |r_prior|^2, sums[1] = sum (|r_prior|^2 - |r_prior + A delta|^2) for the step dc [n_cam][9],
 *   dp [n_pts][3]; part_sq, part_md: ceil(max(n_cam, n_pts) / 256) doubles each.
 * Deterministic: no float atomics; the same inputs give the same bits. */
int c2b_problem_set_priors(c2b_problem *p, const double *cam_center, const double *cam_center_w, const double *cam_intr,
                           const double *cam_intr_w, const double *pt, const double *pt_w);
int c2b_problem_get_priors(const c2b_problem *p, double *cam_center, double *cam_center_w, double *cam_intr, double *cam_intr_w,
                           double *pt, double *pt_w, int64_t *n_center_rows, int64_t *n_intr_rows, int64_t *n_pt_rows);
int c2b_problem_prior_cost(c2b_problem *p, double *cost);
int c2b_problem_prior_residual_jacobian(c2b_problem *p, double *r_cam, double *A_cam, double *r_pt);
int c2b_prior_cameras_rows(const double *camblk, int64_t n_cam, const double *center, const double *center_w, const double *intr,
                           const double *intr_w, double *U, double *gc, double *r, double *A, double *part, double *cost, void *stream);
int c2b_prior_points_rows(const double *pts4, int64_t n_pts, const double *pt, const double *pt_w, double *V, double *gp, double *r,
                          double *part, double *cost, void *stream);
int c2b_prior_model_rows(const double *camblk, int64_t n_cam, const double *center, const double *center_w, const double *intr,
                         const double *intr_w, const double *pts4, int64_t n_pts, const double *pt, const double *pt_w,
                         const double *dc, const double *dp, double *part_sq, double *part_md, double *sums, void *stream);

/* ---- the Levenberg-Marquardt loop on the device: checkpoint, stopping tests ----
 * _checkpoint: takes the problem to bal mode exactly as c2b_problem_apply_step(p, NULL, NULL) does and copies bal9 and the
 *   points into two device buffers the problem owns (allocated on first use, reused while the counts stay).  Device to
 *   device on the problem's stream; no host memory is touched.
 * _rollback: copies them back, rebuilds the in-memory cameras from bal9 by the kernel that built them (the same bits) and
 *   drops the cameras' derived tables.  The row structure, the transpose, the tile records, the solve buffers' allocation,
 *   the loss, the preconditioner and the masks stay.  Without a checkpoint: C2B_ERR_INVALID_ARGUMENT.
 * Lifetime: the checkpoint survives c2b_problem_apply_step and the noise functions.  It is dropped by whatever drops the
 *   constant masks (a cull, a read, a generator, an upload of another size), by ANY upload, and by _drop_checkpoint.
 *   A problem with a shard set is refused, as in c2b_problem_solve_step.
 * _levenberg_marquardt: up to max_iterations iterations on the problem in place.  An iteration solves the damped step
 *   (c2b_problem_solve_step with pcg_max_iters, pcg_rel_tol) into scratch the problem keeps, applies it and keeps it when
 *   the cost falls.  Cost: c2b_problem_robust_cost under a loss, else the square of c2b_problem_total_reprojection_error
 *   (p, 2.0).  Gain ratio rho = (cost - cost_trial) / model_decrease when model_decrease > 0, else -1; accepted when
 *   rho > 0 and cost_trial < cost: lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; rejected: the state is rolled back,
 *   lambda *= nu, nu *= 2 (nu starts at 2); lambda is held in [C2B_STEP_LAMBDA_MIN, C2B_STEP_LAMBDA_MAX] throughout.
 *   Per iteration, in this order: solve; gradient_max = max(|gc|, |gp|) over the gradient the solve formed (exact; a NaN
 *   propagates), step_norm = |(dc, dp)|, x_norm = |(bal9, points)| (sums in a fixed order, no float atomics), and the
 *   iteration's entry is recorded; the gradient test; the parameter test; apply, cost, accept or roll back; after an
 *   accepted step the function test.  termination:
 *     0  max_iterations reached
 *     1  function: cost - cost_trial <= function_tol cost, after an accepted step (which is kept)
 *     2  gradient: gradient_max <= gradient_tol at the state the step was solved at (the step is not applied)
 *     3  parameter: step_norm <= parameter_tol (x_norm + parameter_tol) (the step is not applied)
 *     4  the cost or the gradient is not finite; the state is the last accepted one
 *   A tolerance of 0 disables its test.  An entry's cost_trial repeats cost when its step was not applied.  history (may
 *   be NULL) takes one entry per iteration and needs capacity >= max_iterations; summary may be NULL.  Negative or
 *   non-finite tolerances, max_iterations or pcg_max_iters < 0, lambda0 outside the damping range, capacity too small:
 *   C2B_ERR_INVALID_ARGUMENT.  The loss, the preconditioner and the masks are the handle's and are honoured as
 *   c2b_problem_solve_step honours them.  The checkpoint is the loop's: none is left on return.  Deterministic. */
typedef struct {
    int32_t max_iterations, pcg_max_iters;
    double lambda0, pcg_rel_tol, function_tol, gradient_tol, parameter_tol;
} c2b_lm_options;
typedef struct {
    double cost, cost_trial, lambda, model_decrease, gradient_max, step_norm, x_norm, pcg_rel_residual;
    int32_t accepted, pcg_iterations, status, reserved;
} c2b_lm_iteration;
typedef struct {
    int32_t iterations, termination;
    double initial_cost, final_cost, lambda_next;
} c2b_lm_summary;
int c2b_problem_checkpoint(c2b_problem *p);
int c2b_problem_rollback(c2b_problem *p);
int c2b_problem_drop_checkpoint(c2b_problem *p);
int c2b_problem_levenberg_marquardt(c2b_problem *p, const c2b_lm_options *opt, c2b_lm_iteration *history, int capacity,
                                    c2b_lm_summary *summary);

/* ---- outlier rejection: drop the observations whose reprojection residual is large, in place ----
 * Per observation, with (u, v) what c2b_project gives for it (the same bits) and q the point in its camera's frame:
 *   du = u - obs.x; dv = v - obs.y; r2 = du * du + dv * dv;        (five operations, none fused)
 *   keep = r2 <= max_error * max_error && (!(flags & C2B_FILTER_IN_FRONT) || q.z < 0)
 * max_error is squared once on the host, in double.  A residual that is NaN compares false and is dropped, and so does an
 * infinite one against every finite max_error.  max_error = +inf keeps every finite residual (and, since inf <= inf, an
 * infinite r2 too: only NaN goes).  max_error negative or NaN, or a flag bit other than C2B_FILTER_IN_FRONT:
 * C2B_ERR_INVALID_ARGUMENT.
 * c2b_residual_keep_rows: Level 0, stateless, asynchronous on `stream`: the inputs of c2b_reprojection_error_sum_rows,
 *   keep [n_obs] one byte (0 / 1) per observation.
 * c2b_problem_filter_observations: Level 1, synchronous.  The problem's list is compacted by that mask in place: the
 *   survivors keep their order inside every camera's row (deterministic), n_obs falls, and everything derived from the
 *   list (row structure, transpose, solve buffers) is rebuilt by its next user.  Cameras, points and both counts stay --
 *   nothing is renumbered -- and with them the constant masks, the loss, the preconditioner, the checkpoint and the LM
 *   loop's scratch.  A filter can leave a camera or a point with too few observations: c2b_problem_cull is the caller's
 *   call.  *n_removed (may be NULL) = how many went; when it is 0 the call changed nothing at all and dropped no cache.
 *   A problem without observations returns 0.  A problem with a shard set is refused, and so is every bad argument, with
 *   the problem unchanged. */
#define C2B_FILTER_IN_FRONT 1
int c2b_residual_keep_rows(const double *camblk, const double *pts4, const uint64_t *row_ptr, int64_t n_cam, const void *tiles,
                           const uint32_t *pt_idx, const double *uv_obs, int64_t n_obs, double max_error, int flags, uint8_t *keep,
                           void *stream);
int c2b_problem_filter_observations(c2b_problem *p, double max_error, int flags, int64_t *n_removed);

/* ---- triangulation: points from cameras and observations (linear midpoint, one lane per point) ----
 * Point p's observations are walked in ascending observation index through the point-major transpose (pt_row_ptr / obs_of /
 * cam_of of c2b_normal_transpose).  Per observation of camera c, observed (u, v), with f, k1, k2, R, t of its camblk record
 * and its centre C (record doubles 24..26, the centre of the visibility predicate):
 *   m = (u, v) / f; rd = |m|; rho >= 0 with rho (1 + k1 rho^2 + k2 rho^4) = rd, by Newton from rho = rd, at most 16
 *   iterations, stopping when the update leaves rho unchanged (k1 == 0 && k2 == 0: rho = rd exactly, no iteration);
 *   pn = m rho / rd (0 when rd == 0); the projection is p = -q.xy / q.z with the scene at q.z < 0, so the ray in the camera
 *   frame is (pn.x, pn.y, -1) and d = R^T ray, normalised, is its direction in the world;
 *   A += I - d d^T; b += (I - d d^T) C; n_used += 1.
 * The observation is unusable, and skipped, when f is 0 or not finite, when the derivative 1 + 3 k1 rho^2 + 5 k2 rho^4 is
 * <= 0 at an iterate, or when rho is not finite.  Then, in this order:
 *   C2B_TRI_CONSTANT   the point is constant under pt_mask / c2b_problem_set_constant; none of its observations is read;
 *   C2B_TRI_TOO_FEW    n_used < 2;
 *   C2B_TRI_DEGENERATE lambda_min(A) < 1 - cos(min_angle) (for two rays exactly "less than min_angle apart"; more rays only
 *                      raise lambda_min), or the 3x3 Cholesky of A fails, or X = A^-1 b is not finite.  lambda_min is
 *                      n_used - lambda_max(sum d d^T) in closed form; the threshold is evaluated once on the host as
 *                      2 sin^2(min_angle / 2);
 *   C2B_TRI_BEHIND     a usable observation's camera sees X at q.z >= 0 (a second walk over the row);
 *   C2B_TRI_OK         pts4[p].xyz = X; the fourth lane keeps its value.
 * A point whose status is not C2B_TRI_OK keeps its bits.  No robust loss enters: the loss on the handle is ignored.  The
 * sums of a point depend on its own list alone and there are no float atomics: the same inputs give the same bits.  The
 * pass uses no scratch memory.  min_angle is in radians; negative, NaN or > pi/2: C2B_ERR_INVALID_ARGUMENT.
 * c2b_triangulate_rows: Level 0, stateless, asynchronous on `stream`.  pts4 [n_pts][4] is updated in place; pt_mask (device,
 *   [n_pts] 0 / 1) may be NULL; status [n_pts] one byte per point; counts [5] (device int64, indexed by status) is zeroed
 *   and then summed by integer atomics.  camblk, obs_of, cam_of and uv_obs are read only where a row holds an observation.
 * c2b_problem_triangulate_points: Level 1, synchronous.  The resident points are triangulated from the resident cameras,
 *   read in the mode the problem is in (bal or state; the mode does not change), over the problem's cached transpose,
 *   which is built as c2b_problem_solve_step builds it when absent.  status (host, [n_pts]) and counts (host, [5]) may be
 *   NULL.  Only the points change, as after c2b_problem_apply_step with a point step: the list, the row structure, the
 *   transpose, the solve buffers, the constant masks, the loss, the preconditioner and a checkpoint all stay.  A problem
 *   without observations returns C2B_TRI_TOO_FEW for every point and writes nothing.  A problem with a shard set is
 *   refused, and so is every bad argument, with the problem unchanged. */
#define C2B_TRI_OK 0
#define C2B_TRI_TOO_FEW 1
#define C2B_TRI_DEGENERATE 2
#define C2B_TRI_BEHIND 3
#define C2B_TRI_CONSTANT 4
int c2b_triangulate_rows(const double *camblk, double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                         const uint32_t *cam_of, const double *uv_obs, double min_angle, const uint8_t *pt_mask, uint8_t *status,
                         int64_t *counts, void *stream);
int c2b_problem_triangulate_points(c2b_problem *p, double min_angle, uint8_t *status, int64_t *counts);

/* ---- per-point Levenberg-Marquardt: every point refined by itself, the cameras held (one lane per point) ----
 * Point p's observations are walked in ascending observation index through the point-major transpose, as triangulation
 * walks them.  A walk evaluates at one position X, all in registers:
 *   F = sum_o rho(|r_o|^2) + |w_X o (X - X0)|^2     rho of the loss (kind 0: s itself), then the point prior, in that order;
 *   V = sum_o w Jp^T Jp + diag(w_X^2), g = sum_o w Jp^T r + w_X o r_X, w = rho'(|r_o|^2) at X (IRLS): r and Jp are those of
 *   the step kernel, scaled by sqrt(w) before the products as every weighted pass scales them.
 * A prior component of weight 0 contributes nothing and its target is never read (it may be NaN).  Walk 0 is at the start.
 * Round k, per point, with mu = lambda0 and nu = 2 at the start:
 *   the gradient test: max |g_i| <= gradient_tol -> converged;
 *   (V + mu diag(d)) delta = -g by the 3x3 Cholesky, d_i = min(max(V_ii, 1e-6), 1e32); a pivot <= 0 or a non-finite delta
 *     is a rejection (below);
 *   the parameter test: |delta| <= parameter_tol (|X| + parameter_tol) -> converged, the step not applied;
 *   a walk at X + delta gives F', V', g'; model = -(2 g.delta + delta^T V delta); gain = (F - F') / model if model > 0, else -1;
 *   accepted iff gain > 0, F' < F and F' is finite: X, F, V, g become the trial's, mu *= max(1/3, 1 - (2 gain - 1)^3),
 *     nu = 2, and the function test: F - F' <= function_tol F -> converged;
 *   rejected: mu *= nu, nu *= 2.  mu is held in [C2B_STEP_LAMBDA_MIN, C2B_STEP_LAMBDA_MAX].
 * A tolerance of 0 disables its test.  Status, one byte per point:
 *   C2B_REFINE_CONVERGED   a tolerance test was met;
 *   C2B_REFINE_MAX_ROUNDS  max_rounds rounds were run (max_rounds = 0: no round at all, nothing moves);
 *   C2B_REFINE_UNOBSERVED  no observation and no prior weight; untouched;
 *   C2B_REFINE_FAILED      the start cost is not finite; untouched;
 *   C2B_REFINE_CONSTANT    constant under pt_mask / c2b_problem_set_constant; nothing of it is read; untouched.
 * pts4[p].xyz is written only if the point's cost fell strictly; the fourth lane keeps its value.  counts [6]: the five
 * statuses, then `moved`, the number of points written.  A point's result depends on its own list, its cameras and the
 * options alone; there are no float atomics: the same inputs give the same bits.  The pass uses no scratch memory.
 * max_rounds < 0, reserved != 0, lambda0 outside the damping range, a negative or non-finite tolerance:
 * C2B_ERR_INVALID_ARGUMENT.
 * c2b_refine_points_rows: Level 0, stateless, asynchronous on `stream`.  The arguments of c2b_triangulate_rows; loss_a2 is
 *   the loss's squared scale (ignored for kind 0); prior_pt / prior_pt_w (device, [n_pts][3], in pairs) and pt_mask may be
 *   NULL; counts [6] (device int64) is zeroed and then summed by integer atomics.
 * c2b_problem_refine_points: Level 1, synchronous, with the preconditions and the cache story of
 *   c2b_problem_triangulate_points: the resident cameras in the mode the problem is in, the cached transpose (built when
 *   absent), only the points change, a shard is refused.  It honours the handle's loss, point mask and point priors; the
 *   list, the row structure, the transpose, the solve buffers, the masks, the loss, the preconditioner, the priors and a
 *   checkpoint all stay.  status (host, [n_pts]) and counts (host, [6]) may be NULL.  With no observation at all every
 *   unmasked point without a prior is C2B_REFINE_UNOBSERVED.
 * c2b_problem_set_inner_iterations: the handle's state, with the lifetime of the loss.  With rounds > 0 the loop of
 *   c2b_problem_levenberg_marquardt calls c2b_problem_refine_points with {rounds, 0, 1e-4, 0, 0, 0} directly after it
 *   applied a step and before it takes the trial cost (Ceres' inner iterations with the points as the inner block):
 *   cost_trial is the cost after the refinement, so the gain ratio may exceed 1; acceptance, the lambda update and the
 *   rollback are otherwise unchanged, and a rejected step rolls the points back through the checkpoint.  rounds = 0 (the
 *   default) issues exactly the launches the loop issued without it.  rounds < 0: C2B_ERR_INVALID_ARGUMENT. */
#define C2B_REFINE_CONVERGED 0
#define C2B_REFINE_MAX_ROUNDS 1
#define C2B_REFINE_UNOBSERVED 2
#define C2B_REFINE_FAILED 3
#define C2B_REFINE_CONSTANT 4
typedef struct {
    int32_t max_rounds, reserved;
    double lambda0, function_tol, gradient_tol, parameter_tol;
} c2b_refine_options;
int c2b_refine_points_rows(const double *camblk, double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                           const uint32_t *cam_of, const double *uv_obs, int loss_kind, double loss_a2, const double *prior_pt,
                           const double *prior_pt_w, const c2b_refine_options *opt, const uint8_t *pt_mask, uint8_t *status,
                           int64_t *counts, void *stream);
int c2b_problem_refine_points(c2b_problem *p, const c2b_refine_options *opt, uint8_t *status, int64_t *counts);
int c2b_problem_set_inner_iterations(c2b_problem *p, int rounds);
int c2b_problem_get_inner_iterations(c2b_problem *p, int *rounds);

/* ---- per-camera Levenberg-Marquardt: every camera re-minimised by itself, the points held (motion-only bundle adjustment) ----
 * The dual of c2b_refine_points_rows, with its options, statuses and counts, and its rule set with 9 for 3.  The parameters are
 * q = bal9[c][0..8] (to_vec order: w0 w1 w2 t0 t1 t2 f k1 k2).  For every walk the camera's record is formed from q as
 * c2b_camblk_from_bal forms it; a step is q + delta on the free entries, what c2b_problem_apply_step does to bal9.  A walk at q:
 *   F = sum_o rho(|r_o|^2) + |w_C o (C - C0)|^2 + |w_I o ((f, k1, k2) - I0)|^2     observations, centre prior, intrinsics prior;
 *   U = sum_o w Jc^T Jc + A^T A (9x9), g = sum_o w Jc^T r + A^T r_prior, w = rho'(|r_o|^2) at q: r and Jc scaled by sqrt(w)
 *   before the products; A is the prior Jacobian of c2b_prior_cameras_rows.  A prior component of weight 0 never reads its target.
 *   Then the rows and columns of U and the entries of g of the constant parameters (cam_mask bit k = parameter k) are zeroed;
 *   F is not masked.  Sixteen lanes own a camera: lane l sums observations b + l, b + l + 16, ... of the camera's row, then a
 *   fixed xor tree.  At walk 0, U and g are the bits c2b_problem_normal_equations gives for a handle that holds the same bal9.
 * Round k, per camera, with mu = lambda0 and nu = 2 at the start:
 *   the gradient test: max |g_i| <= gradient_tol -> converged;
 *   (U + mu diag(d)) delta = -g by the 9x9 Cholesky of the step's preconditioner, d_i = min(max(U_ii, 1e-6), 1e32); a pivot
 *     <= 0 or a non-finite delta is a rejection; a constant entry's delta compares == 0;
 *   the parameter test: |delta| <= parameter_tol (|q| + parameter_tol) -> converged, the step not applied;
 *   a walk at q + delta gives F', U', g'; model = -(2 g.delta + delta^T U delta); gain = (F - F') / model if model > 0, else -1;
 *   accepted iff gain > 0, F' < F and F' is finite: q, F, U, g become the trial's, mu *= max(1/3, 1 - (2 gain - 1)^3),
 *     nu = 2, and the function test: F - F' <= function_tol F -> converged;
 *   rejected: mu *= nu, nu *= 2.  mu is held in [C2B_STEP_LAMBDA_MIN, C2B_STEP_LAMBDA_MAX].
 * Status, one byte per camera: C2B_REFINE_CONSTANT all nine mask bits set (nothing of the camera is read);
 * C2B_REFINE_UNOBSERVED an empty row and no prior weight; C2B_REFINE_FAILED the start cost is not finite; C2B_REFINE_CONVERGED;
 * C2B_REFINE_MAX_ROUNDS.  bal9[c] is written only if the camera's cost fell strictly, and its constant entries are not
 * rewritten.  counts [6]: the five statuses, then `moved`.  No float atomics, no scratch memory: a camera's result depends on
 * its own row, its points and the options alone.  Bad options: C2B_ERR_INVALID_ARGUMENT, as c2b_refine_points_rows.
 * c2b_refine_cameras_rows: Level 0, stateless, asynchronous on `stream`.  bal9 [n_cam][9] in place; pts4, row_ptr [n_cam + 1],
 *   pt_idx, uv_obs as c2b_resect_rows takes them (pts4, pt_idx and uv_obs are read only for a non-empty row); loss_a2 is the
 *   loss's squared scale (ignored for kind 0); the prior arrays (device, [n_cam][3], in pairs) in c2b_prior_cameras_rows'
 *   layout; the priors, cam_mask and status may be NULL; counts [6] (device int64) is zeroed and then summed by integer atomics.
 * c2b_problem_refine_cameras: Level 1, synchronous, in c2b_problem_resect_cameras' shape: the row structure (built when absent),
 *   bal9 made the truth (to_vec of the cameras first in state mode), the pass under the handle's loss, camera mask, centre and
 *   intrinsics priors, the cameras rebuilt from bal9: the problem is in bal mode afterwards.  The list, the row structure, the
 *   transpose, the solve buffers, the masks, the loss, the preconditioner, the priors and a checkpoint all stay.  A shard is
 *   refused.  status (host, [n_cam]) and counts (host, [6]) may be NULL.  With no observation at all every unmasked camera
 *   without a prior weight is C2B_REFINE_UNOBSERVED, and one with a prior is pulled towards its target. */
int c2b_refine_cameras_rows(double *bal9, const double *pts4, int64_t n_cam, const uint64_t *row_ptr, const uint32_t *pt_idx,
                            const double *uv_obs, int loss_kind, double loss_a2, const double *prior_center, const double *prior_center_w,
                            const double *prior_intr, const double *prior_intr_w, const c2b_refine_options *opt, const c2b_camera_mask *cam_mask,
                            uint8_t *status, int64_t *counts, void *stream);
int c2b_problem_refine_cameras(c2b_problem *p, const c2b_refine_options *opt, uint8_t *status, int64_t *counts);

/* ---- consensus triangulation: points from the rays that agree (two-ray hypotheses, inlier mask, refit) ----
 * c2b_triangulate_rows is a least-squares midpoint over every ray of a point: one ray that belongs to another point (a
 * wrong match, a joined landmark) drags it arbitrarily far.  This pass forms candidates from pairs of rays, keeps the
 * candidate most of the row agrees with, and refits on those.  Notation as above: point p's row of the transpose in
 * ascending observation index, usable(o) as defined there, thr = 2 sin^2(min_angle / 2) and E2 = max_error * max_error each
 * formed once on the host.  One wave per point.  In this order:
 *   C2B_TRI_CONSTANT     the point is constant under pt_mask; nothing of its row is read.
 *   sample               the usable observations among the FIRST 64 ENTRIES of the row, in row order, numbered 0 .. m - 1.
 *   C2B_TRI_TOO_FEW      m < 2 (or fewer than two usable observations in the whole row, which m < 2 implies).
 *   hypotheses           pair number k = 0, 1, ...: the gap g runs from floor(m / 2) down to 1 and, per gap, i over 0 .. m - 1
 *                        (when 2 g == m only i < g: each pair once); the pair is (i, (i + g) mod m), lower index first.  The
 *                        enumeration stops after max_hypotheses pairs, 1 <= max_hypotheses <= 64.  Hypothesis k is formed
 *                        iff c2b_triangulate_rows' own arithmetic on those two observations alone (the same sums, lower
 *                        index first, the same lambda_min and Cholesky) passes that pass's test lambda_min >= thr && solved;
 *                        X_k is that solution.  Cheirality is not tested here.
 *   C2B_TRI_DEGENERATE   no hypothesis is formed.
 *   score                observation o of the row -- every entry, also past the 64th, also the pair itself -- is an inlier
 *                        of X iff it is usable and c2b_residual_keep_rows with C2B_FILTER_IN_FRONT would keep it at X: with
 *                        (u, v) and q.z of c2b_project at X, du = u - obs.x, dv = v - obs.y, du * du + dv * dv <= E2 (five
 *                        unfused operations; NaN compares false) and q.z < 0.  The score of k is its integer inlier count.
 *   select               the highest score, the LOWEST k among equal scores; I* is its inlier set.
 *   C2B_TRI_NO_CONSENSUS |I*| < min_inliers (min_inliers >= 2).
 *   refit                A, b over I* in ascending row order by c2b_triangulate_rows' expressions and Cholesky:
 *   C2B_TRI_DEGENERATE   lambda_min(A) < thr or not solved;
 *   C2B_TRI_BEHIND       some inlier's camera sees X at q.z >= 0;
 *   C2B_TRI_OK           pts4[p].xyz = X, the fourth lane keeps its value: bit for bit what c2b_triangulate_rows returns
 *                        on the list restricted to I*.
 * A point whose status is not C2B_TRI_OK keeps its bits.  Per point also hyp = the selected k and n_inl = |I*| (set once a
 * hypothesis was selected, whatever the status after it; -1 and 0 under CONSTANT, TOO_FEW and when none was formed).  Per
 * observation, indexed as the camera-major list: inlier[o] = 0 for the observations of a C2B_TRI_OK point that are not in
 * I* (the unusable ones among them), 1 everywhere else -- nothing is claimed about a point that was not triangulated.
 * counts[6] is the histogram of the statuses.  No float atomics, no scratch memory, no workspace, no loss from the handle:
 * the same inputs give the same bits whatever the launch shape.  min_angle outside [0, pi/2] or NaN, max_error negative, NaN
 * or infinite, min_inliers < 2, max_hypotheses outside [1, 64], an unknown flag bit: C2B_ERR_INVALID_ARGUMENT.
 * c2b_triangulate_consensus_rows: Level 0, stateless, asynchronous on `stream`.  The arguments of c2b_triangulate_rows, and
 *   n_obs, the length of the list obs_of indexes; hyp, n_inl [n_pts] (device int32) and inlier [n_obs] (device, one byte)
 *   may each be NULL; counts [6] (device int64) is zeroed and inlier set to 1 before the kernel runs.
 * c2b_problem_triangulate_consensus: Level 1, synchronous, with the preconditions and the cache story of
 *   c2b_problem_triangulate_points: the resident cameras in the mode the problem is in, the cached transpose (built when
 *   absent), only the points change, a shard is refused, a problem without observations returns C2B_TRI_TOO_FEW for every
 *   point and launches nothing.  status [n_pts], hyp [n_pts], inlier [n_obs, in the list's order at call time] and counts [6]
 *   are host arrays and may be NULL.  flags = C2B_TRI_DROP_OUTLIERS: the list is then compacted by the inlier mask exactly
 *   as c2b_problem_filter_observations compacts by its mask (stable inside every camera's row, nothing renumbered, what was
 *   derived from the list is rebuilt by its next user); *n_removed (may be NULL) = how many went, and when it is 0 no cache
 *   is dropped.  Should the compaction fail (an allocation), the points have already moved and the list has not: the
 *   status, the mask and the counts returned describe the pass, and the call returns the error.  Every refusal leaves the
 *   problem unchanged. */
#define C2B_TRI_NO_CONSENSUS 5
#define C2B_TRI_DROP_OUTLIERS 1
int c2b_triangulate_consensus_rows(const double *camblk, double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                                   const uint32_t *cam_of, const double *uv_obs, int64_t n_obs, double min_angle, double max_error,
                                   int min_inliers, int max_hypotheses, const uint8_t *pt_mask, uint8_t *status, int32_t *hyp,
                                   int32_t *n_inl, uint8_t *inlier, int64_t *counts, void *stream);
int c2b_problem_triangulate_consensus(c2b_problem *p, double min_angle, double max_error, int min_inliers, int max_hypotheses, int flags,
                                      uint8_t *status, int32_t *hyp, uint8_t *inlier, int64_t *counts, int64_t *n_removed);

/* ---- resection: camera poses from points and observations (object-space error, one wave per camera) ----
 * The dual of triangulation: camera c's pose (R, t) from the points as they are, its f, k1, k2 kept.  The camera's row of
 * the camera-major list is walked in ascending order.  Per observation of point X, observed (u, v), with f, k1, k2 =
 * bal9[c][6..8]:
 *   the undistorted pixel pn exactly as triangulation forms it (m = (u, v) / f; Newton for rho (1 + k1 rho^2 + k2 rho^4) =
 *   |m| from rho = |m|, at most 16 iterations; pn = m rho / |m|), the same unusable cases, and also unusable when X is not
 *   finite; b = (pn.x, pn.y, -1) normalised, P = I - b b^T.
 * With Xbar the mean of the usable points and Y = X - Xbar, sixty sums are formed in row order: S0 = sum P, S1[a] = sum
 * Y_a P, S2[ac] = sum Y_a Y_c P (the upper triangles).  The object-space error sum |P (R Y + t')|^2 has t' = -S0^-1 sum_a
 * S1[a] R[:, a]; what remains is r^T M r with r[3 a + i] = R[i][a] and M[(a,i),(c,j)] = S2[ac][ij] - (S1[a] S0^-1 S1[c])_ij.
 * lambda_1 <= ... <= lambda_9 are M's eigenvalues (cyclic Jacobi), g the unit eigenvector of lambda_1, G[i][a] = g[3 a + i]
 * negated if det G < 0, R0 the rotation nearest G; then at most 8 Gauss-Newton iterations on r^T M r over R <- exp([d]x) R
 * (H = J^T M J, d = -H^-1 J^T M r, J = [vec([e_k]x R)]), stopping when |d| <= 1e-14; t = t'(R) - R Xbar.  In this order:
 *   C2B_RES_CONSTANT   the camera's mask word holds any of the six pose bits (C2B_CONST_POSE); none of its observations is read;
 *   C2B_RES_TOO_FEW    n_used < min_points;
 *   C2B_RES_DEGENERATE a pivot of S0's 3x3 Cholesky is not > 0; or an eigenvalue is not finite, lambda_2 < min_gap lambda_9
 *                      (coplanar points, too little spread; evaluated from the raw min_gap: 0 disables it) or lambda_1 >=
 *                      lambda_2 / 4 (noise swamps the gap); or H is not positive definite, or d, R or t is not finite;
 *   C2B_RES_BEHIND     a usable observation has (R X + t).z >= 0 (a second walk over the row);
 *   C2B_RES_OK         bal9[c][0..5] = (to_rodrigues(R), t); entries 6..8 keep their bits.
 * A camera whose status is not C2B_RES_OK keeps all nine.  No robust loss enters: the loss on the handle is ignored.  A
 * camera's result depends on its own row alone and there are no float atomics: the same inputs give the same bits.  The
 * pass uses no scratch memory.  min_points < 6, min_gap negative, NaN or >= 1: C2B_ERR_INVALID_ARGUMENT.
 * c2b_resect_rows: Level 0, stateless, asynchronous on `stream`.  bal9 [n_cam][9] is updated in place; cam_mask (device,
 *   [n_cam] c2b_camera_mask) may be NULL; status [n_cam] one byte per camera; counts [5] (device int64, indexed by status)
 *   is zeroed and then summed by integer atomics.  pts4, pt_idx and uv_obs are read only where a row holds an observation.
 * c2b_problem_resect_cameras: Level 1, synchronous.  bal9 is made the truth as c2b_problem_apply_step makes it (state mode:
 *   to_vec of the cameras first), the pass runs over the problem's row structure with its camera mask, and the state is
 *   rebuilt from bal9 (from_vec); the problem is in bal mode afterwards, as after a camera step.  status (host, [n_cam]) and
 *   counts (host, [5]) may be NULL.  The list, the row structure, the transpose, the solve buffers, the constant masks, the
 *   loss, the preconditioner and a checkpoint all stay; a checkpoint taken before the call rolls the cameras back.  A problem
 *   without observations returns C2B_RES_TOO_FEW for every camera and writes nothing.  A problem with a shard set is
 *   refused, and so is every bad argument, with the problem unchanged. */
#define C2B_RES_OK 0
#define C2B_RES_TOO_FEW 1
#define C2B_RES_DEGENERATE 2
#define C2B_RES_BEHIND 3
#define C2B_RES_CONSTANT 4
int c2b_resect_rows(double *bal9, const double *pts4, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx, const double *uv_obs,
                    int min_points, double min_gap, const c2b_camera_mask *cam_mask, uint8_t *status, int64_t *counts, void *stream);
int c2b_problem_resect_cameras(c2b_problem *p, int min_points, double min_gap, uint8_t *status, int64_t *counts);

/* ---- consensus resection: camera poses from the observations that agree (three-point hypotheses, inlier mask, refit) ----
 * c2b_resect_rows is a least-squares fit over every observation of a camera: one pixel matched to another point's
 * coordinates (a wrong match, a joined landmark) drags the sixty sums, and the camera is rejected or placed wrongly.  This
 * pass forms candidate poses from triples of observations, keeps the one most of the row agrees with, and refits on those.
 * Notation as above: camera c's row of the list in ascending order, usable(o) = the ray of c2b_resect_rows exists and the
 * point is finite, f, k1, k2 = bal9[c][6..8], E2 = max_error * max_error formed once on the host.  One wave per camera.  In
 * this order:
 *   C2B_RES_CONSTANT     the camera's mask word holds a pose bit (C2B_CONST_POSE); nothing of its row is read.
 *   C2B_RES_TOO_FEW      the whole row has fewer than min_inliers usable observations (min_inliers >= 6: it is the refit's
 *                        min_points too).
 *   sample               the usable observations among the FIRST 64 ENTRIES of the row, in row order, numbered 0 .. m - 1.
 *   hypotheses           triple number k = 0, 1, ...: the gap g runs from floor(m / 3) down to 1 and, per gap, i over 0 .. m - 1
 *                        (when 3 g == m only i < g: each triple once); the triple is {i, (i + g) mod m, (i + 2 g) mod m} in
 *                        ascending order.  The enumeration stops after max_hypotheses triples, 1 <= max_hypotheses <= 64.
 *   three-point poses    for a triple with unit rays b1..b3 and points X1..X3 the solutions are the real (l1, l2, l3), every
 *                        l > 0, with li^2 + lj^2 - 2 li lj (bi . bj) = |Xi - Xj|^2 for the three pairs.  Whatever finds the
 *                        candidates, each is polished by Newton on the three equations (at most 8 steps, until
 *                        max |step| <= 1e-14 max l) and counts when the last step was at most 1e-9 max l; a solution is NOT
 *                        FORMED when |(X2 - X1) x (X3 - X1)|^2 < 1e-12 |X2 - X1|^2 |X3 - X1|^2 or when the equations'
 *                        Jacobian J at it has |det J| <= 1e-5 (2 max l)^3; two solutions within 1e-9 max l of each other are
 *                        one.  At most FOUR solutions are kept per triple, in the order they are found (the equations have
 *                        no more than four with every l > 0, so the cap drops none); whether the determinant is tested
 *                        before or after the merge is the same, merged solutions sharing it to 1e-9.  The pose: with the orthonormal frames of the triangles (li bi) and (Xi) -- e1 along 1 -> 2,
 *                        e3 along e1 x (1 -> 3), e2 = e3 x e1 -- R = camera frame . (world frame)^T, t = l1 b1 - R X1.
 *   C2B_RES_DEGENERATE   no hypothesis has a formed solution.
 *   score                observation o of the row -- every entry, also past the 64th, also the triple itself -- is an inlier
 *                        of a pose iff it is usable and c2b_residual_keep_rows with C2B_FILTER_IN_FRONT would keep it at a
 *                        camera (R, t, f, k1, k2): du * du + dv * dv <= E2 (five unfused operations; NaN compares false)
 *                        and q.z < 0.  The score is the integer inlier count.
 *   select               the highest score, the LOWEST k among equal scores, the smallest l1 among that triple's solutions
 *                        of that score; I* is its inlier set.
 *   C2B_RES_NO_CONSENSUS |I*| < min_inliers.
 *   refit                c2b_resect_rows' rule set on I* in ascending row order with min_points = min_inliers and min_gap:
 *                        its C2B_RES_DEGENERATE or C2B_RES_BEHIND is the camera's status; C2B_RES_OK writes bal9[c][0..5]
 *                        and keeps the bits of 6..8: bit for bit what c2b_resect_rows returns on the list restricted to I*.
 * A camera whose status is not C2B_RES_OK keeps all nine entries.  Per camera also hyp = the selected k (not a solution
 * number) and n_inl = |I*|, set once a hypothesis was selected, whatever the status after it; -1 and 0 under CONSTANT,
 * TOO_FEW and when no solution was formed.  Per observation inlier[o] = 0 for the observations of a C2B_RES_OK camera
 * outside I* (the unusable ones among them), 1 everywhere else -- nothing is claimed about a camera that was not resected.
 * counts[6] is the histogram of the statuses.  No float atomics, no scratch memory, no workspace, no loss from the handle:
 * the same inputs give the same bits whatever the launch shape.  max_error negative, NaN or infinite, min_inliers < 6,
 * min_gap negative, NaN or >= 1, max_hypotheses outside [1, 64], an unknown flag bit: C2B_ERR_INVALID_ARGUMENT.
 * c2b_resect_consensus_rows: Level 0, stateless, asynchronous on `stream`.  The arguments of c2b_resect_rows, and n_obs, the
 *   length of the list; hyp, n_inl [n_cam] (device int32) and inlier [n_obs] (device, one byte) may each be NULL; counts [6]
 *   (device int64) is zeroed and inlier set to 1 before the kernel runs.
 * c2b_problem_resect_consensus: Level 1, synchronous, with the preconditions and the cache story of
 *   c2b_problem_resect_cameras: bal9 is made the truth, the pass runs over the problem's row structure with its camera
 *   mask, the state is rebuilt from bal9 and the problem is in bal mode afterwards; a shard is refused; a problem without
 *   observations returns C2B_RES_TOO_FEW for every camera and launches nothing.  status, hyp, n_inl [n_cam], inlier [n_obs,
 *   in the list's order at call time] and counts [6] are host arrays and may be NULL.  flags = C2B_RES_DROP_OUTLIERS: the
 *   list is then compacted by the inlier mask exactly as c2b_problem_triangulate_consensus compacts by its own (stable
 *   inside every camera's row, nothing renumbered, what was derived from the list is rebuilt by its next user);
 *   *n_removed (may be NULL) = how many went, and when it is 0 no cache is dropped.  Should the compaction fail (an
 *   allocation), the cameras have already moved and the list has not: the status, the mask and the counts returned
 *   describe the pass, and the call returns the error.  The constant masks, the loss, the preconditioner and a checkpoint
 *   all stay.  Every refusal leaves the problem unchanged. */
#define C2B_RES_NO_CONSENSUS 5
#define C2B_RES_DROP_OUTLIERS 1
int c2b_resect_consensus_rows(double *bal9, const double *pts4, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx,
                              const double *uv_obs, int64_t n_obs, double max_error, int min_inliers, double min_gap, int max_hypotheses,
                              const c2b_camera_mask *cam_mask, uint8_t *status, int32_t *hyp, int32_t *n_inl, uint8_t *inlier,
                              int64_t *counts, void *stream);
int c2b_problem_resect_consensus(c2b_problem *p, double max_error, int min_inliers, double min_gap, int max_hypotheses, int flags,
                                 uint8_t *status, int32_t *hyp, int32_t *n_inl, uint8_t *inlier, int64_t *counts, int64_t *n_removed);

/* ---- landmark merging: two points that are one landmark put back together (the repair of split_landmarks) ----
 * split_landmarks, like a matcher that breaks a track, leaves two points where one belongs, with the observations dealt
 * between them.  This pass finds such pairs and joins them: the two points are close, no camera sees both, and one position
 * explains every observation of both.  Notation: point p's row of the transpose (every entry counts, usable or not), R2 =
 * radius * radius and E2 = max_error * max_error each formed once on the host.  One ROUND on a state (cameras, points, the
 * camera-major list and its transpose):
 *   C2B_MERGE_HELD       p is constant under pt_held (Level 1: under the point mask, or it carries a point prior with a
 *                        non-zero weight); it takes no part: it is nobody's candidate and gets no partner.
 *   C2B_MERGE_UNOBSERVED p's row is empty; it takes no part either.
 *   candidates of p      every other point q that takes part with d2(p, q) <= R2, where d2 = (dx * dx + dy * dy) + dz * dz
 *                        (five unfused operations; dx and -dx square alike, so d2(p, q) and d2(q, p) are the same bits; a
 *                        NaN compares false), ordered by (d2, q) ascending -- d2 >= 0, its bit pattern orders it.
 *   verified pair        with a = min(p, q), b = max(p, q), na and nb the lengths of their rows:
 *                        (i)  no camera index occurs in both rows;
 *                        (ii) with f = nb / (na + nb) and per coordinate m = a + (b - a) * f (a subtraction, a product, a
 *                             sum, unfused, the lower index first: twins with equal bits give m == a exactly), EVERY entry of
 *                             both rows is one that c2b_residual_keep_rows with C2B_FILTER_IN_FRONT would keep at m: du * du +
 *                             dv * dv <= E2 && q.z < 0 (a NaN fails).
 *   C2B_MERGE_CHOSEN     partner[p] = the first verified candidate in that order;
 *   C2B_MERGE_NONE       there is none: partner[p] = -1 (also under HELD and UNOBSERVED).
 *   merge                for every pair with partner[partner[p]] == p, a < b: pts[a].xyz = m, the fourth lane keeps its value;
 *                        every pt_idx == b becomes a; pts[b] keeps its bits and is now unobserved.  Nothing is renumbered
 *                        and no count changes: uv, the row pointer and the order inside every camera's row stay bit for bit.
 * Only mutual choices merge, so the result does not depend on the launch shape or on the order the points are visited, and
 * a chain a-b-c is never merged in one round; the closest verified pair of all is always mutual, so a round that can merge
 * does.  No float atomics, no scratch memory.  The cost is that of the neighbourhoods: all points within one radius of each
 * other cost O(n_pts^2) candidate tests, and nothing bounds that.
 * c2b_merge_partner_rows: Level 0, the partner choice of one round.  camblk, pts4 and the transpose as c2b_triangulate_rows
 *   takes them (pts4 is only read), n_obs the length of the list obs_of indexes; pt_held (device, one byte per point) may be
 *   NULL; partner [n_pts] (device int32), status [n_pts] (device, one byte), counts [4] (device int64, indexed by status,
 *   zeroed and then summed by integer atomics).  The pass builds its own cell list over x / z from the extent of the points
 *   (cells of radius (1 + 2^-20), doubled until there are at most 2^24: the result does not depend on the grid), frees it
 *   and therefore SYNCHRONISES `stream` before it returns.  radius = 0 is valid (exact twins have d2 = 0); n_pts = 0 launches
 *   nothing.  radius or max_error negative, NaN or infinite, n_pts >= 2^31: C2B_ERR_INVALID_ARGUMENT.
 * c2b_problem_merge_points: Level 1, synchronous: rounds >= 1 rounds on the resident problem, each on the state the last one
 *   left with the transpose rebuilt; a round that merges nothing ends the loop (and counts in *rounds_run).  The preconditions
 *   and caches follow c2b_problem_triangulate_consensus with C2B_TRI_DROP_OUTLIERS: a shard is refused; a bad argument (also
 *   rounds < 1) is refused with the problem unchanged; a problem without observations merges nothing and launches nothing;
 *   after a round that merged, what was derived from the list is rebuilt by its next user and nothing else goes -- cameras,
 *   masks, priors, loss, preconditioner, checkpoint and LM scratch stay, as c2b_problem_filter_observations leaves them;
 *   after a round that merged nothing no cache is dropped.  merged_into [n_pts] (host, may be NULL): the point that p's
 *   observations ended on, composed over the rounds, p itself when p was not absorbed; *n_merged (may be NULL) = how many
 *   points were absorbed; *rounds_run (may be NULL).  Absorbed points STAY in the table as unobserved points (the LM step
 *   gives them a zero step); nothing is culled here, because a cull renumbers and drops the masks: c2b_problem_cull is the
 *   caller's call. */
#define C2B_MERGE_NONE 0
#define C2B_MERGE_CHOSEN 1
#define C2B_MERGE_UNOBSERVED 2
#define C2B_MERGE_HELD 3
int c2b_merge_partner_rows(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                           const uint32_t *cam_of, const double *uv_obs, int64_t n_obs, double radius, double max_error,
                           const uint8_t *pt_held, int32_t *partner, uint8_t *status, int64_t *counts, void *stream);
int c2b_problem_merge_points(c2b_problem *p, double radius, double max_error, int rounds, int32_t *merged_into, int64_t *n_merged,
                             int *rounds_run);

/* ---- guided re-matching: an observation with a wrong point index is given the index it fits (the repair of
 * add_incorrect_correspondences and join_landmarks that keeps the measurement) ----
 * Both corruptions leave the pixel right and only pt_idx wrong; the filter and C2B_TRI_DROP_OUTLIERS can only remove such an
 * observation.  This pass finds, for an observation that does not fit the point it names, the nearby point it does fit, and
 * relabels it.  Notation: E2 = max_error * max_error and R2 = radius * radius, each formed once on the host in double;
 * fit(o, q) = the predicate of c2b_residual_keep_rows with C2B_FILTER_IN_FRONT for observation o at point q through o's camera:
 * r2(o, q) = du * du + dv * dv <= E2 && q.z < 0 (unfused; libm's pow when k2 != 0; a NaN fails).  The rules:
 *   1 fits       fits[o] = fit(o, pt_idx[o]): exactly the byte c2b_residual_keep_rows(..., C2B_FILTER_IN_FRONT) writes.
 *   2 trusted    nfit[p] = the number of fitting observations of point p; trusted[p] = x, y, z finite && nfit[p] >= min_fits
 *                (min_fits >= 0; with 0 every finite point is trusted).  Nothing is judged about, or assigned to, a point that
 *                too few observations agree on.
 *   3 classes    observation o of camera c with label p = pt_idx[o]: C2B_REMATCH_FITS if fits[o]; else C2B_REMATCH_SKIPPED if
 *                !trusted[p] -- untouched and kept --; else it is FAILING.  FITS and SKIPPED observations stay, and their
 *                labels are HELD in c.
 *   4 candidates of a failing o: every q with trusted[q], q != p, q not held in c, fit(o, q), and one of
 *                  d2(p, q) = (dx * dx + dy * dy) + dz * dz <= R2 (unfused; the join case: a neighbour of the named point), or
 *                  q is the label of a failing observation of c (the swap case: failing observations give their labels up,
 *                  so a swap or a longer cycle inside one camera resolves in one call; it holds also at radius = 0).
 *   5 choice     choice[o] = the candidate with the smallest key (bits of r2(o, q), q) -- r2 >= 0, its bit pattern orders it --;
 *                choice[o] = -1 when there is none, and for every observation that is not failing.
 *   6 conflicts  among the failing observations of c with the same choice the smallest (bits of r2, o) wins and is
 *                C2B_REMATCH_REASSIGNED; the others, and those without a choice, are C2B_REMATCH_REMOVED.  A loser is not
 *                offered its second candidate.
 *   7 apply      (Level 1) pt_idx[o] = choice[o] for REASSIGNED; the list is then compacted by keep = (status != REMOVED)
 *                exactly as c2b_problem_filter_observations compacts: stable inside every row, nothing renumbered, uv of the
 *                survivors keeps its bits.  Unplaced observations are always removed: their labels may now belong to a
 *                winner, and keeping them would let a camera see a point twice.  A list in which no camera sees a point
 *                twice stays so.
 *   8 counts     counts[4] = the histogram of the statuses, by integer atomics.
 *   9            cameras are independent; nothing depends on the launch shape, on the cell grid or on the arrival order of
 *                the cell fill.
 * No float atomics, no scratch memory.  The cost is that of the neighbourhoods: one scan of the 3 x 3 cells around the named
 * point and of the row's failing labels, with a projection per candidate that survives the distance test, for every failing
 * observation, and a walk of the row for a fitting candidate; nothing bounds that, and a radius of the order of the scene
 * is the wrong input.
 * c2b_rematch_rows: Level 0, stateless, on `stream`: rules 3 - 6 and 8.  camblk and pts4 as c2b_residual_keep_rows takes them
 *   (only read), row_ptr [n_cam + 1] the camera rows of the list pt_idx / uv_obs [n_obs]; fits [n_obs] (device, one byte, rule 1:
 *   the caller's c2b_residual_keep_rows at the same max_error); pt_trusted [n_pts] (device, one byte per point, rule 2, taken as
 *   given; NULL: every finite point).  It writes choice [n_obs] (device int32), status [n_obs] (device, one byte) and counts [4]
 *   (device int64, indexed by status, zeroed and then summed).  It builds its own cell list over x / z as
 *   c2b_merge_partner_rows does, frees it and therefore SYNCHRONISES `stream` before it returns.  radius = 0 is valid (the swap
 *   case alone, and exact twins); n_obs = 0 launches nothing.  radius or max_error negative, NaN or infinite, n_pts >= 2^31,
 *   n_obs > 2^31 - 65: C2B_ERR_INVALID_ARGUMENT.
 * c2b_problem_rematch_observations: Level 1, synchronous: rules 1 - 8 on the resident problem.  radius or max_error negative,
 *   NaN or infinite, min_fits < 0 and a shard are refused with the problem unchanged; a problem without observations launches
 *   nothing and its counts are zero.  status_out [n_obs before the call] (host, may be NULL); *n_reassigned, *n_removed (may
 *   be NULL).  A call that reassigned or removed something drops what was derived from the list and nothing else -- cameras,
 *   points, masks, priors, loss, preconditioner, checkpoint and LM scratch stay, as c2b_problem_filter_observations leaves
 *   them --; a call that changes nothing drops no cache.  A failure leaves the problem as it was. */
#define C2B_REMATCH_FITS 0
#define C2B_REMATCH_SKIPPED 1
#define C2B_REMATCH_REASSIGNED 2
#define C2B_REMATCH_REMOVED 3
int c2b_rematch_rows(const double *camblk, const double *pts4, int64_t n_pts, const uint64_t *row_ptr, int64_t n_cam, const uint32_t *pt_idx,
                     const double *uv_obs, int64_t n_obs, const uint8_t *fits, const uint8_t *pt_trusted, double radius, double max_error,
                     int32_t *choice, uint8_t *status, int64_t *counts, void *stream);
int c2b_problem_rematch_observations(c2b_problem *p, double radius, double max_error, int min_fits, uint8_t *status_out,
                                     int64_t *n_reassigned, int64_t *n_removed);

/* ---- index noise on the device: noise.rs' index-corruption functions -- drop_features (src/noise.rs:229-251),
 * add_incorrect_correspondences (src/noise.rs:180-226), split_landmarks (src/noise.rs:255-291), join_landmarks
 * (src/noise.rs:323-378) -- in place on the resident problem.  The host entries of city2ba_hip_host.h (c2b_drop_features, ...)
 * draw from one sequential std::mt19937_64 and keep their seeded outputs; these are a SECOND draw scheme: every draw is a
 * Philox4x32-10 block of its own, addressed as the arithmetic noise addresses its normals: counter = (entity lo, entity hi, slot,
 * stream), key = the seed's halves, a = o1 << 32 | o0, b = o3 << 32 | o2, u(x) = (x >> 11) * 2^-53 in [0, 1).  Streams: 6 drop,
 * 7 mismatch, 8 split, 9 join.  "Observation index" = the position in the whole camera-major list when the pass starts.  A seed
 * fixes the result whatever the launch shape.  The rules (tests/_indexnoiseref.py restates them):
 *   drop      a camera with len observations keeps l = floor(len * keep_fraction), saturating (below 0: none, above len: all):
 *             those with the l smallest (a, index), a of stream 6, entity = observation index, slot 0.  The kept observations stay
 *             in their order (the reference leaves them shuffled: the kept SET is distributed as the reference's).
 *   mismatch  observation i of a row with len > 1 swaps iff u(a) <= mismatch_chance (stream 7, entity = observation index, slot 0).
 *             Its partner: weights w_k = max_d - d_ik, d_ik = sqrt(dx * dx + dy * dy) unfused, max_d the largest of the row -- so
 *             w_i = max_d, the reference's zeroed-before-shift quirk (:203-205): the likeliest partner is i itself --; j = the
 *             first k whose cumulative weight exceeds u(b) * total, else len - 1 (the cumulative sums are a wave's scan: equal to
 *             a sequential sum to rounding).  partner[i] = j, or -1.  A row with a swapping observation whose total is not
 *             positive (all positions coincide) is counted.  Then per camera the swaps of pt_idx in ascending i.
 *   select    the n smallest (key, index) of N entities, key = a of (stream, entity, slot) or a caller's 64-bit keys.
 *   split     n = min(floor(split_fraction * n_pts), n_pts) points are selected: the n smallest (a, index), stream 8, entity =
 *             point index, slot 0.  The copy of the r-th selected point in ascending index is row n_pts + r, with the same bits; an
 *             observation of a selected point moves to the copy iff bit 0 of a (stream 8, entity = observation index, slot 1).
 *   join      n = floor(join_fraction * n_pts), at most n_obs, observations are selected: the n smallest (a, index), stream 9,
 *             entity = observation index, slot 0.  The point q of each becomes entry 1 + floor(u(b) * avail) of q's nearest
 *             list, avail = min(10, n_pts - 1), b of the same draw.  Every lookup reads the table as it was.
 *   nearest   the up to 11 nearest points of a point q by ascending (d2, index), d2 = (dx * dx + dy * dy) + dz * dz unfused, q
 *             itself included (it is first unless an exact duplicate with a lower index is).
 * Level 0, stateless, on `stream`, device arrays:
 * c2b_drop_keep_rows: keep [n_obs] (one byte) for the rows row_ptr [n_cam + 1].  Asynchronous.
 * c2b_mismatch_partner_rows: partner [n_obs] (int32: the row-relative j, or -1) and *n_zero_rows (device int64, zeroed first: the
 *   rows counted).  Asynchronous.  n_obs > 2^31 - 65: C2B_ERR_INVALID_ARGUMENT.
 * c2b_select_smallest_keys_rows: select [n] (one byte).  keys [n] (device uint64) or NULL: the draws (seed; draw_stream, entity =
 *   index, slot).  n_select <= 0 selects nothing, >= n everything.  A radix select whose digits are picked on the host: SYNCHRONISES.
 * c2b_nearest_points_rows: nearest [n_query * 11] (int32, -1 past the table's size) for the point indices query [n_query] into
 *   pts4 [n_pts] (32-byte rows).  It builds an x / z cell list of about four points per cell and frees it: SYNCHRONISES.  One wave
 *   per query walks the rings of cells outward and stops once the last wanted d2 <= (r * cell * (1 - 2^-20))^2; a scene that is
 *   tall and narrow (everything in one x / z cell) is searched by brute force.
 * Level 1, synchronous, in place; a NaN fraction and a shard are refused with the problem unchanged; the counts may be NULL:
 * c2b_problem_drop_features: the list compacted as c2b_problem_filter_observations compacts it; cameras, points, masks, priors, loss,
 *   options and a checkpoint stay, what was derived from the list goes.  cull is the caller's call.
 * c2b_problem_add_incorrect_correspondences: *n_swaps = the observations that swapped (one with itself included).  A counted row
 *   fails the call with the host entry's message and leaves the list untouched.  uv, the row lengths and every per-entity state
 *   stay; what was derived from the list goes, as after c2b_problem_rematch_observations.
 * c2b_problem_split_landmarks: *n_split = n.  The point table grows, and what has one entry per point is treated as
 *   c2b_problem_cull treats it when a count changes: the constant masks, the priors, a checkpoint with the LM scratch and an origin
 *   are dropped.  n = 0 changes and drops nothing.
 * c2b_problem_join_landmarks: *n_joined = n.  n > 0 with fewer than two points: C2B_ERR_INVALID_ARGUMENT, "No neighbors?!".  Only
 *   pt_idx changes; what was derived from the list goes. */
int c2b_drop_keep_rows(const uint64_t *row_ptr, int64_t n_cam, int64_t n_obs, double keep_fraction, uint64_t seed, uint8_t *keep, void *stream);
int c2b_mismatch_partner_rows(const uint64_t *row_ptr, int64_t n_cam, const double *uv_obs, int64_t n_obs, double mismatch_chance, uint64_t seed,
                              int32_t *partner, int64_t *n_zero_rows, void *stream);
int c2b_select_smallest_keys_rows(const uint64_t *keys, int64_t n, uint64_t seed, int draw_stream, int slot, int64_t n_select, uint8_t *select,
                                  void *stream);
int c2b_nearest_points_rows(const double *pts4, int64_t n_pts, const uint32_t *query, int64_t n_query, int32_t *nearest, void *stream);
int c2b_problem_drop_features(c2b_problem *p, double keep_fraction, uint64_t seed, int64_t *n_removed);
int c2b_problem_add_incorrect_correspondences(c2b_problem *p, double mismatch_chance, uint64_t seed, int64_t *n_swaps);
int c2b_problem_split_landmarks(c2b_problem *p, double split_fraction, uint64_t seed, int64_t *n_split);
int c2b_problem_join_landmarks(c2b_problem *p, double join_fraction, uint64_t seed, int64_t *n_joined);

/* ---- sub-problems on the device: BAProblem::subset (src/baproblem.rs:394-423) for a caller's selection, a window
 * of cameras with its rim held fixed, and the write-back of what a solve of the child moved.  Integer kernels and copies only:
 * the same inputs give the same bits.  Only the selection lists cross PCIe on the way in and the origin lists on the way out.
 * `dst` is a handle from c2b_problem_create on src's device; its contents are replaced as an upload replaces them, and it is
 * left as it was on any failure.  The child is in src's camera mode and holds src's bits.  A pending visibility result of src
 * is not carried; neither are a checkpoint, LM scratch, rows, transpose or solve buffers.
 * c2b_problem_subset: cameras cam_sel and points pt_sel in the given order, repeats allowed; a repeated point appears twice and
 *   its observations name its LAST slot; observations of points that were not selected disappear; duplicated (camera, point)
 *   entries of a row are both kept; empty lists give a child without cameras and / or points.  flags = C2B_SUBSET_CARRY: the child
 *   takes src's options, loss and scale, preconditioner, inner iterations, and the constant masks and every prior kind src
 *   holds, gathered by the lists; and, when neither list repeats an index, an origin.  Without the flag the child's handle state
 *   is a new handle's.  An index out of range: C2B_ERR_INDEX_OUT_OF_RANGE; dst == src, another device, a shard, a NULL list with a
 *   non-zero count, a count >= 2^31, an unknown flag bit: C2B_ERR_INVALID_ARGUMENT.
 * c2b_problem_window: S = the cameras with seed[c] != 0 (seed: host, one byte per camera of src; an empty S is refused), P = the
 *   points with an observation in a row of S.  flags = C2B_WINDOW_HALO: H = the cameras outside S with an observation of a point
 *   of P; the child's cameras are S and H in ascending index, a seed row whole, a halo row's observations of P in row order, and
 *   a halo camera's mask word is src's OR C2B_CONST_ALL.  flags = 0: the child's cameras are S, and a point of P with an observation
 *   outside S is shared: its mask byte is src's OR 1.  The child's points are P in ascending index.  A window always carries the
 *   handle state and always records an origin.  With the rim so chosen every residual that depends on a free variable of the
 *   child is in the child.
 * c2b_problem_get_origin: cam_of [n_cam], pt_of [n_pts] (the parent's index of every camera / point of the child), cam_role
 *   [n_cam] (0 seed, 1 halo), pt_role [n_pts] (0, 1 shared); any pointer may be NULL.  A problem without an origin:
 *   C2B_ERR_INVALID_ARGUMENT.  The origin goes when the child's own entities are replaced or renumbered.
 * c2b_problem_write_back: the child's cameras and points over the parent's, component by component where the child's mask AT THE
 *   CALL leaves it free: bal9 entries whose mask bit is clear, xyz of points whose byte is clear (the fourth lane of the parent's
 *   row stays).  Worded as c2b_problem_apply_step: the parent (and a state-mode child) gets to_vec of its cameras first and is in
 *   bal mode afterwards; the parent's list, rows, transpose, solve buffers, masks, priors, loss and checkpoint stay.
 *   *n_cam_written = cameras with at least one free component, *n_pts_written = free points (may be NULL).  Refused with nothing
 *   written (C2B_ERR_INVALID_ARGUMENT): a child without an origin, a parent that is not the handle the origin names or whose
 *   entities were replaced or renumbered since (upload, read, cull, the generators), child == parent, different devices, a shard. */
#define C2B_SUBSET_CARRY 1
#define C2B_WINDOW_HALO 1
int c2b_problem_subset(c2b_problem *src, const uint32_t *cam_sel, int64_t n_cam_sel, const uint32_t *pt_sel, int64_t n_pt_sel, int flags,
                       c2b_problem *dst);
int c2b_problem_window(c2b_problem *src, const uint8_t *seed, int flags, c2b_problem *dst);
int c2b_problem_get_origin(const c2b_problem *child, uint32_t *cam_of, uint32_t *pt_of, uint8_t *cam_role, uint8_t *pt_role);
int c2b_problem_write_back(c2b_problem *child, c2b_problem *parent, int64_t *n_cam_written, int64_t *n_pts_written);

/* ---- the camera covisibility graph on the device and the search over it ----
 * Cameras are nodes.  shared(c, c'), c != c', = the number of DISTINCT points with at least one observation in row c and at
 * least one in row c': a duplicated (camera, point) entry counts once per camera pair.  The graph at a threshold min_shared >= 1
 * is a symmetric CSR: nbr_ptr [n_cam + 1] (uint64), nbr [n_edges] (uint32: the neighbours of a camera in ASCENDING index, never
 * the camera itself), shared [n_edges] (uint32), holding exactly the pairs with shared >= min_shared; n_edges counts directed
 * entries, twice the undirected number.  It is the sparsity pattern of the reduced camera system.  Integers only: the same list
 * gives the same bytes on every call, whatever the launch shape.  No float atomics, no scratch memory.
 * Level 0, stateless, asynchronous on `stream`, device arrays: row_ptr [n_cam + 1] / pt_idx [n_obs] the camera-major list,
 * pt_row_ptr / obs_of / cam_of its transpose as c2b_normal_transpose writes it (stable: a track ascends in camera index).
 * One wave per camera counts (other camera -> shared) in a table of C2B_COVIS_WAVE_SLOTS slots in LDS; a camera whose bound --
 * the sum over its row of (track length - 1) -- exceeds the table takes the heavy path (a workgroup and a dense counter row in
 * temp) with exactly the same result: no camera is truncated, whatever its degree.
 * c2b_covisibility_temp_bytes: the size of `temp` (16-byte aligned) for n_cam cameras: pass = C2B_COVIS_TEMP_GRAPH for the degree
 *   and fill passes (ONE temp, handed from the first to the second untouched), C2B_COVIS_TEMP_EXPAND for the expansion step.
 * c2b_covisibility_degree_rows: nbr_ptr [n_cam + 1] (the scanned degrees; nbr_ptr[n_cam] = n_edges) and counts [2] (device int64:
 *   n_edges, then the cameras that took the heavy path).  The caller reads counts[0] and allocates nbr and shared.
 * c2b_covisibility_fill_rows: nbr and shared [n_edges] for the nbr_ptr, temp and min_shared of the degree pass.
 *   Both: n_obs = 0 or n_cam = 0 gives an all-zero nbr_ptr and launches nothing else.  min_shared < 1, n_cam >= 2^31,
 *   n_obs > 2^31 - 65, a NULL or misaligned pointer: C2B_ERR_INVALID_ARGUMENT before any device work.
 * c2b_covisibility_expand_rows: one level of a breadth-first search.  level [n_cam] (int32, -1 = not reached); frontier
 *   [n_frontier] = cameras of level hop.  Every neighbour q of a frontier camera with level[q] < 0, shared >= min_shared (applied
 *   to the stored counts, so a graph built at a lower threshold serves) and within[q] != 0 (within: one byte per camera, or NULL)
 *   gets level hop + 1; next [n_cam] takes the cameras of level hop + 1 in ascending index and *n_next (device uint32) their
 *   number.  Refusals as above.
 * Level 1, synchronous, on the resident problem; a shard is refused:
 * c2b_problem_covisibility: builds the graph at min_shared and keeps it in the handle with its threshold; a call with the
 *   threshold it holds returns at once, another threshold rebuilds.  It is derived from the list: whatever drops the transpose
 *   (the table under c2b_problem in capi_problem.hpp) drops it; apply_step, the arithmetic noise and the refine passes keep it.
 *   *n_edges (may be NULL) = the directed entries.
 * c2b_problem_get_covisibility: the graph the handle holds to host buffers nbr_ptr [n_cam + 1], nbr, shared [n_edges]; its
 *   threshold and the number of cameras that took the heavy path; any pointer may be NULL.  No graph: C2B_ERR_INVALID_ARGUMENT.
 * c2b_problem_neighbourhood: seed (host, one byte per camera; an empty set is refused, as c2b_problem_window refuses it), within
 *   (host, one byte per camera, or NULL; a seed outside it is refused).  Level 0 is the seeds; level h + 1 is every camera not
 *   reached yet, inside `within`, with an edge of the graph at min_shared to a camera of level h; at most `hops` levels beyond
 *   the seeds (hops = 0 returns the seeds, hops < 0: until nothing new is reached -- the seeds' connected components).
 *   max_cameras <= 0: no cap.  With a cap (fewer than the seeds: refused) whole levels are taken while they fit; the first level
 *   that does not fit is ranked by (score descending, index ascending), score = the sum of shared over the candidate's edges
 *   into the levels already taken, saturating at 2^32 - 1, its best fill the remainder (c2b_select_smallest_keys_rows' radix
 *   select), and the search ends.  member [n_cam] (host bytes), level [n_cam] (host int32, -1 = not reached), *n = the members;
 *   each may be NULL.  Nothing is written on a refusal. */
#define C2B_COVIS_WAVE_SLOTS 2048
#define C2B_COVIS_TEMP_GRAPH 0
#define C2B_COVIS_TEMP_EXPAND 1
int64_t c2b_covisibility_temp_bytes(int64_t n_cam, int pass);
int c2b_covisibility_degree_rows(const uint64_t *row_ptr, const uint32_t *pt_idx, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                                 const uint32_t *cam_of, int64_t n_cam, int64_t n_pts, int64_t n_obs, int min_shared, void *temp,
                                 uint64_t *nbr_ptr, int64_t *counts, void *stream);
int c2b_covisibility_fill_rows(const uint64_t *row_ptr, const uint32_t *pt_idx, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                               const uint32_t *cam_of, int64_t n_cam, int64_t n_pts, int64_t n_obs, int min_shared, void *temp,
                               const uint64_t *nbr_ptr, uint32_t *nbr, uint32_t *shared, void *stream);
int c2b_covisibility_expand_rows(const uint64_t *nbr_ptr, const uint32_t *nbr, const uint32_t *shared, int64_t n_cam, int min_shared,
                                 const uint8_t *within, const uint32_t *frontier, int64_t n_frontier, int hop, int32_t *level, uint32_t *next,
                                 uint32_t *n_next, void *temp, void *stream);
int c2b_problem_covisibility(c2b_problem *p, int min_shared, int64_t *n_edges);
int c2b_problem_get_covisibility(c2b_problem *p, uint64_t *nbr_ptr, uint32_t *nbr, uint32_t *shared, int *min_shared, int64_t *n_heavy);
int c2b_problem_neighbourhood(c2b_problem *p, const uint8_t *seed, int hops, int min_shared, int64_t max_cameras, const uint8_t *within,
                              uint8_t *member, int32_t *level, int64_t *n);

/* ---- the explicit Schur complement on the covisibility pattern ----
 * c2b_problem_solve_step solves S dc = b, S = U_l - W V_l^-1 W^T, without forming S.  With C2B_SCHUR_EXPLICIT it forms S once per
 * call in block-CSR and runs the same PCG on the stored blocks; the step it converges to is the same.  Notation as above: U, V, gc, gp
 * are the stacked system's (priors in, constant rows and columns zeroed), W_o = w_o Jc_o^T Jp_o with w_o the loss's weight, U_l and
 * V_l are damped by the clamp rule.
 * Pattern: the covisibility graph above at min_shared = 1, plus the diagonal: nbr_ptr [n_cam + 1] (uint64), nbr [n_edges] (uint32,
 *   ascending, no self edge).  The handle keeps its OWN copy (built by the Level-0 covisibility passes, or copied from the cached graph
 *   when that is at threshold 1), so c2b_problem_covisibility at another threshold does not disturb it; it is derived from the list
 *   and dropped with the rows, the transpose and the solve buffers.
 * Off-diagonal block of edge e = (c, c'), 81 doubles row-major at S_off[e]:
 *   S_e = - sum_{p seen by both} (sum_{o in (c,p)} W_o) V_l,p^-1 (sum_{o' in (c',p)} W_o')^T     (duplicated pairs: the inner sums).
 * Diagonal block at S_diag[c]:  S_cc = U_l,c - sum_p (sum_{o in (c,p)} W_o) V_l,p^-1 (sum_{o in (c,p)} W_o)^T -- S's own diagonal,
 *   the cross terms of a duplicated pair included (so not the Schur-Jacobi M_c when a pair repeats; M_c itself does not change).
 * Storage is full: (c, c') and (c', c) are both stored and S_off[(c', c)] == S_off[(c, c')]^T bit for bit.
 * Constants: the constant rows and columns of every block are 0, a constant diagonal entry is lambda 1e-6, a constant point
 *   contributes nothing; every constant entry of dc and every dp row of a constant point compares == 0.0 as before.
 * Deterministic: no float atomics; a block's terms are added in ascending observation of the lower camera's row, then ascending
 *   position in the point's track; the product adds a row's blocks in ascending edge order in a fixed tree.
 * _set_schur / _get_schur: the handle's state like the preconditioner (default C2B_SCHUR_IMPLICIT): it survives uploads, reads
 *   and culls and is carried by subset / window under C2B_SUBSET_CARRY.  Another kind: C2B_ERR_INVALID_ARGUMENT.  With
 *   C2B_SCHUR_IMPLICIT c2b_problem_solve_step launches exactly what it launched before this entry existed, bit for bit.  With
 *   C2B_SCHUR_EXPLICIT the set-up builds the pattern if absent, Y_o = L_p^-1 Jp_o^T Jc_o per observation (V_l,p = L L^T; 216 bytes
 *   each, in the solve buffers), the blocks, and q = S p of every iteration is one product with them; b and the back-substitution
 *   stay the implicit passes; both preconditioners work unchanged.  If the buffers cannot be allocated the call returns
 *   C2B_ERR_OOM with the bytes in the message and the handle stays usable (set C2B_SCHUR_IMPLICIT): there is no silent fallback.
 * _schur_bytes: the bytes the explicit solve adds to the solve buffers, 648 (n_edges + n_cam) + 216 n_obs; builds the pattern.
 * _schur_complement: S and b = -gc + W V_l^-1 gp at lambda into the caller's DEVICE arrays S_diag [n_cam][81], S_off [n_edges][81],
 *   b [n_cam][9] (8-byte aligned; S_off may be NULL when there is no edge), *n_edges = the directed entries; under either setting,
 *   which it leaves as it is.  It needs the explicit solve's buffers (c2b_problem_schur_bytes) for the duration of the call: under
 *   C2B_SCHUR_EXPLICIT they are the handle's and stay, under C2B_SCHUR_IMPLICIT they are freed before it returns.  NULL p / S_diag / b / n_edges, a misaligned pointer or a lambda outside the step's range:
 *   C2B_ERR_INVALID_ARGUMENT before any device work.  A shard is refused.  Without observations S = lambda 1e-6 I and b = 0.
 * _get_schur_pattern: the pattern to HOST arrays nbr_ptr [n_cam + 1], nbr [n_edges] (either may be NULL); builds it if absent.
 * Level 0, stateless, asynchronous on `stream`, device arrays, 8-byte aligned doubles and row pointers, 4-byte indices; a NULL or
 * misaligned pointer or a count out of range: C2B_ERR_INVALID_ARGUMENT before any device work:
 * _schur_y_rows(_loss): Y [n_obs][3][9] from the inputs of c2b_schur_points_rows, cam_idx [n_obs] (c2b_expand_rows) and V.
 * _schur_blocks_rows: S_off [n_edges][81] written, and the cross terms of duplicated pairs ADDED to S_diag [n_cam][81] (which holds
 *   M of c2b_schur_jacobi_rows on entry), from Y, the list, its transpose and the pattern -- which must be the covisibility graph
 *   of that list at min_shared 1: a pair it does not hold is skipped.  Rows of more than C2B_SCHUR_LDS_BLOCKS neighbours take the
 *   heavy path with the same result.
 * _schur_spmv_rows: y [n_cam][9] = S x; part (may be NULL) takes x.y as 4 ceil(n_cam / 4) partials, one per wave. */
#define C2B_SCHUR_IMPLICIT 0
#define C2B_SCHUR_EXPLICIT 1
#define C2B_SCHUR_LDS_BLOCKS 32
int c2b_problem_set_schur(c2b_problem *p, int kind);
int c2b_problem_get_schur(const c2b_problem *p, int *kind);
int c2b_problem_schur_bytes(c2b_problem *p, int64_t *bytes);
int c2b_problem_schur_complement(c2b_problem *p, double lambda, double *S_diag, double *S_off, double *b, int64_t *n_edges);
int c2b_problem_get_schur_pattern(c2b_problem *p, uint64_t *nbr_ptr, uint32_t *nbr);
int c2b_schur_y_rows(const double *camblk, const double *pts4, const uint32_t *cam_idx, const uint32_t *pt_idx, const double *uv_obs,
                     int64_t n_obs, const double *V, double lambda, double *Y, void *stream);
int c2b_schur_y_rows_loss(const double *camblk, const double *pts4, const uint32_t *cam_idx, const uint32_t *pt_idx, const double *uv_obs,
                          int64_t n_obs, const double *V, double lambda, double *Y, int kind, double scale, void *stream);
int c2b_schur_blocks_rows(const uint64_t *row_ptr, const uint32_t *pt_idx, const uint64_t *pt_row_ptr, const uint32_t *obs_of,
                          const uint32_t *cam_of, int64_t n_cam, int64_t n_obs, const uint64_t *nbr_ptr, const uint32_t *nbr,
                          const double *Y, double *S_diag, double *S_off, void *stream);
int c2b_schur_spmv_rows(const uint64_t *nbr_ptr, const uint32_t *nbr, int64_t n_cam, const double *S_diag, const double *S_off,
                        const double *x, double *y, double *part, void *stream);

/* ---- the direct solve of the reduced camera system: dense Cholesky on the device ----
 * A second linear solver for c2b_problem_solve_step, chosen per handle: C2B_LINEAR_PCG (the default) or C2B_LINEAR_CHOLESKY, under
 * which the step forms S as the explicit path does, scatters it into a dense lower triangle, factors it by a blocked Cholesky,
 * solves by two triangular substitutions and back-substitutes dp as before.  There is no PCG and no preconditioner.
 * Setting.  _set_linear_solver / _get_linear_solver: the handle's state like the preconditioner: it survives uploads, reads and
 *   culls and is carried by subset / window under C2B_SUBSET_CARRY.  It is NOT a value of c2b_problem_set_schur, which keeps its two.
 *   Another kind: C2B_ERR_INVALID_ARGUMENT.  Under C2B_LINEAR_PCG every entry launches exactly what it launched before this entry
 *   existed, bit for bit, whatever `schur` is.
 * Set-up under C2B_LINEAR_CHOLESKY: the explicit set-up whatever `schur` says (`schur` is left alone, as c2b_problem_schur_complement
 *   leaves it): the pattern if absent, S into S_diag / S_off without the preconditioner's factors, b by the implicit pass as before.
 *   The preconditioner setting is ignored and c2b_problem_preconditioner_fallbacks is 0.
 * Dense image.  N = 9 n_cam, Np = 64 ceil(N / 64).  A is row-major with leading dimension Np.  Only the lower triangle, diagonal
 *   included, is meaningful: the upper triangle is never read and is unspecified afterwards.  The padding rows i >= N hold 1 on the
 *   diagonal and 0 elsewhere.  A and two Np vectors are carved from the solve buffers after Y, present only under
 *   C2B_LINEAR_CHOLESKY.  _linear_solver_bytes: what the direct solve adds to the solve buffers,
 *   8 (schur_explicit_doubles + Np^2 + 2 Np) with schur_explicit_doubles = c2b_problem_schur_bytes / 8; builds the pattern.
 *   C2B_DENSE_MAX_CAMERAS (Np = 36 864, 10.9 GB) is a condition, not a tuning result: above it c2b_problem_solve_step and
 *   _linear_solver_bytes return C2B_ERR_INVALID_ARGUMENT naming the cap.  A failed allocation returns C2B_ERR_OOM with the bytes in
 *   the message and the handle stays usable under C2B_LINEAR_PCG: there is no silent fallback.  A shard is refused as before.
 * Constants and empty cameras need nothing special: a constant entry's row and column of S are exactly 0 with lambda 1e-6 on the
 *   diagonal, an empty camera's block is lambda 1e-6 I, b is exactly 0 there, and the substitutions return exactly +0.0 in those
 *   entries of dc.
 * Result.  info.iterations is 0.  info.status is 0 when every pivot was finite and > 0; otherwise 2 with dc = dp = 0, rel_residual 1
 *   and model_decrease 0 (the rule for a step without a factor: the LM loops raise lambda).  info.rel_residual is the true
 *   |b - S dc| / |b| from one product with the stored blocks (0 when b = 0).  max_iters and rel_tol are validated as before and
 *   otherwise unused.  sum_sq and model_decrease are the unchanged model pass's.  Deterministic: every entry has one owner and a
 *   fixed summation order, no float atomics: the same problem and arguments give the same bits.
 * Level 0, stateless, asynchronous on `stream`, device pointers, doubles and nbr_ptr 8-byte aligned, nbr and info 4; a NULL or
 * misaligned pointer, an ld that is no multiple of 64 or exceeds 9 C2B_DENSE_MAX_CAMERAS, n > ld: C2B_ERR_INVALID_ARGUMENT before any
 * device work:
 * _dense_scatter_rows: the lower triangle of S (the blocks of a camera's neighbours c' < c of the ascending pattern, and S_cc) into
 *   A [64 ceil(9 n_cam / 64)][ld], zeros elsewhere in it, and the padding rows.
 * _dense_cholesky: A [64 ceil(n / 64)][ld] = L L^T in place, lower triangle; n need not be a multiple of 64, ld must be; the rows
 *   from n to the next multiple of 64 must be padding rows as above and stay so.  info (device int32) is set to 0, then to the
 *   1-based index of the FIRST pivot that is not finite or not > 0; the factorisation goes on with a pivot of 1 there (a numerical
 *   status, never a fault: no address depends on matrix data) and what it leaves is then meaningless.
 * _dense_cholesky_solve: x [64 ceil(n / 64)] holds b on entry (its padding entries finite, e.g. 0) and L^-T L^-1 b on return. */
#define C2B_LINEAR_PCG 0
#define C2B_LINEAR_CHOLESKY 1
#define C2B_DENSE_MAX_CAMERAS 4096
int c2b_problem_set_linear_solver(c2b_problem *p, int kind);
int c2b_problem_get_linear_solver(const c2b_problem *p, int *kind);
int c2b_problem_linear_solver_bytes(c2b_problem *p, int64_t *bytes);
int c2b_dense_scatter_rows(const uint64_t *nbr_ptr, const uint32_t *nbr, int64_t n_cam, const double *S_diag, const double *S_off,
                           double *A, int64_t ld, void *stream);
int c2b_dense_cholesky(double *A, int64_t n, int64_t ld, int32_t *info, void *stream);
int c2b_dense_cholesky_solve(const double *A, int64_t n, int64_t ld, double *x, void *stream);

/* ---- a problem compared against ground truth: similarity alignment on the device ----
 * Build-defined (the reference has nothing like it).  Two problems on one device, the estimate p and the reference ref, with equal
 * n_cam and n_pts; index i of one corresponds to index i of the other.
 * 1. Correspondences.  `on` is C2B_ALIGN_CAMERAS, C2B_ALIGN_POINTS or both OR-ed.  A camera contributes its centre, a point its
 *    position: x_i from p, y_i from ref.  Optional byte masks use_cam [n_cam], use_pt [n_pts] switch correspondences off (NULL: all
 *    on).  With both kinds the two sets are pooled and every correspondence has weight 1.
 * 2. Fit.  (s, R, t) minimising sum |s R x_i + t - y_i|^2 in Umeyama's closed form: means mu_x, mu_y; var_x = sum |x - mu_x|^2 / n,
 *    var_y, cov = sum (y - mu_y)(x - mu_x)^T / n; cov = U D V^T; R = U diag(1, 1, det(U V^T)) V^T; s = tr(D diag(1, 1, det(U V^T))) / var_x,
 *    or 1 when `scale` is off; t = mu_y - s R mu_x.  The moments are centred: a first pass sums the coordinates, a second sums the
 *    moments about the rounded mean together with the residual sums, and the host moves them onto the mean itself.  Raw sums
 *    xx^T - n mu mu^T are never formed.
 * 3. Status.  C2B_ALIGN_OK; C2B_ALIGN_TOO_FEW: fewer than 3 correspondences; C2B_ALIGN_DEGENERATE: var_x = 0, or the second singular
 *    value of cov is at most 1e-12 times the first (collinear: the rotation is not determined).  On either failure of the FIRST fit the
 *    transform returned is the identity and nothing else is written.  A planar cloud (rank 2) is not degenerate: the det correction
 *    picks the proper rotation.
 * 4. Errors after alignment.  Per camera e_c = |s R c + t - c_ref| and, with the aligned rotation R_c' = R_c R^T,
 *    theta_c = 2 asin(min(1, |R_c' - R_c_ref|_F / (2 sqrt 2))) in radians (the chord keeps a small angle, which acos((tr - 1) / 2) does
 *    not); per point e_p = |s R X + t - X_ref|.  Summaries per kind over the correspondences that are on: count, sum e^2, sum e, max and
 *    the lowest index attaining it (-1 with nothing on); the rotation errors likewise, over the cameras that are on.  A masked-off
 *    entity still gets its per-entity error; it is left out of the fit and the summaries only.  A kind that is not in `on` is
 *    summarised over the caller's mask of that kind.
 * 5. Trimming (max_dist > 0 and rounds >= 1; otherwise one fit).  After a fit a correspondence stays on only if it is on in the
 *    caller's mask and its aligned distance, in the reference's frame, is <= max_dist; the fit is repeated on that set, until the set
 *    repeats or after `rounds` re-fits.  A set below 3 (or a degenerate one) ends the loop with that status and the last good
 *    transform; the inlier masks and the summaries are then those of the set that failed.  Otherwise the inlier masks are the set the
 *    returned transform was fitted on, and the summaries run over it: a call with rounds = 0 and those masks as use_* returns the same
 *    bits.  This is trimming from the least-squares start, NOT a consensus search: gross outliers pull the first fit away and can empty
 *    the set, which is reported (TOO_FEW), not hidden.
 * 6. c2b_problem_transform: every point X <- s R X + t; every camera gets the rotation R_c R^T and the centre s R c + t
 *    (t_c <- -R_c' (s R c + t)); f, k1, k2 stay.  Projections are invariant (R_c' (X' - c') = s R_c (X - c), and the projection
 *    divides by depth).  Caches as after the arithmetic noise: the camera table, the centre table and bal9 are dropped (the problem
 *    is in state mode afterwards); rows, transpose, solve buffers, the covisibility graph, masks, loss, preconditioner and a
 *    checkpoint stay.  Priors hold positions in the OLD frame and are left as they are: re-set them after a transform.
 *    Refused: a non-finite entry, s <= 0, |R^T R - I|_F > 1e-9, det R < 0.
 * 7. Deterministic: no float atomics; workgroup partials are folded in a fixed order; two calls give the same bits.
 * c2b_similarity.rotation is row-major.  Host arithmetic (no device): c2b_similarity_from_moments (rule 2 and 3; var_y is not used by
 *   the closed form and only has to be >= 0), c2b_align_finish_moments (means [7] and moments [23] as the two passes leave them ->
 *   n, the means, var_x, var_y, cov), c2b_align_launch_shape (threads per workgroup, most workgroups, entities per thread and trip).
 * Level 0, stateless, asynchronous on `stream`, device pointers; tables are 32-byte rows [n][4] (16-byte aligned), cam15 tables
 *   [n][15]; a kind with a zero count may pass NULL tables; workspace as for c2b_stats (one launch at a time).  A NULL or misaligned
 *   pointer or a negative count: C2B_ERR_INVALID_ARGUMENT before any device work.
 *   _means_rows: means [7] = count, sum x, sum y.  _moments_rows: moments [23] = sum |x - m_x|^2, sum |y - m_y|^2, the nine of
 *   sum (y - m_y)(x - m_x)^T row-major, sum (x - m_x), sum (y - m_y), and the pivot m_x, m_y = sums / count it read from `means`.
 *   _errors_rows: err [n] (may be NULL); base / use (may be NULL: all on): the caller's mask and the set summarised; next (may be
 *   NULL): base && e <= max_dist (max_dist <= 0: base), it must not be `use`; summary [7] = count, sum e^2, sum e, max, argmax, bytes of
 *   next that differ from use, size of next.  _rotation_errors_rows: the same over two cam15 tables, the error being theta.
 *   c2b_similarity_apply: cam15 and pts4 in place (either may be NULL with a zero count).
 * Level 1, synchronous; neither problem is modified by c2b_problem_align (derived caches may be built).  use_cam / use_pt / the
 *   outputs are host arrays, every output may be NULL: cam_err, cam_rot_err [n_cam], pt_err [n_pts], cam_inlier [n_cam], pt_inlier
 *   [n_pts].  Both entries refuse a shard, different devices, different sizes, nothing uploaded: C2B_ERR_INVALID_ARGUMENT, nothing written. */
#define C2B_ALIGN_CAMERAS 1
#define C2B_ALIGN_POINTS 2
#define C2B_ALIGN_BOTH 3
#define C2B_ALIGN_OK 0
#define C2B_ALIGN_TOO_FEW 1
#define C2B_ALIGN_DEGENERATE 2
typedef struct {
    double scale, rotation[9], translation[3];
} c2b_similarity;
typedef struct {
    int32_t on, scale, rounds, reserved;      /* C2B_ALIGN_*; 0 / 1; re-fits at most (0: one fit); 0 */
    double max_dist;                          /* <= 0: no trimming */
    const uint8_t *use_cam, *use_pt;          /* host, may be NULL */
} c2b_align_options;
typedef struct {
    int64_t n, argmax;
    double sum_sq, sum, max;
} c2b_align_stat;
typedef struct {
    int32_t status, rounds;                   /* C2B_ALIGN_*; re-fits done */
    c2b_align_stat cameras, camera_rotations, points;
} c2b_align_summary;
void c2b_align_options_init(c2b_align_options *opt);
int c2b_similarity_from_moments(int64_t n, const double mean_x[3], const double mean_y[3], double var_x, double var_y, const double cov9[9],
                                int scale, c2b_similarity *sim, int *status);
int c2b_align_finish_moments(const double means7[7], const double moments23[23], double *n, double mean_x[3], double mean_y[3],
                             double *var_x, double *var_y, double cov9[9]);
int c2b_align_launch_shape(int *threads_per_workgroup, int *max_workgroups, int *entities_per_trip);
int c2b_align_means_rows(const double *x_cam4, const double *y_cam4, const uint8_t *use_cam, int64_t n_cam, const double *x_pts4,
                         const double *y_pts4, const uint8_t *use_pt, int64_t n_pts, void *workspace, double *means7, void *stream);
int c2b_align_moments_rows(const double *x_cam4, const double *y_cam4, const uint8_t *use_cam, int64_t n_cam, const double *x_pts4,
                           const double *y_pts4, const uint8_t *use_pt, int64_t n_pts, const double *means7, void *workspace,
                           double *moments23, void *stream);
int c2b_align_errors_rows(const double *x4, const double *y4, int64_t n, const c2b_similarity *sim, const uint8_t *base, const uint8_t *use,
                          double max_dist, double *err, uint8_t *next, void *workspace, double *summary7, void *stream);
int c2b_align_rotation_errors_rows(const double *x_cam15, const double *y_cam15, int64_t n, const c2b_similarity *sim, const uint8_t *use,
                                   double *err, void *workspace, double *summary7, void *stream);
int c2b_similarity_apply(double *cam15, int64_t n_cam, double *pts4, int64_t n_pts, const c2b_similarity *sim, void *stream);
int c2b_problem_align(c2b_problem *p, c2b_problem *ref, const c2b_align_options *opt, c2b_similarity *sim, c2b_align_summary *summary,
                      double *cam_err, double *cam_rot_err, double *pt_err, uint8_t *cam_inlier, uint8_t *pt_inlier);
int c2b_problem_transform(c2b_problem *p, const c2b_similarity *sim);

/* ---- f32 extension (BASELINE.json configs[4]).  The reference has NO f32 compute path:
 * these run the same kernels over a float state -- cam15 / pts4 stored as float -- with the draws and
 * the statistics kept in f64; results track the f64 path to f32 accuracy (tested at an f32 tolerance). */
int c2b_convert_f64_to_f32(const double *src, int64_t n, float *dst, void *stream);
int c2b_convert_f32_to_f64(const float *src, int64_t n, double *dst, void *stream);
int c2b_stats_f32(const float *cam15, int64_t n_cam, const float *pts4, int64_t n_pts, void *workspace,
                  double *stats, void *stream);
int c2b_add_drift_f32(float *cam15, int64_t n_cam, float *pts4, int64_t n_pts, const double *origin,
                      double strength, double angle_strength, double std, double dir_x, double dir_y,
                      double dir_z, uint64_t seed, void *stream);
int c2b_add_drift_normalized_f32(float *cam15, int64_t n_cam, float *pts4, int64_t n_pts,
                                 const double *stats, double strength, double angle_strength,
                                 double std, uint64_t seed, void *stream);
int c2b_add_noise_entities_f32(float *cam15, int64_t n_cam, float *pts4, int64_t n_pts,
                               const double *stats, double translation_std, double rotation_std,
                               double point_std, uint64_t seed, void *stream);
int c2b_add_sin_noise_f32(float *cam15, int64_t n_cam, float *pts4, int64_t n_pts, const double *stats,
                          double dir_x, double dir_y, double dir_z, double ndir_x, double ndir_y,
                          double ndir_z, double strength, double frequency, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CITY2BA_HIP_EXPERIMENTAL_H */
