// schur_kernels.hpp -- gfx950 kernels of the damped Gauss-Newton step (included by capi.hip only, after normal_kernels.hpp).
//
// The step solves (J^T J + lambda D) delta = -g through the Schur complement on the cameras, S = U_l - W V_l^-1 W^T,
// by block-Jacobi preconditioned conjugate gradients, never forming W (= sum Jc^T Jp) or S: every product with them is
// a pass over the observations that recomputes J through jacobian_obs, as the normal_kernels.hpp passes do.
//   * k_schur_points: point-major through the transpose, one lane per point walking its observations in ascending
//     index: t_p = V_l,p^-1 (h_p + sum Jp^T (Jc x_c)), the 3x3 solve in registers.
//   * k_schur_cameras: camera-major, kNormG lanes per camera (the k_normal_cameras layout and xor tree), one wave per
//     four cameras: y_c = U_l,c x_c - sum Jc^T (Jp t_p), optionally with the wave's x.y as one partial.
//   * k_schur_factor / k_pcg_update / k_pcg_direction: the 9x9 Cholesky preconditioner, the PCG vector updates with
//     r.r and r.z as one partial per workgroup, p = z + beta p.
//   * k_schur_jacobi / k_schur_factor_blocks: the Schur-Jacobi preconditioner, S's own 9x9 diagonal blocks in place of
//     U_l's, factored into k_schur_factor's format (an option of the solve).
//   * k_schur_model: ||r||^2 and ||r||^2 - ||r + Jc dc + Jp dp||^2 per observation, one partial per workgroup.
//   * k_const_cameras / k_const_points / k_const_blocks / k_const_point_blocks: constant parameters, the
//     projection onto the free ones applied around the passes above; k_add_free / k_points_add_free: the step added to
//     the free entries alone.  None is launched while no mask is set.
//   * k_lm_norms / k_lm_gradient_max / k_lm_max_fold: the step's and the state's squared norms and the gradient's largest
//     magnitude, what the stopping tests of c2b_problem_levenberg_marquardt read.
// Damping (Marquardt with Ceres' clamps): A_l = A + lambda diag(d), d_i = min(max(A_ii, 1e-6), 1e32).
// Every partial is summed by k_normal_sum in a fixed order; no float atomics, so the same inputs give the same bits.
// Robust losses: the passes over the observations scale (r, Jc, Jp) by sqrt(w) right after jacobian_obs.  Each is one
// template with a trailing pack `class... Loss`: empty is the squared-loss kernel as it always was, <..., int, double>
// takes (kind, a2) last and makes that one call (loss_scale_obs, normal_kernels.hpp, says why a pack and not a shared
// device body or a flag).
#pragma once
#include "normal_kernels.hpp"

namespace c2b {

constexpr int kSchurBlock = 256;
constexpr int kCholPacked = 45;                   // lower triangle of a 9x9, row by row
enum { kSchurApply = 0, kSchurDot = 1, kSchurRhs = 2, kSchurNoX = 3 };
// device scalars of a solve (c2b_problem::sv_sc): p.q, r.r, r.z ping-pong, sum |r|^2, model decrease
enum { kScPq = 0, kScRr = 1, kScRz0 = 2, kScRz1 = 3, kScSumSq = 4, kScModel = 5, kScSlots = 8 };

C2B_DEV double damped(double a, double lam) { return a + lam * fmin(fmax(a, 1e-6), 1e32); }

// index of (i, j), j <= i, in the packed lower triangle
C2B_DEV constexpr int tri9(int i, int j) { return i * (i + 1) / 2 + j; }

// the workgroup's sum of one value per thread, in a fixed order, written by thread 0
C2B_DEV void block_sum_to(double v, double *sRed, double *__restrict__ out) {
    const double w = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// ---- point pass ----------------------------------------------------------------------------------------------
// t_p = (NEG ? -1 : 1) V_l,p^-1 (h_p + sum_o Jp_o^T (Jc_o x_c(o))); h == NULL is 0, x == NULL is 0 (no observation read)
template <bool NEG, class... Loss>
__global__ __launch_bounds__(kSchurBlock) void k_schur_points(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
    const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs,
    const double *__restrict__ V, double lam, const double *__restrict__ x, const double *__restrict__ h, double *__restrict__ t,
    Loss... loss) {
    const int64_t p = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (p >= n_pts) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (h) { a0 = h[3 * p]; a1 = h[3 * p + 1]; a2 = h[3 * p + 2]; }
    if (x) {
        const uint64_t b = pt_row_ptr[p], e = pt_row_ptr[p + 1];
        if (e > b) {
            const double4 X = pts4[p];
            for (uint64_t j = b; j < e; ++j) {
                const uint32_t o = obs_of[j], c = cam_of[j];
                double r0, r1, jc[18], jp[6];
                jacobian_obs(cam_ref(camblk, c), X, uv_obs[o], r0, r1, jc, jp);
                if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
                const double *xc = x + (int64_t)c * 9;
                double z0 = 0.0, z1 = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const double xk = xc[k];
                    z0 += jc[k] * xk;
                    z1 += jc[9 + k] * xk;
                }
                a0 += jp[0] * z0 + jp[3] * z1;
                a1 += jp[1] * z0 + jp[4] * z1;
                a2 += jp[2] * z0 + jp[5] * z1;
            }
        }
    }
    // V_l = L L^T, L in registers
    const double *Vp = V + p * 9;
    const Chol3 L = chol3_factor(damped(Vp[0], lam), Vp[3], Vp[6], damped(Vp[4], lam), Vp[7], damped(Vp[8], lam));
    double t0, t1, t2;
    L.solve(a0, a1, a2, t0, t1, t2);
    t[3 * p] = NEG ? -t0 : t0;
    t[3 * p + 1] = NEG ? -t1 : t1;
    t[3 * p + 2] = NEG ? -t2 : t2;
}

// ---- camera pass ---------------------------------------------------------------------------------------------
// s_c = sum_o Jc_o^T (Jp_o t_p(o)) over the camera's list, then
//   kSchurApply: y_c = U_l,c x_c - s_c;  kSchurNoX: y_c = -s_c (x unused);  kSchurDot: as kSchurApply, and sum_c x_c . y_c
//   leaves as one partial per wave in block_part;  kSchurRhs: y_c = s_c - h_c (the reduced right-hand side when
//   t = V_l^-1 gp, h = gc).  One instance per mode: a pointer its mode does not read costs it no scalar registers.
template <int MODE, class... Loss>
__global__ __launch_bounds__(kNormBlock) void k_schur_cameras(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint64_t *__restrict__ row_ptr, int n_cam,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, const double *__restrict__ U, double lam,
    const double *__restrict__ x, const double *__restrict__ h, const double *__restrict__ t, double *__restrict__ y,
    double *__restrict__ block_part, Loss... loss) {
    constexpr int kWaves = kNormBlock / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / kNormG, gl = lane % kNormG;
    const int q = (int)blockIdx.x * kWaves + wave;                   // one wave per kNormCamsPerWave cameras, no grid-stride loop
    const int c = q * kNormCamsPerWave + grp;
    const bool cam_ok = c < n_cam;
    const uint64_t b = cam_ok ? row_ptr[c] : 0, e = cam_ok ? row_ptr[c + 1] : 0;
    const CamRef cam = cam_ref(camblk, cam_ok ? (uint32_t)c : 0u);
    double s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = 0.0;
#pragma unroll 1
    for (uint64_t o = b + gl; o < e; o += kNormG) {
        const uint32_t pi = pt_idx[o];
        double r0, r1, jc[18], jp[6];
        jacobian_obs(cam, pts4[pi], uv_obs[o], r0, r1, jc, jp);
        if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
        const double *tp = t + (int64_t)pi * 3;
        const double t0 = tp[0], t1 = tp[1], t2 = tp[2];
        const double z0 = (jp[0] * t0 + jp[1] * t1) + jp[2] * t2;
        const double z1 = (jp[3] * t0 + jp[4] * t1) + jp[5] * t2;
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += jc[k] * z0 + jc[9 + k] * z1;
    }
    // fixed xor tree over the group's 16 lanes (every lane ends with the same bits)
#pragma unroll
    for (int off = kNormG / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += __shfl_xor(s[k], off, 64);
    }
    double sg = 0.0;                                                 // s[gl] without a dynamically indexed register array
#pragma unroll
    for (int k = 0; k < 9; ++k) sg = gl == k ? s[k] : sg;
    double yg = 0.0, xg = 0.0;
    if (cam_ok && gl < 9) {
        if (MODE == kSchurRhs) {
            yg = sg - h[(int64_t)c * 9 + gl];
        } else {
            double ux = 0.0;
            if (MODE != kSchurNoX) {
                const double *Ur = U + (int64_t)c * 81 + gl * 9, *xc = x + (int64_t)c * 9;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const double u = Ur[k];
                    ux += (k == gl ? damped(u, lam) : u) * xc[k];
                }
                xg = xc[gl];
            }
            yg = ux - sg;
        }
        y[(int64_t)c * 9 + gl] = yg;
    }
    if (MODE == kSchurDot) {                                         // the wave's x.y: its four cameras, in a fixed tree
        const double w = wave_sum(xg * yg);                          // 0 on lanes gl >= 9 and past n_cam
        if (lane == 0) block_part[q] = w;
    }
}

// ---- preconditioner and PCG vectors ----------------------------------------------------------------------------------
// Lf[c] = the Cholesky factor of U_l,c, packed lower rows with the reciprocal of each diagonal entry in its place
__global__ __launch_bounds__(kSchurBlock) void k_schur_factor(int64_t n_cam, const double *__restrict__ U, double lam,
                                                              double *__restrict__ Lf) {
    const int64_t c = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (c >= n_cam) return;
    const double *Uc = U + c * 81;
    double a[kCholPacked];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) a[tri9(i, j)] = i == j ? damped(Uc[i * 9 + j], lam) : Uc[i * 9 + j];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        double d = a[tri9(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= a[tri9(j, k)] * a[tri9(j, k)];
        const double inv = 1.0 / sqrt(d);
        a[tri9(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < 9; ++i) {
            double v = a[tri9(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= a[tri9(i, k)] * a[tri9(j, k)];
            a[tri9(i, j)] = v * inv;
        }
    }
    double *Lc = Lf + c * kCholPacked;
#pragma unroll
    for (int k = 0; k < kCholPacked; ++k) Lc[k] = a[k];
}

// z = (L L^T)^-1 r with a factor of k_schur_factor
C2B_DEV void chol9_solve(const double *__restrict__ Lc, const double (&r)[9], double (&z)[9]) {
    double l[kCholPacked];
#pragma unroll
    for (int k = 0; k < kCholPacked; ++k) l[k] = Lc[k];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double v = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= l[tri9(i, k)] * z[k];
        z[i] = v * l[tri9(i, i)];
    }
#pragma unroll
    for (int i = 8; i >= 0; --i) {
        double v = z[i];
#pragma unroll
        for (int k = i + 1; k < 9; ++k) v -= l[tri9(k, i)] * z[k];
        z[i] = v * l[tri9(i, i)];
    }
}

// FIRST: r holds b; x = 0, z = M^-1 r, p = z.  Otherwise alpha = sc[rz] / sc[pq] (no update at all unless pq > 0 and
// alpha is finite: the host then reports a breakdown with x the last good iterate): x += alpha p, r -= alpha q,
// z = M^-1 r.  Both: r.r and r.z leave as one partial per workgroup (part_rr, part_rz).
template <bool FIRST>
__global__ __launch_bounds__(kSchurBlock) void k_pcg_update(
    int64_t n_cam, const double *__restrict__ Lf, const double *__restrict__ sc, int rz_slot, double *__restrict__ x,
    double *__restrict__ r, double *__restrict__ p, const double *__restrict__ q, double *__restrict__ z,
    double *__restrict__ part_rr, double *__restrict__ part_rz) {
    __shared__ double sRed[2][4];
    const int64_t c = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if (c < n_cam) {
        double rc[9], zc[9];
        bool go = true;
        double alpha = 0.0;
        if (!FIRST) {
            const double pq = sc[kScPq];
            alpha = sc[rz_slot] / pq;
            go = pq > 0.0 && isfinite(alpha);
        }
        if (go) {
#pragma unroll
            for (int k = 0; k < 9; ++k) rc[k] = r[c * 9 + k];
            if (FIRST) {
#pragma unroll
                for (int k = 0; k < 9; ++k) x[c * 9 + k] = 0.0;
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const double pk = p[c * 9 + k];
                    x[c * 9 + k] += alpha * pk;
                    rc[k] -= alpha * q[c * 9 + k];
                    r[c * 9 + k] = rc[k];
                }
            }
            chol9_solve(Lf + c * kCholPacked, rc, zc);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (FIRST) p[c * 9 + k] = zc[k];
                else z[c * 9 + k] = zc[k];
                rr += rc[k] * rc[k];
                rz += rc[k] * zc[k];
            }
        }
    }
    block_sum_to(rr, sRed[0], part_rr + blockIdx.x);
    block_sum_to(rz, sRed[1], part_rz + blockIdx.x);
}

// p = z + beta p over n doubles
__global__ __launch_bounds__(kSchurBlock) void k_pcg_direction(int64_t n, double beta, const double *__restrict__ z, double *__restrict__ p) {
    const int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (i < n) p[i] = z[i] + beta * p[i];
}

// ---- Schur-Jacobi preconditioner ----------------------------------------------------------------------
// M_c = lam diag(d_c) + sum_o Jc_o^T (I2 - Jp_o V_l,p(o)^-1 Jp_o^T) Jc_o over the camera's list: the 9x9 diagonal block of
// S when no camera sees a point twice.  Every term is positive semi-definite (V_l >= Jp_o^T Jp_o) and is accumulated as
// such: nothing is subtracted from U_l, so nothing cancels at small lam.  The layout of k_normal_cameras (16 lanes per
// camera, the xor tree, the packed sums staged in LDS for the 81 stores) on the grid of k_schur_cameras (one wave per four
// cameras).  Per observation: V_l,p = L L^T in registers as in k_schur_points, y_a = L^-1 Jp_a^T for the two rows a of
// Jp, F = I2 - [y_a . y_b].  d_c is read from U's diagonal when the block is written.
constexpr int kScFallback = 6;                    // device scalar of a solve: cameras whose Schur-Jacobi factor fell back
static_assert(kScFallback > kScModel && kScFallback < kScSlots, "kScFallback must be a free slot of c2b_problem::sv_sc");

template <class... Loss>
__global__ __launch_bounds__(kNormBlock) void k_schur_jacobi(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint64_t *__restrict__ row_ptr, int n_cam,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, const double *__restrict__ U,
    const double *__restrict__ V, double lam, double *__restrict__ M, Loss... loss) {
    constexpr int kWaves = kNormBlock / 64;
    __shared__ double sAcc[kWaves * kNormCamsPerWave * kNormSym];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / kNormG, gl = lane % kNormG;
    double *mine = sAcc + (wave * kNormCamsPerWave + grp) * kNormSym;
    const int q = (int)blockIdx.x * kWaves + wave;                   // one wave per kNormCamsPerWave cameras, no grid-stride loop
    const int c = q * kNormCamsPerWave + grp;
    const bool cam_ok = c < n_cam;
    const uint64_t b = cam_ok ? row_ptr[c] : 0, e = cam_ok ? row_ptr[c + 1] : 0;
    const CamRef cam = cam_ref(camblk, cam_ok ? (uint32_t)c : 0u);
    double acc[kNormSym];
#pragma unroll
    for (int k = 0; k < kNormSym; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (uint64_t o = b + gl; o < e; o += kNormG) {
        const uint32_t pi = pt_idx[o];
        double r0, r1, jc[18], jp[6];
        jacobian_obs(cam, pts4[pi], uv_obs[o], r0, r1, jc, jp);
        if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
        // V_l = L L^T, L in registers
        const double *Vp = V + (int64_t)pi * 9;
        const Chol3 L = chol3_factor(damped(Vp[0], lam), Vp[3], Vp[6], damped(Vp[4], lam), Vp[7], damped(Vp[8], lam));
        double ya0, ya1, ya2, yb0, yb1, yb2;
        L.forward(jp[0], jp[1], jp[2], ya0, ya1, ya2);
        L.forward(jp[3], jp[4], jp[5], yb0, yb1, yb2);
        const double f00 = 1.0 - ((ya0 * ya0 + ya1 * ya1) + ya2 * ya2);
        const double f01 = -((ya0 * yb0 + ya1 * yb1) + ya2 * yb2);
        const double f11 = 1.0 - ((yb0 * yb0 + yb1 * yb1) + yb2 * yb2);
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const double g0 = f00 * jc[a] + f01 * jc[9 + a], g1 = f01 * jc[a] + f11 * jc[9 + a];
#pragma unroll
            for (int d = a; d < 9; ++d) acc[sym9(a, d)] += g0 * jc[d] + g1 * jc[9 + d];
        }
    }
    // fixed tree over the group's 16 lanes (xor: every lane ends with the same bits)
#pragma unroll
    for (int off = kNormG / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kNormSym; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
    }
    if (gl == 0) {
#pragma unroll
        for (int k = 0; k < kNormSym; ++k) mine[k] = acc[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (cam_ok) {
        // both triangles from one packed entry: M[a][d] and M[d][a] are the same bits; 16 lanes write a block of 81
        const double *Uc = U + (int64_t)c * 81;
        double *Mc = M + (int64_t)c * 81;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int i = gl + t * kNormG;
            if (i < 81) {
                const int a = i / 9, d = i % 9;
                const double s = mine[a <= d ? sym9(a, d) : sym9(d, a)];
                Mc[i] = a == d ? s + lam * fmin(fmax(Uc[i], 1e-6), 1e32) : s;
            }
        }
    }
}

// a (packed lower rows) to its Cholesky factor in place, the reciprocal of each diagonal entry in its place: the
// arithmetic of k_schur_factor.  False when a pivot is not finite or not > 0 (a then holds no factor): an entry that is
// not finite reaches a later pivot, so the pivots alone decide.
C2B_DEV bool chol9_packed(double (&a)[kCholPacked]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        double d = a[tri9(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= a[tri9(j, k)] * a[tri9(j, k)];
        ok = ok && isfinite(d) && d > 0.0;
        const double inv = 1.0 / sqrt(d);
        a[tri9(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < 9; ++i) {
            double v = a[tri9(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= a[tri9(i, k)] * a[tri9(j, k)];
            a[tri9(i, j)] = v * inv;
        }
    }
    return ok;
}

// Lf[c] = the factor of M_c in k_schur_factor's format, so k_pcg_update and chol9_solve apply it unchanged.  A camera
// whose M_c has a pivot that is not finite or not > 0 gets the factor of U_l,c instead (the block-Jacobi one, by the same
// arithmetic); how many did leaves as one count per workgroup (a double holding an integer: k_normal_sum adds them exactly)
__global__ __launch_bounds__(kSchurBlock) void k_schur_factor_blocks(int64_t n_cam, const double *__restrict__ M,
                                                                     const double *__restrict__ U, double lam,
                                                                     double *__restrict__ Lf, double *__restrict__ part_fb) {
    __shared__ double sRed[4];
    const int64_t c = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    double fell = 0.0;
    if (c < n_cam) {
        const double *Mc = M + c * 81;
        double a[kCholPacked];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) a[tri9(i, j)] = Mc[i * 9 + j];
        }
        if (!chol9_packed(a)) {
            const double *Uc = U + c * 81;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) a[tri9(i, j)] = i == j ? damped(Uc[i * 9 + j], lam) : Uc[i * 9 + j];
            }
            (void)chol9_packed(a);
            fell = 1.0;
        }
        double *Lc = Lf + c * kCholPacked;
#pragma unroll
        for (int k = 0; k < kCholPacked; ++k) Lc[k] = a[k];
    }
    block_sum_to(fell, sRed, part_fb + blockIdx.x);
}

// ---- model decrease ---------------------------------------------------------------------------------------------
// per observation e = Jc dc + Jp dp: |r|^2 and |r|^2 - |r + e|^2 = -(2r + e).e, one partial of each per workgroup
template <class... Loss>
__global__ __launch_bounds__(kSchurBlock) void k_schur_model(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint32_t *__restrict__ cam_idx,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, int64_t n_obs, const double *__restrict__ dc,
    const double *__restrict__ dp, double *__restrict__ part_sq, double *__restrict__ part_md, Loss... loss) {
    __shared__ double sRed[2][4];
    const int64_t o = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    double sq = 0.0, md = 0.0;
    if (o < n_obs) {
        const uint32_t c = cam_idx[o], pi = pt_idx[o];
        double r0, r1, jc[18], jp[6];
        jacobian_obs(cam_ref(camblk, c), pts4[pi], uv_obs[o], r0, r1, jc, jp);
        if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
        const double *dcc = dc + (int64_t)c * 9, *dpp = dp + (int64_t)pi * 3;
        double e0 = 0.0, e1 = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            e0 += jc[k] * dcc[k];
            e1 += jc[9 + k] * dcc[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            e0 += jp[k] * dpp[k];
            e1 += jp[3 + k] * dpp[k];
        }
        sq = r0 * r0 + r1 * r1;
        md = -((2.0 * r0 + e0) * e0 + (2.0 * r1 + e1) * e1);
    }
    block_sum_to(sq, sRed[0], part_sq + blockIdx.x);
    block_sum_to(md, sRed[1], part_md + blockIdx.x);
}

// ---- constant parameters --------------------------------------------------------------------------------
// A camera's mask has bit k set when its parameter k (to_vec order) is constant; a point's is 0 or 1.  The solve is that
// of J~, J with those columns zero.  The passes above keep J: these kernels put the zeros where J~ has them, after the
// pass.  They store and never load what they mask: an entity with nothing constant costs its mask word and no more.
constexpr double kConstPointV = __builtin_huge_val();      // the diagonal of a constant point's V while k_schur_jacobi reads it

// y[c][k] = 0 where bit k of cam_mask[c] is set: y = b or q after a camera pass, or gc.  One lane per camera.
__global__ __launch_bounds__(kSchurBlock) void k_const_cameras(int64_t n_cam, const uint16_t *__restrict__ cam_mask,
                                                               double *__restrict__ y) {
    const int64_t c = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (c >= n_cam) return;
    const unsigned m = cam_mask[c];
    if (!m) return;
    double *yc = y + c * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if ((m >> k) & 1u) yc[k] = 0.0;
}

// t[p] = 0 for a constant point: t after a point pass (V_l^-1 = 1e6 / lam would multiply W^T x into it), or dp.
__global__ __launch_bounds__(kSchurBlock) void k_const_points(int64_t n_pts, const uint8_t *__restrict__ pt_mask,
                                                              double *__restrict__ t) {
    const int64_t p = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (p >= n_pts || !pt_mask[p]) return;
    t[3 * p] = 0.0; t[3 * p + 1] = 0.0; t[3 * p + 2] = 0.0;
}

// A [n_cam][9][9] = U or M: row and column k of a camera's block to 0 where bit k is set, the diagonal entry to `diag`
// (U: 0; M: lam 1e-6, the damping of a diagonal of 0, which is all J~ leaves there).  One lane per row of a block.
__global__ __launch_bounds__(kSchurBlock) void k_const_blocks(int64_t n_rows, const uint16_t *__restrict__ cam_mask, double diag,
                                                              double *__restrict__ A) {
    const int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t c = i / 9;
    const int row = (int)(i - c * 9);
    const unsigned m = cam_mask[c];
    if (!m) return;
    const bool whole = (m >> row) & 1u;
    double *Ar = A + i * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if (whole || ((m >> k) & 1u)) Ar[k] = (whole && k == row) ? diag : 0.0;
}

// V [n_pts][3][3] (and gp [n_pts][3] unless NULL) of a constant point: V = diag I3, gp = 0.  diag = 0 is J~'s V; diag =
// kConstPointV (+inf) is what k_schur_jacobi is given: the reciprocals of L's diagonal are then 0, L^-1 Jp^T is 0 and
// I2 - Jp V_l^-1 Jp^T is I2 to the bit, which is the term of an observation whose Jp is 0.
__global__ __launch_bounds__(kSchurBlock) void k_const_point_blocks(int64_t n_pts, const uint8_t *__restrict__ pt_mask, double diag,
                                                                    double *__restrict__ V, double *__restrict__ gp) {
    const int64_t p = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (p >= n_pts || !pt_mask[p]) return;
    double *Vp = V + p * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) Vp[k] = (k % 4 == 0) ? diag : 0.0;
    if (gp) { gp[3 * p] = 0.0; gp[3 * p + 1] = 0.0; gp[3 * p + 2] = 0.0; }
}

// ---- apply -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSchurBlock) void k_add_f64(int64_t n, const double *__restrict__ d, double *__restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (i < n) a[i] += d[i];
}

__global__ __launch_bounds__(kSchurBlock) void k_points_add(int64_t n_pts, const double *__restrict__ dp, double4 *__restrict__ pts4) {
    const int64_t p = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (p >= n_pts) return;
    double4 X = pts4[p];
    X.x += dp[3 * p]; X.y += dp[3 * p + 1]; X.z += dp[3 * p + 2];
    pts4[p] = X;
}

// the two above over the free entries only: a constant one keeps its bits whatever d holds there (-0 + 0 is +0)
__global__ __launch_bounds__(kSchurBlock) void k_add_free(int64_t n, const double *__restrict__ d, const uint16_t *__restrict__ cam_mask,
                                                          double *__restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t c = i / 9;
    if (!((cam_mask[c] >> (int)(i - c * 9)) & 1u)) a[i] += d[i];
}

__global__ __launch_bounds__(kSchurBlock) void k_points_add_free(int64_t n_pts, const double *__restrict__ dp,
                                                                 const uint8_t *__restrict__ pt_mask, double4 *__restrict__ pts4) {
    const int64_t p = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (p >= n_pts || pt_mask[p]) return;
    double4 X = pts4[p];
    X.x += dp[3 * p]; X.y += dp[3 * p + 1]; X.z += dp[3 * p + 2];
    pts4[p] = X;
}

// ---- what the Levenberg-Marquardt loop's stopping tests read ---------------------------------------------
// Both kernels run on lm_grid(n) workgroups, n the longer of their two index ranges: one lane per entry up to kLmGridCap
// workgroups, a grid-stride walk beyond.  A lane's entries and the order it adds them in depend on the counts alone, so
// the same problem gives the same bits.  Lanes past an array's end (the tail wave; every lane of an empty array) carry the
// identity, 0: an empty problem writes partials of 0 and never reads.
constexpr int kLmGridCap = 2048;                  // 8 workgroups of 256 on each of the 256 CUs
enum { kLmStepCam = 0, kLmStepPts = 1, kLmXCam = 2, kLmXPts = 3, kLmSums = 4 };

inline unsigned lm_grid(int64_t n) {
    const int64_t g = (n + kSchurBlock - 1) / kSchurBlock;
    return (unsigned)(g < 1 ? 1 : (g > kLmGridCap ? kLmGridCap : g));
}

// |dc|^2, |dp|^2, |bal9|^2, |points|^2 in one pass: partial k of workgroup b at part[k * gridDim.x + b] (k in the enum's
// order), each then summed by k_normal_sum.  A point's fourth lane is padding and is never added.  A constant entry's step
// is already exactly 0 (c2b_problem_solve_step), so no mask is read.
__global__ __launch_bounds__(kSchurBlock) void k_lm_norms(int64_t n_cam9, int64_t n_pts, const double *__restrict__ bal9,
                                                          const double4 *__restrict__ pts4, const double *__restrict__ dc,
                                                          const double *__restrict__ dp, double *__restrict__ part) {
    __shared__ double sRed[kLmSums][4];
    const int64_t stride = (int64_t)gridDim.x * kSchurBlock, n = n_cam9 > n_pts ? n_cam9 : n_pts;
    double s[kLmSums] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x; i < n; i += stride) {
        if (i < n_cam9) {
            const double d = dc[i], x = bal9[i];
            s[kLmStepCam] += d * d;
            s[kLmXCam] += x * x;
        }
        if (i < n_pts) {
            const double4 X = pts4[i];
            const double d0 = dp[3 * i], d1 = dp[3 * i + 1], d2 = dp[3 * i + 2];
            s[kLmStepPts] += (d0 * d0 + d1 * d1) + d2 * d2;
            s[kLmXPts] += (X.x * X.x + X.y * X.y) + X.z * X.z;
        }
    }
#pragma unroll
    for (int k = 0; k < kLmSums; ++k) {
        const double w = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) sRed[k][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x < kLmSums) {
        const double *r = sRed[threadIdx.x];
        part[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

// the larger of two magnitudes, a NaN on either side kept (fmax would drop it): once m is a NaN no comparison replaces it
C2B_DEV double max_keep_nan(double m, double v) { return (v > m || v != v) ? v : m; }

C2B_DEV double wave_max_keep_nan(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max_keep_nan(v, __shfl_down(v, off, 64));
    return v;
}

// max |gc_i| over n_gc entries and max |gp_i| over n_gp: workgroup b's pair at part[b] and part[gridDim.x + b].  A max does
// not depend on the order, so the result is exact; a NaN anywhere reaches the result.
__global__ __launch_bounds__(kSchurBlock) void k_lm_gradient_max(int64_t n_gc, int64_t n_gp, const double *__restrict__ gc,
                                                                 const double *__restrict__ gp, double *__restrict__ part) {
    __shared__ double sRed[2][4];
    const int64_t stride = (int64_t)gridDim.x * kSchurBlock, n = n_gc > n_gp ? n_gc : n_gp;
    double mc = 0.0, mp = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x; i < n; i += stride) {
        if (i < n_gc) mc = max_keep_nan(mc, fabs(gc[i]));
        if (i < n_gp) mp = max_keep_nan(mp, fabs(gp[i]));
    }
    mc = wave_max_keep_nan(mc);
    mp = wave_max_keep_nan(mp);
    if ((threadIdx.x & 63) == 0) { sRed[0][threadIdx.x >> 6] = mc; sRed[1][threadIdx.x >> 6] = mp; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *r = sRed[threadIdx.x];
        part[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = max_keep_nan(max_keep_nan(r[0], r[1]), max_keep_nan(r[2], r[3]));
    }
}

// the two maxima of k_lm_gradient_max's partials (n per kind) into out[0], out[1]: one workgroup
__global__ __launch_bounds__(kSchurBlock) void k_lm_max_fold(const double *__restrict__ part, int n, double *__restrict__ out) {
    __shared__ double sRed[2][4];
    double m[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < n; k += kSchurBlock) {
        m[0] = max_keep_nan(m[0], part[k]);
        m[1] = max_keep_nan(m[1], part[n + k]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double w = wave_max_keep_nan(m[j]);
        if ((threadIdx.x & 63) == 0) sRed[j][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *r = sRed[threadIdx.x];
        out[threadIdx.x] = max_keep_nan(max_keep_nan(r[0], r[1]), max_keep_nan(r[2], r[3]));
    }
}

}  // namespace c2b
