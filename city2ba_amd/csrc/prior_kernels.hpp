// prior_kernels.hpp -- priors on camera centres, intrinsics and points in the device LM step, gfx950, f64.
//
// Optional residual rows beside the observations', never reweighted by a loss (costs are sums of squares without a 1/2):
//   camera c:  r_C = w_C o (C - C0), C = -R^T t the centre of the camblk record (3 rows);  r_I = w_I o ((f, k1, k2) - I0) (3 rows)
//   point  p:  r_X = w_X o (X - X0) (3 rows)
// Weights are per component, finite and >= 0; a weight of 0 switches its row off and its target is never read into a result.
// With the step kernel's left-Jacobian convention (dR = [J_l dw]x R):  dC/dw = -R^T [t]x J_l,  dC/dt = -R^T, all of it in the
// record (kR, kT, kJl, kCenter): no trigonometry, no pow.  A = the 6x9 stack of diag(w_C) [dC/dw | -R^T | 0] and
// [0 | 0 | diag(w_I)]; its non-trivial part is the 3x6 block the kernels call A.
//   * k_prior_cameras: U_c += A^T A, gc_c += A^T r (either may be NULL); optionally r [n_cam][6] and A [n_cam][3][6] to the
//     caller; optionally the cost sum |r|^2 as one partial per workgroup.
//   * k_prior_points: V_p += diag(w_X^2), gp_p += w_X o r_X; optionally r [n_pts][3]; optionally the cost partials.
//   * k_prior_model: the prior part of a step's sum_sq and model_decrease, sum |r|^2 and sum -(2r + e).e with e = A delta.
// They follow the k_const_* kernels: streaming, kSchurBlock lanes, placed around the pinned passes, and a lane whose entity
// has every weight 0 loads no block.  No float atomics: the partials are summed by k_normal_sum in a fixed order, so the
// same inputs give the same bits.
//
// k_prior_cameras runs one lane per ROW of a camera's 9x9 block, as k_const_blocks does: the 39 entries of U a prior
// touches (the 6x6 pose block and the three intrinsics' diagonal) are the pass's traffic, a read-modify-write of 6 (or 1)
// consecutive doubles per lane with consecutive lanes on consecutive rows, so a wave's accesses cover whole lines of U.
// One lane per camera would stride 648 bytes between lanes.  The price is the record read and the 3x6 block formed by six
// lanes instead of one: 32 doubles from a line the neighbouring lanes share, and about 120 flops.
//
// Rounding of an entry of A (what tests/test_gpu_priors.py holds the device to), on its longest path:
//   m = t x J_l[:, j]        a product and a subtraction per term                                2 roundings
//   s = sum_i R[i][k] m_i    a product per term, two additions                                   3 roundings
//   A[k][j] = -(w_k s)       one product (the negation is exact)                                 1 rounding
// so |dA[k][j]| <= 6 u w_k sum_i |R[i][k]| (|t| x |J_l[:, j]|)_i to first order, u = 2^-53 (a contraction to FMA only
// removes roundings).  The translation columns take one rounding, a residual two.
#pragma once
#include "schur_kernels.hpp"

namespace c2b {

// r_C and the 3x6 block of one camera from its record (anything indexable by record double: the table in place, or an
// LDS-typed pointer); cw == NULL or a zero weight leaves that row 0 (its target unread)
template <typename P>
C2B_DEV void prior_center_rows(const P cam, const double *__restrict__ c0, const double w[3], double r[3], double A[18]) {
    const double t0 = cam[kT], t1 = cam[kT + 1], t2 = cam[kT + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = w[k] != 0.0 ? w[k] * (cam[kCenter + k] - c0[k]) : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double j0 = cam[kJl + j], j1 = cam[kJl + 3 + j], j2 = cam[kJl + 6 + j];
        const double m0 = t1 * j2 - t2 * j1, m1 = t2 * j0 - t0 * j2, m2 = t0 * j1 - t1 * j0;      // t x J_l[:, j]
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            A[k * 6 + j] = -(w[k] * ((cam[kR + k] * m0 + cam[kR + 3 + k] * m1) + cam[kR + 6 + k] * m2));
            A[k * 6 + 3 + j] = -(w[k] * cam[kR + 3 * j + k]);
        }
    }
}

C2B_DEV void prior_weights(const double *__restrict__ w, int64_t i, double out[3], bool &any) {
    out[0] = out[1] = out[2] = 0.0;
    if (w) { out[0] = w[3 * i]; out[1] = w[3 * i + 1]; out[2] = w[3 * i + 2]; }
    any = out[0] != 0.0 || out[1] != 0.0 || out[2] != 0.0;
}

// One lane per row of a camera's block (n_rows = 9 n_cam).  Rows 0..5 (pose) need the centre prior, rows 6..8 their own
// intrinsic's.  The lane of row 0 writes r_C, A and the centre's cost; the lanes of rows 6..8 their r_I and its cost.
__global__ __launch_bounds__(kSchurBlock) void k_prior_cameras(
    int64_t n_rows, const double *__restrict__ camblk, const double *__restrict__ c0, const double *__restrict__ cw,
    const double *__restrict__ i0, const double *__restrict__ iw, double *__restrict__ U, double *__restrict__ gc,
    double *__restrict__ r_out, double *__restrict__ A_out, double *__restrict__ part) {
    __shared__ double sRed[4];
    const int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    double cost = 0.0;
    if (i < n_rows) {
        const int64_t c = i / 9;
        const int row = (int)(i - c * 9);
        if (row < 6) {
            double w[3];
            bool any;
            prior_weights(cw, c, w, any);
            if (any) {
                double r[3], A[18];
                prior_center_rows(cam_ref(camblk, (uint32_t)c), c0 + 3 * c, w, r, A);
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;         // column `row` of A (a select per entry: no indexed registers)
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k == row) { a0 = A[k]; a1 = A[6 + k]; a2 = A[12 + k]; }
                if (U) {
                    double *Ur = U + i * 9;
#pragma unroll
                    for (int k = 0; k < 6; ++k) Ur[k] += (a0 * A[k] + a1 * A[6 + k]) + a2 * A[12 + k];
                }
                if (gc) gc[i] += (a0 * r[0] + a1 * r[1]) + a2 * r[2];
                if (row == 0) {
                    cost = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                    if (r_out) { r_out[6 * c] = r[0]; r_out[6 * c + 1] = r[1]; r_out[6 * c + 2] = r[2]; }
                    if (A_out) {
#pragma unroll
                        for (int k = 0; k < 18; ++k) A_out[18 * c + k] = A[k];
                    }
                }
            } else if (row == 0) {
                if (r_out) { r_out[6 * c] = 0.0; r_out[6 * c + 1] = 0.0; r_out[6 * c + 2] = 0.0; }
                if (A_out) {
#pragma unroll
                    for (int k = 0; k < 18; ++k) A_out[18 * c + k] = 0.0;
                }
            }
        } else {
            const int m = row - 6;
            const double w = iw ? iw[3 * c + m] : 0.0;
            double r = 0.0;
            if (w != 0.0) {
                r = w * (cam_ref(camblk, (uint32_t)c)[kIntr + m] - i0[3 * c + m]);
                if (U) U[i * 9 + row] += w * w;
                if (gc) gc[i] += w * r;
                cost = r * r;
            }
            if (r_out) r_out[6 * c + 3 + m] = r;
        }
    }
    if (part) block_sum_to(cost, sRed, part + blockIdx.x);
}

// One lane per point.
__global__ __launch_bounds__(kSchurBlock) void k_prior_points(
    int64_t n_pts, const double4 *__restrict__ pts4, const double *__restrict__ x0, const double *__restrict__ xw,
    double *__restrict__ V, double *__restrict__ gp, double *__restrict__ r_out, double *__restrict__ part) {
    __shared__ double sRed[4];
    const int64_t p = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    double cost = 0.0;
    if (p < n_pts) {
        double w[3], r[3] = {0.0, 0.0, 0.0};
        bool any;
        prior_weights(xw, p, w, any);
        if (any) {
            const double4 X = pts4[p];
            const double x[3] = {X.x, X.y, X.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (w[k] != 0.0) {
                    r[k] = w[k] * (x[k] - x0[3 * p + k]);
                    if (V) V[9 * p + 4 * k] += w[k] * w[k];
                    if (gp) gp[3 * p + k] += w[k] * r[k];
                }
            }
            cost = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        }
        if (r_out) { r_out[3 * p] = r[0]; r_out[3 * p + 1] = r[1]; r_out[3 * p + 2] = r[2]; }
    }
    if (part) block_sum_to(cost, sRed, part + blockIdx.x);
}

// One lane per index i over max(n_cam, n_pts): camera i's six rows and point i's three.  e = A delta; the lane's share of
// sum |r|^2 and of sum (|r|^2 - |r + e|^2) = sum -(2r + e).e, one partial of each per workgroup (k_schur_model's form).
__global__ __launch_bounds__(kSchurBlock) void k_prior_model(
    int64_t n_cam, const double *__restrict__ camblk, const double *__restrict__ c0, const double *__restrict__ cw,
    const double *__restrict__ i0, const double *__restrict__ iw, int64_t n_pts, const double4 *__restrict__ pts4,
    const double *__restrict__ x0, const double *__restrict__ xw, const double *__restrict__ dc, const double *__restrict__ dp,
    double *__restrict__ part_sq, double *__restrict__ part_md) {
    __shared__ double sRed[2][4];
    const int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    double sq = 0.0, md = 0.0;
    if (i < n_cam) {
        double w[3];
        bool any;
        prior_weights(cw, i, w, any);
        const double *d = dc + 9 * i;
        if (any) {
            double r[3], A[18];
            prior_center_rows(cam_ref(camblk, (uint32_t)i), c0 + 3 * i, w, r, A);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double e = 0.0;
#pragma unroll
                for (int j = 0; j < 6; ++j) e += A[6 * k + j] * d[j];
                sq += r[k] * r[k];
                md -= (2.0 * r[k] + e) * e;
            }
        }
        prior_weights(iw, i, w, any);
        if (any) {
            const CamRef cam = cam_ref(camblk, (uint32_t)i);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (w[k] != 0.0) {
                    const double r = w[k] * (cam[kIntr + k] - i0[3 * i + k]), e = w[k] * d[6 + k];
                    sq += r * r;
                    md -= (2.0 * r + e) * e;
                }
            }
        }
    }
    if (i < n_pts) {
        double w[3];
        bool any;
        prior_weights(xw, i, w, any);
        if (any) {
            const double4 X = pts4[i];
            const double x[3] = {X.x, X.y, X.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (w[k] != 0.0) {
                    const double r = w[k] * (x[k] - x0[3 * i + k]), e = w[k] * dp[3 * i + k];
                    sq += r * r;
                    md -= (2.0 * r + e) * e;
                }
            }
        }
    }
    block_sum_to(sq, sRed[0], part_sq + blockIdx.x);
    block_sum_to(md, sRed[1], part_md + blockIdx.x);
}

}  // namespace c2b
