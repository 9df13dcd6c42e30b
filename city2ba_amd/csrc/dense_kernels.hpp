// dense_kernels.hpp -- gfx950 kernels of the DIRECT solve of the reduced camera system (included by capi.hip only, after
// schur_explicit_kernels.hpp).
//
// The explicit Schur complement (schur_explicit_kernels.hpp) leaves S in block-CSR.  These kernels scatter it into a dense
// lower triangle A [Np][ld], row-major, Np = 64 ceil(9 n_cam / 64) <= ld, factor A = L L^T in place by a right-looking blocked
// Cholesky on 64 x 64 tiles and solve L L^T x = b by two blocked substitutions.  Only the lower triangle (diagonal included)
// is read or written; the padding rows i >= 9 n_cam are rows of the identity before and after.
//   * k_dense_scatter: one wave per camera c (k_schur_spmv's mapping: lane l holds entries l and l + 64 of a block) owns the
//     rows 9c .. 9c + 8 up to the diagonal block: it walks c's ascending neighbours c' < c, stores each block at column 9c' and
//     zeros in the gaps between them, then S_cc.  The waves past the cameras write the padding rows.  Every entry is written
//     once, by one lane.
//   * k_chol_panel: one workgroup factors the diagonal tile in LDS, column by column.  A pivot that is not finite or not > 0
//     leaves its 1-based index in *info (the first only: one lane, an ordinary store) and is replaced by 1, so that what is
//     queued behind runs to its end on garbage: no address depends on matrix data.
//   * k_chol_trsm: a workgroup per 64-row tile below the panel, a lane per row, the row in registers: X L11^T = A21 by
//     substitution with the divisions a substitution has (no inverse of L11 is formed).
//   * k_chol_syrk: C_ij -= L_i L_j^T over the lower tile pairs of the trailing matrix by v_mfma_f64_16x16x4_f64; four waves
//     per workgroup, a wave per 32 x 32 quadrant as 2 x 2 MFMA tiles: four independent accumulators that start from C and take
//     16 k-steps each in ascending k, the A operand negated (exact).  C/D: col = lane & 15, row = (lane >> 4) + 4 reg; A / B:
//     one f64 per lane, row or column lane & 15 at k = lane >> 4.  The two panel tiles are staged through LDS, coalesced in and
//     swizzled (measured against operands straight from L2: DESIGN 4.23); the wave of a diagonal tile's upper quadrant leaves
//     after the barrier.
//   * k_chol_solve_tile<TRANS> / k_chol_solve_update<TRANS>: per 64-row panel, one wave solves the triangular tile in LDS,
//     then a workgroup per remaining tile subtracts the tile's product from the rest of the right-hand side: 4 partial sums of
//     16 terms in ascending order, combined as (p0 + p1) + (p2 + p3).
//   * k_dense_residual: the partials of |b - q|^2 and |b|^2 for k_normal_sum.
// Every product-sum is an explicit fma in a fixed order; no float atomics, no scratch: the same inputs give the same bits.
#pragma once
#include "schur_explicit_kernels.hpp"

namespace c2b {

constexpr int kDnTile = 64;                                  // the tile edge of every kernel here
constexpr int kDnBlock = 256;
constexpr int kDnScatterWaves = 4;                           // cameras (or padding rows) per workgroup of k_dense_scatter
constexpr int kDnPad = kDnTile + 1;                          // row stride of an LDS tile read by columns

typedef double dn_f64x4 __attribute__((ext_vector_type(4)));

// ---- S into the dense lower triangle ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kDnScatterWaves * 64) void k_dense_scatter(const uint64_t *__restrict__ nbr_ptr, const uint32_t *__restrict__ nbr,
                                                                        int64_t n_cam, const double *__restrict__ S_diag,
                                                                        const double *__restrict__ S_off, double *__restrict__ A, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kDnScatterWaves + (threadIdx.x >> 6);
    const int64_t N = 9 * n_cam, Np = (N + kDnTile - 1) / kDnTile * kDnTile;
    if (w >= n_cam) {                                                        // a padding row: zeros, then 1 on the diagonal
        const int64_t i = N + (w - n_cam);
        if (i >= Np) return;
        double *row = A + i * ld;
        for (int64_t col = lane; col < i; col += 64) row[col] = 0.0;
        if (lane == 0) row[i] = 1.0;
        return;
    }
    const int64_t c = w;
    const SxLane ln(lane);
    double *rows = A + 9 * c * ld;                                           // rows 9c .. 9c + 8; columns [0, 9c + 9) are this wave's
    int64_t done = 0;                                                        // columns [0, done) are written
    const uint64_t ne = nbr_ptr[c + 1];
#pragma unroll 1
    for (uint64_t e = nbr_ptr[c]; e < ne; ++e) {                             // ascending neighbours; wave-uniform
        const int64_t q = (int64_t)nbr[e];
        if (q >= c) break;
        const int64_t at = 9 * q;
        if (at < done) continue;                                             // (not an ascending row: never outside [0, 9c))
        for (int r = 0; r < 9; ++r)
            for (int64_t col = done + lane; col < at; col += 64) rows[r * ld + col] = 0.0;
        const double *B = S_off + e * 81;
        rows[ln.i0 * ld + at + ln.j0] = B[lane];
        if (ln.two) rows[ln.i1 * ld + at + ln.j1] = B[lane + 64];
        done = at + 9;
    }
    for (int r = 0; r < 9; ++r)
        for (int64_t col = done + lane; col < 9 * c; col += 64) rows[r * ld + col] = 0.0;
    const double *D = S_diag + c * 81;
    rows[ln.i0 * ld + 9 * c + ln.j0] = D[lane];
    if (ln.two) rows[ln.i1 * ld + 9 * c + ln.j1] = D[lane + 64];
}

// ---- the factorisation -----------------------------------------------------------------------------------------------
// the diagonal tile at (k0, k0)
__global__ __launch_bounds__(kDnBlock) void k_chol_panel(double *__restrict__ A, int64_t ld, int64_t k0, int *__restrict__ info) {
    __shared__ double sT[kDnTile * kDnPad];
    __shared__ double sPiv[kDnTile];
    const int t = threadIdx.x;
    double *tile = A + k0 * ld + k0;
    for (int idx = t; idx < kDnTile * kDnTile; idx += kDnBlock) {
        const int r = idx >> 6, c = idx & 63;
        sT[r * kDnPad + c] = c <= r ? tile[r * ld + c] : 0.0;
    }
    bool failed = false;
    if (t == 0) failed = *info != 0;                                         // a pivot of an earlier panel failed: that one stays
    __syncthreads();
    const int i = t >> 2, q = t & 3;
#pragma unroll 1
    for (int j = 0; j < kDnTile; ++j) {
        if (t < kDnTile) {                                                   // the first wave: column j
            const double d = sT[j * kDnPad + j];
            const bool ok = d > 0.0 && d < __builtin_inf();
            const double piv = ok ? sqrt(d) : 1.0;
            if (t == 0 && !ok && !failed) {
                failed = true;
                *info = (int)(k0 + j + 1);
            }
            if (t > j) sT[t * kDnPad + j] = sT[t * kDnPad + j] / piv;
            if (t == j) sPiv[j] = piv;
        }
        __syncthreads();
        if (i > j) {                                                         // the trailing rows: entries (i, k), j < k <= i
            const double lij = sT[i * kDnPad + j];
            for (int k = j + 1 + q; k <= i; k += 4) sT[i * kDnPad + k] = fma(-lij, sT[k * kDnPad + j], sT[i * kDnPad + k]);
        }
        __syncthreads();
    }
    for (int idx = t; idx < kDnTile * kDnTile; idx += kDnBlock) {
        const int r = idx >> 6, c = idx & 63;
        if (c < r) tile[r * ld + c] = sT[r * kDnPad + c];
        else if (c == r) tile[r * ld + c] = sPiv[r];
    }
}

// the tiles (k0 + 64 (1 + blockIdx.x), k0): X L11^T = A21, a lane per row
__global__ __launch_bounds__(kDnTile) void k_chol_trsm(double *__restrict__ A, int64_t ld, int64_t k0) {
    __shared__ double sLt[kDnTile * kDnPad];                                 // sLt[j][k] = L11[k][j], k >= j
    const int lane = threadIdx.x;
    const double *L11 = A + k0 * ld + k0;
    for (int r = 0; r < kDnTile; ++r) sLt[lane * kDnPad + r] = r >= lane ? L11[r * ld + lane] : 0.0;
    __syncthreads();
    double *row = A + (k0 + kDnTile * (1 + (int64_t)blockIdx.x) + lane) * ld + k0;
    double x[kDnTile];
#pragma unroll
    for (int j = 0; j < kDnTile; ++j) x[j] = row[j];
#pragma unroll
    for (int j = 0; j < kDnTile; ++j) {
        x[j] = x[j] / sLt[j * kDnPad + j];
#pragma unroll
        for (int k = j + 1; k < kDnTile; ++k) x[k] = fma(-x[j], sLt[j * kDnPad + k], x[k]);
    }
#pragma unroll
    for (int j = 0; j < kDnTile; ++j) row[j] = x[j];
}

// the lower tile pair `b` of m tile rows: (i, j), j <= i, b = i (i + 1) / 2 + j
C2B_DEV void dn_tile_pair(unsigned b, int &i, int &j) {
    int r = (int)((sqrtf(8.0f * (float)b + 1.0f) - 1.0f) * 0.5f);
    while ((unsigned)r * (unsigned)(r + 1) / 2 > b) --r;
    while ((unsigned)(r + 1) * (unsigned)(r + 2) / 2 <= b) ++r;
    i = r;
    j = (int)(b - (unsigned)r * (unsigned)(r + 1) / 2);
}

// the trailing matrix behind panel k0: tile (i, j) -= L_i L_j^T, L_i = the tile (k0 + 64 (1 + i), k0)
__global__ __launch_bounds__(kDnBlock) void k_chol_syrk(double *__restrict__ A, int64_t ld, int64_t k0) {
    __shared__ double sOp[2 * kDnTile * kDnTile];                            // L_i, then L_j: 64 KiB, two workgroups a CU
    int ti, tj;
    dn_tile_pair(blockIdx.x, ti, tj);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = wave >> 1, qj = wave & 1;
    const bool diag = ti == tj;
    {                                                                        // both panel tiles into LDS, column swizzled by 2 (row & 15)
        const double *Ti = A + (k0 + kDnTile * (1 + (int64_t)ti)) * ld + k0, *Tj = A + (k0 + kDnTile * (1 + (int64_t)tj)) * ld + k0;
        for (int idx = threadIdx.x; idx < kDnTile * kDnTile; idx += kDnBlock) {
            const int r = idx >> 6, c = idx & 63, at = r * kDnTile + (c ^ (2 * (r & 15)));
            sOp[at] = Ti[r * ld + c];
            sOp[kDnTile * kDnTile + at] = Tj[r * ld + c];
        }
        __syncthreads();
    }
    if (diag && qj > qi) return;                                             // the upper quadrant of a diagonal tile (wave-uniform)
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t row0 = k0 + kDnTile * (1 + (int64_t)ti) + 32 * qi, col0 = k0 + kDnTile * (1 + (int64_t)tj) + 32 * qj;
    dn_f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 16 * a + lk + 4 * r, col = col0 + 16 * b + lr;
                acc[a][b][r] = col <= row ? A[row * ld + col] : 0.0;         // (only a diagonal tile has col > row)
            }
    // the operands of the 16 k-steps: a half-wave's 32 reads of 8 bytes fall on 32 distinct doubles of a 256-byte window (conflict-free)
    double a0[kDnTile / 4], a1[kDnTile / 4], b0[kDnTile / 4], b1[kDnTile / 4];
#pragma unroll
    for (int kk = 0; kk < kDnTile / 4; ++kk) {
        const int c = (4 * kk + lk) ^ (2 * lr);
        const double *sI = sOp + (32 * qi + lr) * kDnTile + c, *sJ = sOp + kDnTile * kDnTile + (32 * qj + lr) * kDnTile + c;
        a0[kk] = sI[0];
        a1[kk] = sI[16 * kDnTile];
        b0[kk] = sJ[0];
        b1[kk] = sJ[16 * kDnTile];
    }
#pragma unroll
    for (int kk = 0; kk < kDnTile / 4; ++kk) {                               // ascending k
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0[kk], b0[kk], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0[kk], b1[kk], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1[kk], b0[kk], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1[kk], b1[kk], acc[1][1], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 16 * a + lk + 4 * r, col = col0 + 16 * b + lr;
                if (col <= row) A[row * ld + col] = acc[a][b][r];
            }
}

// ---- the substitutions -----------------------------------------------------------------------------------------------
// x [k0, k0 + 64) <- L_kk^-1 x (TRANS: L_kk^-T x): one wave, a lane per unknown, the tile in LDS
template <bool TRANS>
__global__ __launch_bounds__(kDnTile) void k_chol_solve_tile(const double *__restrict__ A, int64_t ld, int64_t k0, double *__restrict__ x) {
    __shared__ double sL[kDnTile * kDnPad];
    const int lane = threadIdx.x;
    const double *tile = A + k0 * ld + k0;
    for (int r = 0; r < kDnTile; ++r) sL[r * kDnPad + lane] = lane <= r ? tile[r * ld + lane] : 0.0;
    __syncthreads();
    double xi = x[k0 + lane];
    const double d = sL[lane * kDnPad + lane];
#pragma unroll 1
    for (int s = 0; s < kDnTile; ++s) {
        const int j = TRANS ? kDnTile - 1 - s : s;
        if (lane == j) xi = xi / d;
        const double xj = __shfl(xi, j, 64);
        if (TRANS ? lane < j : lane > j) xi = fma(-(TRANS ? sL[j * kDnPad + lane] : sL[lane * kDnPad + j]), xj, xi);
    }
    x[k0 + lane] = xi;
}

// forward: x [r0, r0 + 64) -= L (r0, k0) x [k0, k0 + 64), r0 = k0 + 64 (1 + blockIdx.x); TRANS: x [c0, c0 + 64) -= L (k0, c0)^T
// x [k0, k0 + 64), c0 = 64 blockIdx.x
template <bool TRANS>
__global__ __launch_bounds__(kDnBlock) void k_chol_solve_update(const double *__restrict__ A, int64_t ld, int64_t k0, double *__restrict__ x) {
    __shared__ double sP[4][kDnTile];
    const int t = threadIdx.x;
    const double *xk = x + k0;
    if (!TRANS) {
        const int r = t >> 2, q = t & 3;                                     // four lanes of a wave per row
        const int64_t r0 = k0 + kDnTile * (1 + (int64_t)blockIdx.x);
        const double *L = A + (r0 + r) * ld + k0 + 16 * q;
        double p = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) p = fma(L[c], xk[16 * q + c], p);
        p = p + __shfl_xor(p, 1, 64);
        p = p + __shfl_xor(p, 2, 64);
        if (q == 0) x[r0 + r] = x[r0 + r] - p;
    } else {
        const int c = t & 63, q = t >> 6;                                    // a wave per 16 rows of the tile
        const int64_t c0 = kDnTile * (int64_t)blockIdx.x;
        const double *L = A + (k0 + 16 * q) * ld + c0 + c;
        double p = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) p = fma(L[r * ld], xk[16 * q + r], p);
        sP[q][c] = p;
        __syncthreads();
        if (q == 0) x[c0 + c] = x[c0 + c] - ((sP[0][c] + sP[1][c]) + (sP[2][c] + sP[3][c]));
    }
}

// ---- the true residual of the direct solve ---------------------------------------------------------------------------
// per workgroup |b - q|^2 into part_a and |b|^2 into part_b, q = S dc
__global__ __launch_bounds__(kSchurBlock) void k_dense_residual(int64_t n, const double *__restrict__ b, const double *__restrict__ q,
                                                                double *__restrict__ part_a, double *__restrict__ part_b) {
    __shared__ double sRed[2][4];
    const int64_t i = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    double d = 0.0, v = 0.0;
    if (i < n) {
        v = b[i];
        d = v - q[i];
    }
    block_sum_to(d * d, sRed[0], part_a + blockIdx.x);
    block_sum_to(v * v, sRed[1], part_b + blockIdx.x);
}

}  // namespace c2b
