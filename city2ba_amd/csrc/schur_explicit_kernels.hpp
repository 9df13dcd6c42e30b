// schur_explicit_kernels.hpp -- gfx950 kernels of the EXPLICIT Schur complement (included by capi.hip only, after
// schur_kernels.hpp and covis_kernels.hpp).
//
// schur_kernels.hpp applies S = U_l - W V_l^-1 W^T without forming it.  These kernels form it, in block-CSR on the camera
// covisibility graph at min_shared = 1 (nbr_ptr [n_cam + 1], nbr [n_edges] ascending, no self edge) plus the diagonal:
// S_diag [n_cam][9][9] and S_off [n_edges][9][9], row-major, BOTH (c, c') and (c', c) stored, the one the transpose of the
// other bit for bit.
//   * k_schur_y: per observation, Y_o = L_p^-1 Jp_o^T Jc_o (3x9, stored [o][3][9]) with V_l,p = L L^T factored in registers as
//     k_schur_points does, so that W_o V_l^-1 W_o'^T = Y_o^T Y_o' for two observations of one point.  Under a loss Jc and Jp
//     carry sqrt(w) each.  A constant point's V is kConstPointV: L^-1 = 0 and Y_o = 0.
//   * k_schur_blocks_light / _heavy: one owner per camera c walks its row in ascending observation; for an observation o of
//     (c, p) it walks p's track through the transpose in ascending position; an entry o' of a camera c' > c adds -Y_o^T Y_o'
//     to the block of (c, c'), found by binary search in c's ascending nbr row; an entry o' != o of c itself adds the same to
//     the diagonal block (the cross terms of a duplicated (camera, point) pair, which k_schur_jacobi's M_c leaves out).
//     Lane l of the owning wave holds entries l and l + 64 of EVERY 9x9 block (81 entries on 64 lanes: lanes 0..16 hold
//     two): an entry has one lane, its terms arrive in the walk's order, so nothing is reduced across lanes and nothing
//     depends on timing.  Light rows (degree <= kSxLdsBlocks): one wave, the blocks in LDS, written out once with their
//     transposes.  Heavy rows: a workgroup whose waves each own a contiguous range of the row's slots and accumulate in the
//     row's own S_off (ownership by slot, never by observation: the order of a block's terms stays the walk's); each
//     wave then writes its slots' transposes.  A pair (c, c') has ONE writer, the owner of min(c, c'): no races, no atomics.
//   * k_schur_spmv<DOT>: y_c = S_cc x_c + sum_e S_e x_nbr(e), one wave per camera, the blocks streamed 648 bytes at a time
//     (lane l reads entries l and l + 64), blocks added in ascending edge order, then each row's nine products in a fixed
//     tree; DOT also leaves x.y as one partial per wave.
//   * k_const_offdiag: constant parameters in the off-diagonal blocks: the rows of c's mask and the columns
//     of c''s to 0.  Stores zeros only and loads nothing of what it masks.
// No float atomics, no scratch: the same inputs give the same bits.
#pragma once
#include "covis_kernels.hpp"
#include "schur_kernels.hpp"

namespace c2b {

constexpr int kSxLdsBlocks = C2B_SCHUR_LDS_BLOCKS;           // blocks of a light row's LDS image: 648 bytes each
constexpr int kSxHeavyWaves = 4;                             // waves of a heavy row's workgroup
constexpr int kSxHeavyGrid = 1024;                           // workgroups striding over the cameras in search of heavy rows
constexpr int kSxSpmvWaves = 4;                              // cameras per workgroup of k_schur_spmv
static_assert(kSxLdsBlocks >= 1 && kSxLdsBlocks * 648 <= 64 * 1024, "a light row's image is a static LDS array");

// ---- Y ---------------------------------------------------------------------------------------------------------------
template <class... Loss>
__global__ __launch_bounds__(kSchurBlock) void k_schur_y(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint32_t *__restrict__ cam_idx,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, int64_t n_obs, const double *__restrict__ V,
    double lam, double *__restrict__ Y, Loss... loss) {
    const int64_t o = (int64_t)blockIdx.x * kSchurBlock + threadIdx.x;
    if (o >= n_obs) return;
    const uint32_t c = cam_idx[o], pi = pt_idx[o];
    double r0, r1, jc[18], jp[6];
    jacobian_obs(cam_ref(camblk, c), pts4[pi], uv_obs[o], r0, r1, jc, jp);
    if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
    // V_l = L L^T, L in registers
    const double *Vp = V + (int64_t)pi * 9;
    const Chol3 L = chol3_factor(damped(Vp[0], lam), Vp[3], Vp[6], damped(Vp[4], lam), Vp[7], damped(Vp[8], lam));
    double *Yo = Y + o * 27;
#pragma unroll
    for (int k = 0; k < 9; ++k) {                            // column k of Jp^T Jc, then L^-1 of it
        const double a0 = jp[0] * jc[k] + jp[3] * jc[9 + k];
        const double a1 = jp[1] * jc[k] + jp[4] * jc[9 + k];
        const double a2 = jp[2] * jc[k] + jp[5] * jc[9 + k];
        double y0, y1, y2;
        L.forward(a0, a1, a2, y0, y1, y2);
        Yo[k] = y0; Yo[9 + k] = y1; Yo[18 + k] = y2;
    }
}

// ---- the blocks ------------------------------------------------------------------------------------------------------
// the first slot of the ascending row nbr[b, e) whose camera is >= q (e when none is)
C2B_DEV uint64_t sx_lower(const uint32_t *__restrict__ nbr, uint64_t b, uint64_t e, uint32_t q) {
    while (b < e) {
        const uint64_t mid = (b + e) >> 1;
        if (nbr[mid] < q) b = mid + 1;
        else e = mid;
    }
    return b;
}

// the slot of camera q in the row, `none` when the row does not hold it
C2B_DEV uint64_t sx_find(const uint32_t *__restrict__ nbr, uint64_t b, uint64_t e, uint32_t q, uint64_t none) {
    const uint64_t s = sx_lower(nbr, b, e, q);
    return s < e && nbr[s] == q ? s : none;
}

// The entries a lane holds of every block: e0 = lane = (i0, j0) and, on lanes 0..16, e1 = lane + 64 = (i1, j1).
struct SxLane {
    int i0, j0, i1, j1;
    bool two;
    __device__ __forceinline__ explicit SxLane(int lane)
        : i0(lane / 9), j0(lane % 9), i1((lane + 64) / 9 % 9), j1((lane + 64) % 9), two(lane + 64 < 81) {}
};

// The walk of camera c's row [rb, re) by one wave: add(slot, t0, t1) for every term of a block (c, c'), c' > c, whose slot
// lies in [s_lo, s_hi), t0 / t1 the lane's two entries of -Y_o^T Y_o'; with DIAG the cross terms of c's duplicated pairs go
// to d0 / d1.  Every branch is wave-uniform.  [nb, ne) is c's row of the pattern; a camera the pattern does not hold (it
// then is not the covisibility graph of this list) is skipped.
template <class Add>
__device__ __forceinline__ void sx_walk(const uint32_t c, const uint64_t rb, const uint64_t re, const SxLane ln, const uint64_t s_lo, const uint64_t s_hi,
                                        const bool diag, const uint32_t *__restrict__ pt_idx, const uint64_t *__restrict__ pt_row_ptr,
                                        const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, const uint32_t *__restrict__ nbr,
                                        const uint64_t nb, const uint64_t ne, const double *__restrict__ Y, double &d0, double &d1, Add &&add) {
#pragma unroll 1
    for (uint64_t o = rb; o < re; ++o) {
        const uint32_t p = pt_idx[o];
        const uint64_t tb = pt_row_ptr[p], te = pt_row_ptr[p + 1];
        const double *Yo = Y + o * 27;
        const double a0 = Yo[ln.i0], a1 = Yo[9 + ln.i0], a2 = Yo[18 + ln.i0];
        const double b0 = Yo[ln.i1], b1 = Yo[9 + ln.i1], b2 = Yo[18 + ln.i1];
        uint32_t last = kCvEmpty;
        uint64_t slot = ne;
#pragma unroll 1
        for (uint64_t k = tb; k < te; ++k) {
            const uint32_t c2 = cam_of[k];
            if (c2 < c) continue;
            const uint64_t o2 = obs_of[k];
            if (c2 == c) {
                if (!diag || o2 == o) continue;
            } else {
                if (c2 != last) {                            // a track ascends in camera: the entries of one camera are adjacent
                    slot = sx_find(nbr, nb, ne, c2, ne);
                    last = c2;
                }
                if (slot < s_lo || slot >= s_hi) continue;
            }
            const double *Y2 = Y + o2 * 27;
            const double t0 = -((a0 * Y2[ln.j0] + a1 * Y2[9 + ln.j0]) + a2 * Y2[18 + ln.j0]);
            const double t1 = -((b0 * Y2[ln.j1] + b1 * Y2[9 + ln.j1]) + b2 * Y2[18 + ln.j1]);
            if (c2 == c) { d0 += t0; d1 += t1; }
            else add(slot, t0, t1);
        }
    }
}

// block `s` of row c as the lane holds it (v0, v1), stored at its slot and, transposed, at c's slot in the row of nbr[s]
__device__ __forceinline__ void sx_store_pair(const uint32_t c, const uint64_t s, const SxLane ln, const int lane, const double v0, const double v1,
                                              const uint64_t *__restrict__ nbr_ptr, const uint32_t *__restrict__ nbr, double *__restrict__ S_off) {
    double *at = S_off + s * 81;
    at[lane] = v0;
    if (ln.two) at[lane + 64] = v1;
    const uint32_t c2 = nbr[s];
    const uint64_t e2 = nbr_ptr[c2 + 1], none = ~0ull;
    const uint64_t ts = sx_find(nbr, nbr_ptr[c2], e2, c, none);
    if (ts == none) return;                                  // (a pattern that is not symmetric)
    double *tr = S_off + ts * 81;
    tr[ln.j0 * 9 + ln.i0] = v0;
    if (ln.two) tr[ln.j1 * 9 + ln.i1] = v1;
}

// One wave per camera whose degree fits the LDS image.  S_diag holds M_c on entry and S_cc on exit.
__global__ __launch_bounds__(64) void k_schur_blocks_light(const uint64_t *__restrict__ row_ptr, const uint32_t *__restrict__ pt_idx,
                                                           const uint64_t *__restrict__ pt_row_ptr, const uint32_t *__restrict__ obs_of,
                                                           const uint32_t *__restrict__ cam_of, const uint64_t *__restrict__ nbr_ptr,
                                                           const uint32_t *__restrict__ nbr, const double *__restrict__ Y,
                                                           double *__restrict__ S_diag, double *__restrict__ S_off) {
    __shared__ double sAcc[kSxLdsBlocks * 81];
    const int lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const uint64_t nb = nbr_ptr[c], ne = nbr_ptr[c + 1];
    if (ne - nb > (uint64_t)kSxLdsBlocks) return;            // a heavy row
    const uint64_t rb = row_ptr[c], re = row_ptr[c + 1];
    if (rb == re) return;
    const SxLane ln(lane);
    const uint64_t first = sx_lower(nbr, nb, ne, c);         // the slots of the cameras above c (no self edge)
    const int n_up = (int)(ne - first);
    // a lane reads and writes its own two entries of every block and no other: no barrier anywhere
    for (int s = 0; s < n_up; ++s) {
        sAcc[s * 81 + lane] = 0.0;
        if (ln.two) sAcc[s * 81 + lane + 64] = 0.0;
    }
    double d0 = 0.0, d1 = 0.0;
    sx_walk(c, rb, re, ln, first, ne, true, pt_idx, pt_row_ptr, obs_of, cam_of, nbr, nb, ne, Y, d0, d1, [&](uint64_t slot, double t0, double t1) {
        double *a = sAcc + (int)(slot - first) * 81;
        a[lane] += t0;
        if (ln.two) a[lane + 64] += t1;
    });
    for (int s = 0; s < n_up; ++s)
        sx_store_pair(c, first + (uint64_t)s, ln, lane, sAcc[s * 81 + lane], ln.two ? sAcc[s * 81 + lane + 64] : 0.0, nbr_ptr, nbr, S_off);
    double *Dc = S_diag + (int64_t)c * 81;
    Dc[lane] += d0;
    if (ln.two) Dc[lane + 64] += d1;
}

// The rows above the LDS budget: workgroups stride over the cameras, a workgroup per heavy row, wave w owning the w-th
// quarter of the row's upper slots and accumulating in S_off itself (a lane re-reads what it alone wrote).
__global__ __launch_bounds__(kSxHeavyWaves * 64) void k_schur_blocks_heavy(const uint64_t *__restrict__ row_ptr, const uint32_t *__restrict__ pt_idx,
                                                                          const uint64_t *__restrict__ pt_row_ptr, const uint32_t *__restrict__ obs_of,
                                                                          const uint32_t *__restrict__ cam_of, const uint64_t *__restrict__ nbr_ptr,
                                                                          const uint32_t *__restrict__ nbr, int64_t n_cam, const double *__restrict__ Y,
                                                                          double *__restrict__ S_diag, double *S_off) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SxLane ln(lane);
#pragma unroll 1
    for (int64_t cc = blockIdx.x; cc < n_cam; cc += gridDim.x) {             // workgroup-uniform
        const uint32_t c = (uint32_t)cc;
        const uint64_t nb = nbr_ptr[c], ne = nbr_ptr[c + 1];
        if (ne - nb <= (uint64_t)kSxLdsBlocks) continue;
        const uint64_t rb = row_ptr[c], re = row_ptr[c + 1];
        const uint64_t first = sx_lower(nbr, nb, ne, c);
        const uint64_t per = (ne - first + kSxHeavyWaves - 1) / kSxHeavyWaves;
        const uint64_t s_lo = first + per * (uint64_t)wave < ne ? first + per * (uint64_t)wave : ne;
        const uint64_t s_hi = s_lo + per < ne ? s_lo + per : ne;
        for (uint64_t s = s_lo; s < s_hi; ++s) {
            S_off[s * 81 + lane] = 0.0;
            if (ln.two) S_off[s * 81 + lane + 64] = 0.0;
        }
        double d0 = 0.0, d1 = 0.0;
        sx_walk(c, rb, re, ln, s_lo, s_hi, wave == 0, pt_idx, pt_row_ptr, obs_of, cam_of, nbr, nb, ne, Y, d0, d1, [&](uint64_t slot, double t0, double t1) {
            double *a = S_off + slot * 81;
            a[lane] += t0;
            if (ln.two) a[lane + 64] += t1;
        });
        for (uint64_t s = s_lo; s < s_hi; ++s)
            sx_store_pair(c, s, ln, lane, S_off[s * 81 + lane], ln.two ? S_off[s * 81 + lane + 64] : 0.0, nbr_ptr, nbr, S_off);
        if (wave == 0) {
            double *Dc = S_diag + (int64_t)c * 81;
            Dc[lane] += d0;
            if (ln.two) Dc[lane + 64] += d1;
        }
    }
}

// ---- the product -----------------------------------------------------------------------------------------------------
template <bool DOT>
__global__ __launch_bounds__(kSxSpmvWaves * 64) void k_schur_spmv(const uint64_t *__restrict__ nbr_ptr, const uint32_t *__restrict__ nbr, int64_t n_cam,
                                                                  const double *__restrict__ S_diag, const double *__restrict__ S_off,
                                                                  const double *__restrict__ x, double *__restrict__ y,
                                                                  double *__restrict__ block_part) {
    __shared__ double sProd[kSxSpmvWaves][81];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * kSxSpmvWaves + wave;             // one wave per camera, no grid-stride loop
    const bool cam_ok = c < n_cam;
    const SxLane ln(lane);
    double a0 = 0.0, a1 = 0.0;
    if (cam_ok) {
        const double *D = S_diag + c * 81, *xc = x + c * 9;
        a0 = D[lane] * xc[ln.j0];
        if (ln.two) a1 = D[lane + 64] * xc[ln.j1];
        const uint64_t ne = nbr_ptr[c + 1];
#pragma unroll 1
        for (uint64_t e = nbr_ptr[c]; e < ne; ++e) {                         // ascending edge order
            const double *B = S_off + e * 81, *xq = x + (int64_t)nbr[e] * 9;
            a0 += B[lane] * xq[ln.j0];
            if (ln.two) a1 += B[lane + 64] * xq[ln.j1];
        }
    }
    sProd[wave][lane] = a0;
    if (ln.two) sProd[wave][lane + 64] = a1;
    covis_wave_sync();
    double yv = 0.0, xv = 0.0;
    if (cam_ok && lane < 9) {                                                // row `lane`: its nine sums in a fixed tree
        const double *r = sProd[wave] + lane * 9;
        yv = (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) + r[8];
        y[c * 9 + lane] = yv;
        xv = x[c * 9 + lane];
    }
    if (DOT) {                                                               // the wave's x.y: 0 on lanes >= 9 and past n_cam
        const double w = wave_sum(xv * yv);
        if (lane == 0) block_part[(int64_t)blockIdx.x * kSxSpmvWaves + wave] = w;
    }
}

// ---- constant parameters --------------------------------------------------------------------------------
// S_off's blocks of row c: row k to 0 where bit k of cam_mask[c] is set, column k where bit k of cam_mask[nbr[e]] is.  One
// wave per camera, a lane per row of a block.
__global__ __launch_bounds__(256) void k_const_offdiag(const uint64_t *__restrict__ nbr_ptr, const uint32_t *__restrict__ nbr, int64_t n_cam,
                                                       const uint16_t *__restrict__ cam_mask, double *__restrict__ S_off) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_cam) return;
    const unsigned mr = cam_mask[c];
    const uint64_t nb = nbr_ptr[c], n9 = (nbr_ptr[c + 1] - nb) * 9;
    for (uint64_t t = lane; t < n9; t += 64u) {
        const uint64_t e = nb + t / 9;
        const int row = (int)(t % 9);
        const unsigned mc = cam_mask[nbr[e]];
        if (!(mr | mc)) continue;
        const bool whole = (mr >> row) & 1u;
        double *Ar = S_off + e * 81 + row * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (whole || ((mc >> k) & 1u)) Ar[k] = 0.0;
    }
}

}  // namespace c2b
