// normal_kernels.hpp -- gfx950 kernels of the Gauss-Newton diagonal blocks (included by capi.hip only, after kernels.hpp).
//
// What a solver does first with J: U_c = sum Jc^T Jc (9x9) and g_c = sum Jc^T r per camera, V_p = sum Jp^T Jp (3x3) and
// g_p = sum Jp^T r per point.  These kernels form them from the per-observation Jacobian in registers (jacobian_obs, the
// step's own algebra, called, not copied) instead of writing J (208 B per observation) and reducing it again.
//   * k_normal_cameras: camera-major over the CSR list.  A group of kNormG = 16 lanes owns one camera: lane l of the group
//     accumulates observations b + l, b + l + 16, ... of the camera's list [b, e) (45 + 9 products), then a fixed xor tree
//     over the 16 lanes.  The summation order of a camera's block depends on its own list alone -- not on the grid, on
//     the other cameras or on the launch's offset -- so a shard's rows are the whole problem's bits.  The grid is fixed
//     by n_cam (grid-stride over groups of four cameras per wave); the sum of squared residuals leaves as one partial per
//     wave, summed in a fixed order by k_normal_sum (no float atomics; the ticket fold's extra scalar registers
//     would spill in this kernel).
//   * k_normal_points: point-major through the transpose below.  One lane owns one point and walks its observations in
//     ascending observation index: the order depends on the point's list alone.
//   * transpose (k_nt_count, the shared scan, k_bucket_fill, k_nt_rank): pt_row_ptr / obs_of / cam_of from pt_idx and
//     row_ptr.  An integer histogram, its scan (scan_kernels.hpp), the fill every bucket list uses (cell_kernels.hpp:
//     integer atomic cursors, arbitrary order), then each slot's final place by rank within its
//     point's list (observation indices are unique, so the rank is a permutation): the result is exactly the stable
//     argsort of pt_idx.  The rank step costs k^2 loads for a point of k observations (cached; k is tens here).
//   * robust losses: iteratively reweighted least squares.  An observation's weight w = rho'(s),
//     s = |r|^2, is recomputed from the r jacobian_obs returns and (r, Jc, Jp) are scaled by sqrt(w) before anything is
//     accumulated: no weight array, no extra memory traffic.  Every pass over the observations is one kernel template
//     with a trailing parameter pack `class... Loss`: empty, the instance is the squared-loss kernel, its arguments and
//     its code what they were before losses existed; <..., int, double> takes (kind, a2) last and makes that one call
//     (loss_scale_obs explains why a pack).
#pragma once
#include "kernels.hpp"

namespace c2b {

constexpr int kNormG = 16;                        // lanes per camera in k_normal_cameras
constexpr int kNormCamsPerWave = 64 / kNormG;
constexpr int kNormBlock = 256;
constexpr int kNormMaxGrid = 1024;                // x 4 wave partials <= the workspace's partial slots (block_part_slots)
constexpr int kNormSym = 45;                      // distinct entries of a symmetric 9x9
constexpr int kNormAcc = kNormSym + 9;            // + the gradient

// A camblk record read in place through the blocked table, shaped like a pointer for jacobian_obs (which indexes cam[j]
// and takes cam + kJl): every index is a constant after inlining, so the layout arithmetic folds away.
struct CamRef {
    const double *group;
    int k, off;
    __device__ __forceinline__ double operator[](int j) const { return group[cam_in_group_at(k, off + j)]; }
    __device__ __forceinline__ CamRef operator+(int d) const { return CamRef{group, k, off + d}; }
};
C2B_DEV CamRef cam_ref(const double *camblk, uint32_t c) { return CamRef{camblk + cam_group_at(c), (int)(c & 7u), 0}; }

// index of (a, b), a <= b, in the packed upper triangle of a 9x9: row a starts at 9a - a(a-1)/2
C2B_DEV int sym9(int a, int b) { return a * 9 - (a * (a - 1)) / 2 + (b - a); }

// ---- robust losses ---------------------------------------------------------------------------------------------
// kind: 0 squared, 1 Huber, 2 Cauchy, 3 soft-L1 (Ceres' definitions, scale a, a2 = a * a); s = |r|^2
enum { kLossSquared = 0, kLossHuber = 1, kLossCauchy = 2, kLossSoftL1 = 3 };

// w = rho'(s), in (0, 1]; s = 0 gives exactly 1 in every kind (Huber takes the s <= a2 branch: nothing divides by s)
C2B_DEV double loss_weight(int kind, double a2, double s) {
    if (kind == kLossHuber) return s <= a2 ? 1.0 : sqrt(a2 / s);
    const double q = 1.0 + s / a2;
    if (kind == kLossCauchy) return 1.0 / q;
    if (kind == kLossSoftL1) return 1.0 / sqrt(q);
    return 1.0;
}

// rho(s).  soft-L1 as 2 s / (sqrt(1 + s / a2) + 1), which is 2 a2 (sqrt(1 + s / a2) - 1) without its cancellation
C2B_DEV double loss_rho(int kind, double a2, double s) {
    if (kind == kLossHuber) return s <= a2 ? s : 2.0 * sqrt(a2 * s) - a2;
    if (kind == kLossCauchy) return a2 * log1p(s / a2);
    if (kind == kLossSoftL1) return 2.0 * s / (sqrt(1.0 + s / a2) + 1.0);
    return s;
}

// (r, Jc, Jp) *= sqrt(w): the one substitution every weighted pass makes, right after jacobian_obs, as
//     if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
// with (kind, a2) the kernel's own trailing pack `Loss... loss`.  The pack is the mechanism because it leaves the
// empty instance exactly the kernel it was, signature and body: the squared-loss kernels are pinned to the code they
// compiled to before losses existed.  The other way of sharing the text did not: as instances of a common C2B_DEV body
// with a LOSS flag, k_schur_cameras<kSchurApply> went from 110 to 128 VGPRs and k_normal_cameras from 252 to 248, and
// the rest kept their registers but not their code.  A run-time flag would put the weighting's code and registers into
// the squared-loss kernel itself.  tests/test_isa_pins.py holds both instances of every pass to their registers.
C2B_DEV void loss_scale_obs(int kind, double a2, double &r0, double &r1, double jc[18], double jp[6]) {
    const double sw = sqrt(loss_weight(kind, a2, r0 * r0 + r1 * r1));
    r0 *= sw; r1 *= sw;
#pragma unroll
    for (int k = 0; k < 18; ++k) jc[k] *= sw;
#pragma unroll
    for (int k = 0; k < 6; ++k) jp[k] *= sw;
}

// host side of the pack: launch(kind, a2) under a loss, launch() without, so a pass is launched from one place as
//     with_loss(kind, a2, [&](auto... loss) { hipLaunchKernelGGL((k_x<..., decltype(loss)...>), ..., loss...); });
template <class Launch>
inline void with_loss(int kind, double a2, Launch &&launch) {
    if (kind != kLossSquared) launch(kind, a2);
    else launch();
}

// ---- point-major transpose ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nt_count(const uint32_t *__restrict__ pt_idx, int64_t n_obs, int64_t n_pts,
                                                  uint32_t *__restrict__ cnt) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const uint32_t p = pt_idx[o];
    if (p < (uint64_t)n_pts) atomicAdd(cnt + p, 1u);
}

// slot j holds some observation o of point p (in fill order); its place in the stable order is b + #{k in [b, e): slots[k] < o}
__global__ __launch_bounds__(256) void k_nt_rank(const uint32_t *__restrict__ pt_idx, const uint64_t *__restrict__ pt_row_ptr,
                                                 int64_t n_pts, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ row_ptr,
                                                 int n_cam, uint32_t *__restrict__ obs_of, uint32_t *__restrict__ cam_of) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= (int64_t)pt_row_ptr[n_pts]) return;                     // slots filled (observations with p < n_pts)
    const uint32_t o = slots[j];
    const uint32_t p = pt_idx[o];
    const uint64_t b = pt_row_ptr[p], e = pt_row_ptr[p + 1];
    uint64_t rank = 0;
    for (uint64_t k = b; k < e; ++k) rank += slots[k] < o ? 1u : 0u;
    obs_of[b + rank] = o;
    cam_of[b + rank] = csr_search(row_ptr, n_cam, o);
}

// ---- camera pass ---------------------------------------------------------------------------------------------
// The weighted camera pass is k_normal_cameras<false, int, double>: it has no sum of squares.  With the fold of
// k_normal_cameras<true> it needs two scalar registers more than there are, so the weighted sum is k_robust_cost<true>'s.
template <bool WITH_SUM, class... Loss>
__global__ __launch_bounds__(kNormBlock) void k_normal_cameras(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint64_t *__restrict__ row_ptr, int n_cam,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, double *__restrict__ U, double *__restrict__ gc,
    double *__restrict__ block_part, Loss... loss) {
    static_assert(!(WITH_SUM && sizeof...(Loss) > 0), "the weighted camera pass has no scalar registers left for the sum's fold");
    constexpr int kWaves = kNormBlock / 64;
    __shared__ double sAcc[kWaves * kNormCamsPerWave * kNormAcc];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / kNormG, gl = lane % kNormG;
    double *mine = sAcc + (wave * kNormCamsPerWave + grp) * kNormAcc;
    const int n_quads = (n_cam + kNormCamsPerWave - 1) / kNormCamsPerWave;          // 32-bit: this kernel has no scalar
    const int wave_step = (int)gridDim.x * kWaves;                                  // registers to spare (n_cam < 2^31)
    double ssq = 0.0;                                                // lane gl == 0 of a group: its cameras' sums, in order
#pragma unroll 1
    for (int q = (int)blockIdx.x * kWaves + wave; q < n_quads; q += wave_step) {   // wave-uniform
        const int c = q * kNormCamsPerWave + grp;
        const bool cam_ok = c < n_cam;
        const uint64_t b = cam_ok ? row_ptr[c] : 0, e = cam_ok ? row_ptr[c + 1] : 0;
        const CamRef cam = cam_ref(camblk, cam_ok ? (uint32_t)c : 0u);
        double acc[kNormAcc], sq = 0.0;
#pragma unroll
        for (int k = 0; k < kNormAcc; ++k) acc[k] = 0.0;
#pragma unroll 1
        for (uint64_t o = b + gl; o < e; o += kNormG) {
            double r0, r1, jc[18], jp[6];
            jacobian_obs(cam, pts4[pt_idx[o]], uv_obs[o], r0, r1, jc, jp);
            if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
#pragma unroll
            for (int a = 0; a < 9; ++a) {
#pragma unroll
                for (int d = a; d < 9; ++d) acc[sym9(a, d)] += jc[a] * jc[d] + jc[9 + a] * jc[9 + d];
                acc[kNormSym + a] += jc[a] * r0 + jc[9 + a] * r1;
            }
            sq += r0 * r0 + r1 * r1;
        }
        // fixed tree over the group's 16 lanes (xor: every lane ends with the same bits)
#pragma unroll
        for (int off = kNormG / 2; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < kNormAcc; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
            sq += __shfl_xor(sq, off, 64);
        }
        if (gl == 0) {
#pragma unroll
            for (int k = 0; k < kNormAcc; ++k) mine[k] = acc[k];
            ssq += sq;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (cam_ok) {
            // both triangles from one packed entry: U[a][d] and U[d][a] are the same bits; 16 lanes write a row of 81 + 9
            double *Uc = U + (int64_t)c * 81;
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int i = gl + t * kNormG;
                if (i < 81) {
                    const int a = i / 9, d = i % 9;
                    Uc[i] = mine[a <= d ? sym9(a, d) : sym9(d, a)];
                }
            }
            if (gl < 9) gc[(int64_t)c * 9 + gl] = mine[kNormSym + gl];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (WITH_SUM) {                                                  // one partial per wave
        const double w = wave_sum(ssq);
        if (lane == 0) block_part[blockIdx.x * kWaves + wave] = w;
    }
}

// the wave partials of k_normal_cameras in a fixed order (one workgroup): thread t sums partials t, t + 256, ...
__global__ __launch_bounds__(256) void k_normal_sum(const double *__restrict__ block_part, int n, double *__restrict__ out_sum) {
    __shared__ double sRed[4];
    double a = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) a += block_part[k];
    const double w = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) out_sum[0] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// ---- point pass ------------------------------------------------------------------------------------------------
template <class... Loss>
__global__ __launch_bounds__(kNormBlock) void k_normal_points(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
    const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs,
    double *__restrict__ V, double *__restrict__ gp, Loss... loss) {
    const int64_t p = (int64_t)blockIdx.x * kNormBlock + threadIdx.x;
    if (p >= n_pts) return;
    const uint64_t b = pt_row_ptr[p], e = pt_row_ptr[p + 1];
    double v00 = 0.0, v01 = 0.0, v02 = 0.0, v11 = 0.0, v12 = 0.0, v22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (e > b) {
        const double4 X = pts4[p];
        for (uint64_t j = b; j < e; ++j) {
            const uint32_t o = obs_of[j];
            double r0, r1, jc[18], jp[6];
            jacobian_obs(cam_ref(camblk, cam_of[j]), X, uv_obs[o], r0, r1, jc, jp);
            if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);
            v00 += jp[0] * jp[0] + jp[3] * jp[3];
            v01 += jp[0] * jp[1] + jp[3] * jp[4];
            v02 += jp[0] * jp[2] + jp[3] * jp[5];
            v11 += jp[1] * jp[1] + jp[4] * jp[4];
            v12 += jp[1] * jp[2] + jp[4] * jp[5];
            v22 += jp[2] * jp[2] + jp[5] * jp[5];
            g0 += jp[0] * r0 + jp[3] * r1;
            g1 += jp[1] * r0 + jp[4] * r1;
            g2 += jp[2] * r0 + jp[5] * r1;
        }
    }
    double *Vp = V + p * 9;
    Vp[0] = v00; Vp[1] = v01; Vp[2] = v02;
    Vp[3] = v01; Vp[4] = v11; Vp[5] = v12;
    Vp[6] = v02; Vp[7] = v12; Vp[8] = v22;
    gp[3 * p] = g0; gp[3 * p + 1] = g1; gp[3 * p + 2] = g2;
}

// ---- robust cost -----------------------------------------------------------------------------------------------
// one projection per observation, one partial per workgroup (k_normal_sum adds them): sum rho(s), what a loop under a loss
// minimises; WEIGHTED_SQ: sum w s instead, the weighted sum of squares (the weighted k_normal_cameras with the fold of
// k_normal_cameras<true> needs two scalar registers more than there are, so under a loss the sum is this pass).
// cam_idx == NULL: the observation's camera is searched in row_ptr
template <bool WEIGHTED_SQ>
__global__ __launch_bounds__(kNormBlock) void k_robust_cost(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint32_t *__restrict__ cam_idx,
    const uint64_t *__restrict__ row_ptr, int n_cam, const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs,
    int64_t n_obs, int kind, double a2, double *__restrict__ part) {
    __shared__ double sRed[4];
    const int64_t o = (int64_t)blockIdx.x * kNormBlock + threadIdx.x;
    double v = 0.0;
    if (o < n_obs) {
        const double4 X = pts4[pt_idx[o]];
        const double2 ob = uv_obs[o];
        const uint32_t c = cam_idx ? cam_idx[o] : csr_search(row_ptr, n_cam, (uint32_t)o);
        const Proj pr = project_obs(cam_ref(camblk, c), X.x, X.y, X.z);
        double r0 = pr.u - ob.x, r1 = pr.v - ob.y;
        const double s = r0 * r0 + r1 * r1;
        if (WEIGHTED_SQ) {
            const double sw = sqrt(loss_weight(kind, a2, s));
            r0 *= sw; r1 *= sw;
            v = r0 * r0 + r1 * r1;
        } else {
            v = loss_rho(kind, a2, s);
        }
    }
    const double w = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

}  // namespace c2b
