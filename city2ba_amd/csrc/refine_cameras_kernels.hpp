// refine_cameras_kernels.hpp -- gfx950 kernel of per-camera Levenberg-Marquardt (included by capi.hip only, after
// prior_kernels.hpp and refine_kernels.hpp).
//
// c2b_refine_cameras_rows / c2b_problem_refine_cameras: every camera re-minimised by itself against the points
// as they stand, with its own damping and its own acceptance -- the dual of k_refine_points (refine_kernels.hpp), whose
// rule set it follows with 9 for 3: motion-only bundle adjustment, block diagonal over the cameras.
//   * the parameters are q = bal9[c][0..8] (to_vec order).  For every walk the camera's record is formed from q by
//     from_rodrigues and fill_camblk, the arithmetic of k_cameras_prepare<true>, into LDS by the group's first lane
//     (refine_camera_record); jacobian_obs reads it through an LDS-typed pointer.  A step is q + delta on the free entries, what c2b_problem_apply_step does to bal9.
//   * a walk is k_normal_cameras' own: kNormG = 16 lanes own a camera, lane l sums observations b + l, b + l + 16, ... of
//     the row (45 + 9 products and rho), then the fixed xor tree: every lane of the group ends with the same bits.  Then the
//     centre prior's A^T A and A^T r (prior_center_rows, k_prior_cameras' expressions), then the intrinsics prior's, then
//     the zeros of the constant entries: at walk 0 (U, g) are the bits of c2b_problem_normal_equations.
//   * everything after the tree is computed by all 16 lanes of the group alike (the same instructions on the same bits: what
//     one lane would cost, and no lane waits for another): the decision, the 9x9 factor and solve (chol9_packed and
//     chol9_solve, the Schur passes' routine), the model decrease, the trial parameters.  What crosses a walk -- the
//     accepted (F, U, g), q, the trial q, mu, nu, the model decrease -- is parked in the camera's LDS slot by lane 0 of the
//     group, so that a walk holds its 55 accumulators in registers and little else.  One template per loss pack, as every
//     pass over the observations (normal_kernels.hpp): the empty instance carries no code of the losses.
//   * the round loop's bound is uniform (max_rounds); a group whose camera met a tolerance, or has nothing to do, idles, and a
//     wave none of whose four cameras is running leaves the loop.  A group never synchronises with another: wave barriers only.
//   * one status byte per camera and six counts: LDS integer atomics, then at most six 64-bit integer atomics per workgroup.
// No float atomics and no scratch memory: a camera's result depends on its own row, its points and the options alone.
// The register margin is thin: 241 (squared loss) and 255 (weighted) of the 256 vector registers two waves per SIMD leave, held
// there by amdgpu_waves_per_eu(2).  After a toolchain update run tools/isa_report.py --filter k_refine_cameras (and
// tests/test_isa_pins.py, which refuses scratch and spills in every kernel) before anything else: a compiler that needs one
// register more spills instead of failing.
#pragma once
#include "prior_kernels.hpp"
#include "refine_kernels.hpp"

namespace c2b {

constexpr int kRcBlock = 256;
constexpr int kRcCams = kRcBlock / kNormG;        // cameras per workgroup
// a camera's LDS slot, in doubles: the trial record | the accepted U (packed upper triangle) and g | the accepted q | the
// trial q | F, mu, nu, model.  An odd stride spreads the groups' slots over the banks.
constexpr int kRcRec = 0, kRcSums = kCamBlk, kRcQ = kRcSums + kNormAcc, kRcTrial = kRcQ + 9, kRcF = kRcTrial + 9, kRcMu = kRcF + 1,
              kRcNu = kRcMu + 1, kRcModel = kRcNu + 1, kRcSlot = kRcModel + 2;
static_assert(kRcSlot % 2 == 1, "odd slot stride");

// what lane 0 of a group wrote to the slot is visible to the group's other lanes after this (one wave: no workgroup barrier)
C2B_DEV void refine_group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A camera's record from its nine parameters, LDS to LDS: k_cameras_prepare<true>'s arithmetic.  A call, not inlined: inlined
// into the round loop, the constants of its sines, cosines and series are hoisted out of the loop and stay live across the walk,
// which has no register for them.
__device__ __attribute__((noinline)) void refine_camera_record(const double *q9, double *rec) {
    double q[9], cam15[15];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = q9[k];
    from_rodrigues(q[0], q[1], q[2], cam15);
#pragma unroll
    for (int k = 0; k < 6; ++k) cam15[9 + k] = q[3 + k];
    fill_camblk(cam15, q[0], q[1], q[2], rec);
}

// The launch's arguments that the round loop reads between walks only, parked in LDS: the walk inherits k_normal_cameras'
// scalar registers (the constants of pow and of the losses) and has neither scalar nor vector registers to spare, so what a
// walk does not read is fetched (into vector registers, for as long as it is needed) where it is.
struct RcArgs {
    double *bal9;
    const double *c0, *cw, *i0, *iw;
    uint8_t *status;
    unsigned long long *counts;
    double function_tol, gradient_tol, parameter_tol, mu_min, mu_max, third;       // (the update's three constants with them)
};

// c0 / cw, i0 / iw (the camera priors, in pairs), cam_mask and status may be NULL.  counts[kRefCounts] must be zero when the
// kernel starts.
template <class... Loss>
__global__ __launch_bounds__(kRcBlock) __attribute__((amdgpu_waves_per_eu(2))) void k_refine_cameras(
    double *__restrict__ bal9, const double4 *__restrict__ pts4, int n_cam, const uint64_t *__restrict__ row_ptr,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, const double *__restrict__ c0,
    const double *__restrict__ cw, const double *__restrict__ i0, const double *__restrict__ iw, const RefOptions opt,
    const uint16_t *__restrict__ cam_mask, uint8_t *__restrict__ status, unsigned long long *__restrict__ counts, Loss... loss) {
    constexpr int kRunning = kRefCounts;                     // the status of a camera still in the round loop (never written)
    constexpr unsigned kAll = 0x1ffu;
    __shared__ double sSlot[kRcCams * kRcSlot];
    __shared__ unsigned sCnt[kRefCounts];
    __shared__ RcArgs sArgs;
    // a camera's row [b, e) and the offset of its priors' rows (3 c), read where they are used, not held across a walk
    __shared__ uint64_t sRow[kRcCams][3];
    if (threadIdx.x < kRefCounts) sCnt[threadIdx.x] = 0u;
    if (threadIdx.x == 0)
        sArgs = RcArgs{bal9, c0, cw, i0, iw, status, counts, opt.function_tol, opt.gradient_tol, opt.parameter_tol, C2B_STEP_LAMBDA_MIN,
                       C2B_STEP_LAMBDA_MAX, 1.0 / 3.0};
    __syncthreads();
    const int gl = threadIdx.x % kNormG;
    const int grp = (int)threadIdx.x / kNormG;
    const int c = (int)blockIdx.x * kRcCams + grp;
    double *const slot = sSlot + grp * kRcSlot;
    const lds_cptr rec = (lds_cptr)(slot + kRcRec);
    // a group without a camera to refine runs the uniform loop idle and touches no memory; past the last camera: no status
    int st = c < n_cam ? kRefConstant : -1;
    // the group's bits, one register: the camera's mask (bits 0..8), has a centre prior / an intrinsics prior, and the loop's two
    // flags.  `stepped` false: the round's factorisation failed, there is nothing to walk at, and the round is a rejection.  An
    // accepted step lowers the cost strictly, so `moved` is "the cost fell".
    constexpr unsigned kPriC = 1u << 9, kPriI = 1u << 10, kStepped = 1u << 11, kMoved = 1u << 12;
    unsigned bits = kStepped;
    if (st >= 0) {
        bits |= cam_mask ? cam_mask[c] & kAll : 0u;
        if ((bits & kAll) != kAll) {
            double w[3];
            bool pri_c, pri_i;
            const uint64_t b = row_ptr[c], e = row_ptr[c + 1];
            prior_weights(cw, c, w, pri_c);
            prior_weights(iw, c, w, pri_i);
            bits |= (pri_c ? kPriC : 0u) | (pri_i ? kPriI : 0u);
            st = (e > b || pri_c || pri_i) ? kRunning : kRefUnobserved;
            if (gl == 0) { sRow[grp][0] = b; sRow[grp][1] = e; sRow[grp][2] = (uint64_t)c * 3; }
        }
    }
    if (st == kRunning) {
        if (gl < 9) {
            const double v = bal9[(int64_t)c * 9 + gl];
            slot[kRcQ + gl] = v;
            slot[kRcTrial + gl] = v;
        }
        if (gl == 0) { slot[kRcF] = 0.0; slot[kRcMu] = opt.mu0; slot[kRcNu] = 2.0; slot[kRcModel] = 0.0; }
    }
    // One copy of the walk: pass 0 walks at the start, pass k > 0 is round k - 1's walk at its trial parameters, whose step
    // and model decrease the pass before it prepared.
#pragma unroll 1
    for (int pass = 0; pass <= opt.max_rounds; ++pass) {
        if (__builtin_amdgcn_ballot_w64(st == kRunning) == 0) break;            // wave-uniform
        refine_group_sync();
        const bool walk = st == kRunning && (bits & kStepped);
        if (walk && gl == 0) refine_camera_record(slot + kRcTrial, slot + kRcRec);       // the trial record, by the group's first lane
        refine_group_sync();
        double acc[kNormAcc], F = 0.0;
#pragma unroll
        for (int k = 0; k < kNormAcc; ++k) acc[k] = 0.0;
        const uint64_t we = walk ? sRow[grp][1] : 0;
#pragma unroll 1
        for (uint64_t o = (walk ? sRow[grp][0] : 0) + gl; o < we; o += kNormG) {
            double r0, r1, jc[18], jp[6];
            jacobian_obs(rec, pts4[pt_idx[o]], uv_obs[o], r0, r1, jc, jp);
            [[maybe_unused]] double sq;                      // |r|^2 before the weighting
            if constexpr (sizeof...(Loss) > 0) {
                sq = r0 * r0 + r1 * r1;
                loss_scale_obs(loss..., r0, r1, jc, jp);
            }
#pragma unroll
            for (int a = 0; a < 9; ++a) {
#pragma unroll
                for (int d = a; d < 9; ++d) acc[sym9(a, d)] += jc[a] * jc[d] + jc[9 + a] * jc[9 + d];
                acc[kNormSym + a] += jc[a] * r0 + jc[9 + a] * r1;
            }
            if constexpr (sizeof...(Loss) > 0) F += loss_rho(loss..., sq);      // (after the products: the Jacobian's registers are free again)
            else F += r0 * r0 + r1 * r1;
        }
        // k_normal_cameras' tree over the group's 16 lanes (xor: every lane ends with the same bits)
#pragma unroll
        for (int off = kNormG / 2; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < kNormAcc; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
            F += __shfl_xor(F, off, 64);
        }
        if (st == kRunning) {
            if (walk) {
                if (bits & kPriC) {                                 // the centre prior: k_prior_cameras' rows 0..5
                    double w[3], r[3], A[18];
                    bool any;
                    const uint64_t c3 = sRow[grp][2];
                    prior_weights(refine_in_vgprs(sArgs.cw) + c3, 0, w, any);
                    prior_center_rows(rec, refine_in_vgprs(sArgs.c0) + c3, w, r, A);
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
#pragma unroll
                        for (int d = a; d < 6; ++d) acc[sym9(a, d)] += (A[a] * A[d] + A[6 + a] * A[6 + d]) + A[12 + a] * A[12 + d];
                        acc[kNormSym + a] += (A[a] * r[0] + A[6 + a] * r[1]) + A[12 + a] * r[2];
                    }
                    F += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                }
                if (bits & kPriI) {                                 // the intrinsics prior: its rows 6..8
                    double ri[3] = {0.0, 0.0, 0.0};
                    const uint64_t c3 = sRow[grp][2];
                    const double *const wi = refine_in_vgprs(sArgs.iw) + c3, *const ti = refine_in_vgprs(sArgs.i0) + c3;
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        const double w = wi[m];
                        if (w != 0.0) {
                            ri[m] = w * (rec[kIntr + m] - ti[m]);
                            acc[sym9(6 + m, 6 + m)] += w * w;
                            acc[kNormSym + 6 + m] += w * ri[m];
                        }
                    }
                    F += (ri[0] * ri[0] + ri[1] * ri[1]) + ri[2] * ri[2];
                }
                if (const unsigned mask = bits & kAll) {     // the zeros of J~; F is not masked
#pragma unroll
                    for (int a = 0; a < 9; ++a) {
#pragma unroll
                        for (int d = a; d < 9; ++d)
                            if (((mask >> a) | (mask >> d)) & 1u) acc[sym9(a, d)] = 0.0;
                        if ((mask >> a) & 1u) acc[kNormSym + a] = 0.0;
                    }
                }
            }
            double mu = slot[kRcMu], nu = slot[kRcNu];
            bool accepted = false;
            if (walk) {
                if (pass == 0) {
                    accepted = isfinite(F);
                    if (!accepted) st = kRefFailed;
                } else {
                    const double Fc = slot[kRcF], model = slot[kRcModel];
                    const double rho = model > 0.0 ? (Fc - F) / model : -1.0;
                    accepted = rho > 0.0 && F < Fc && isfinite(F);
                    if (accepted) {
                        const double t = 2.0 * rho - 1.0;
                        mu = fmin(fmax(mu * fmax(sArgs.third, 1.0 - (t * t) * t), sArgs.mu_min), sArgs.mu_max);
                        nu = 2.0;
                        bits |= kMoved;
                        if (Fc - F <= sArgs.function_tol * Fc) st = kRefConverged;
                    }
                }
            }
            refine_group_sync();                             // every lane has read the slot's F, mu, nu and model
            if (accepted) {
                if (gl == 0) {
#pragma unroll
                    for (int k = 0; k < kNormAcc; ++k) slot[kRcSums + k] = acc[k];
                    slot[kRcF] = F;
#pragma unroll
                    for (int k = 0; k < 9; ++k) slot[kRcQ + k] = slot[kRcTrial + k];
                }
            } else {
                mu = fmin(fmax(mu * nu, sArgs.mu_min), sArgs.mu_max);
                nu *= 2.0;
            }
            refine_group_sync();
            // round `pass`: the gradient test at the state the step is solved at, the step, the parameter test (the step is not applied)
            double model = 0.0;
            if (st == kRunning && pass < opt.max_rounds) {
                double g[9], gmax = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    g[k] = slot[kRcSums + kNormSym + k];
                    gmax = fmax(gmax, fabs(g[k]));
                }
                if (gmax <= sArgs.gradient_tol) {
                    st = kRefConverged;
                } else {
                    double a[kCholPacked], rhs[9], d[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) {
#pragma unroll
                        for (int j = 0; j <= i; ++j) a[tri9(i, j)] = i == j ? damped(slot[kRcSums + sym9(i, i)], mu) : slot[kRcSums + sym9(j, i)];
                        rhs[i] = -g[i];
                    }
                    const bool ok = chol9_packed(a);
                    chol9_solve(a, rhs, d);
                    bool stepped = ok;
#pragma unroll
                    for (int k = 0; k < 9; ++k) stepped = stepped && isfinite(d[k]);
                    bits = stepped ? bits | kStepped : bits & ~kStepped;
                    if (stepped) {
                        double q[9], dd = 0.0, qq = 0.0, gd = 0.0, dUd = 0.0;
#pragma unroll
                        for (int k = 0; k < 9; ++k) {
                            q[k] = slot[kRcQ + k];
                            dd += d[k] * d[k];
                            qq += q[k] * q[k];
                            gd += g[k] * d[k];
                        }
                        const double parameter_tol = sArgs.parameter_tol;
                        if (sqrt(dd) <= parameter_tol * (sqrt(qq) + parameter_tol)) st = kRefConverged;
#pragma unroll
                        for (int i = 0; i < 9; ++i) {
                            double Ud = 0.0;
#pragma unroll
                            for (int j = 0; j < 9; ++j) Ud += slot[kRcSums + (i <= j ? sym9(i, j) : sym9(j, i))] * d[j];
                            dUd += d[i] * Ud;
                        }
                        model = -(2.0 * gd + dUd);
                        if (gl == 0) {                       // a constant entry keeps its bits
#pragma unroll
                            for (int k = 0; k < 9; ++k) slot[kRcTrial + k] = (bits >> k) & 1u ? q[k] : q[k] + d[k];
                        }
                    }
                }
            }
            if (gl == 0) { slot[kRcMu] = mu; slot[kRcNu] = nu; slot[kRcModel] = model; }
        }
    }
    refine_group_sync();
    // the tail forms what it needs of the thread's index again (behind the asm the compiler holds none of it across the loop)
    unsigned tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const unsigned tl = tid % kNormG;
    const int64_t tc = (int64_t)blockIdx.x * kRcCams + tid / kNormG;
    if (st == kRunning) st = kRefMaxRounds;
    if (st >= 0) {
        if ((bits & kMoved) && tl < 9 && !((bits >> tl) & 1u)) refine_in_vgprs(sArgs.bal9)[tc * 9 + tl] = sSlot[(tid / kNormG) * kRcSlot + kRcQ + tl];
        if (tl == 0) {
            uint8_t *const out = refine_in_vgprs(sArgs.status);
            if (bits & kMoved) atomicAdd(&sCnt[kRefMoved], 1u);
            if (out) out[tc] = (uint8_t)st;
            atomicAdd(&sCnt[st], 1u);
        }
    }
    __syncthreads();
    if (tid < kRefCounts && sCnt[tid]) atomicAdd(refine_in_vgprs(sArgs.counts) + tid, (unsigned long long)sCnt[tid]);
}

}  // namespace c2b
