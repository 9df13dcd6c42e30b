// refine_kernels.hpp -- gfx950 kernel of per-point Levenberg-Marquardt (included by capi.hip only, after triangulate_kernels.hpp).
//
// c2b_refine_points_rows / c2b_problem_refine_points: every point re-minimised by itself against the cameras as
// they stand, with its own damping and its own acceptance -- the point half of bundle adjustment, block diagonal over the
// points, without the Schur machinery and without one point's bad step rejecting every other point's good one.
//   * k_refine_points: point-major through the transpose, one lane per point walking its observations in ascending index,
//     the walk of k_normal_points, k_schur_points and k_triangulate_points.  A walk (refine_walk) evaluates at one position
//     the point's cost F = sum rho(|r|^2) + |w_X o (X - X0)|^2 (the point prior of DESIGN 4.13, added after the
//     observations) and its linearisation V = sum w Jp^T Jp + diag(w_X^2), g = sum w Jp^T r + w_X o r_X, with r and Jp from
//     jacobian_obs itself (inlined; the camera block it also forms is never read and falls to dead-code elimination) scaled
//     by sqrt(w), w = rho'(|r|^2) at that position, as every weighted pass scales them (loss_scale_obs): IRLS, DESIGN 4.3.
//   * a round solves (V + mu diag(d)) delta = -g by Chol3 (d = V's diagonal clamped to [1e-6, 1e32], `damped`), walks at
//     X + delta, and accepts by Nielsen's rule exactly as the LM loop words it: the gain ratio against
//     model = -(2 g.delta + delta^T V delta), accepted when it is > 0 and the cost fell to a finite value; then the trial's
//     sums become the state's (no re-walk).  A failed factorisation or a non-finite delta is a rejection.  mu stays in the
//     damping range.  Everything lives in registers: two sets of (F, V, g), X, delta, mu, nu, the prior's six doubles.
//   * the round loop's bound is uniform (max_rounds); a lane whose point met a tolerance, or has nothing to do, idles.
//   * one status byte per point and six counts (the five statuses and `moved`): LDS integer atomics per workgroup, then at
//     most six 64-bit integer atomics per workgroup into counts[6] (zeroed by the launcher), as k_triangulate_points.
// No float atomics, no scratch memory, no cross-lane traffic in the arithmetic: a point's result depends on its own list,
// its cameras and the options alone, so the same inputs give the same bits.
#pragma once
#include "triangulate_kernels.hpp"

namespace c2b {

constexpr int kRefBlock = 256;
// C2B_REFINE_* of include/city2ba_hip_experimental.h; the sixth count is the number of points written
enum { kRefConverged = 0, kRefMaxRounds = 1, kRefUnobserved = 2, kRefFailed = 3, kRefConstant = 4, kRefKinds = 5, kRefMoved = 5, kRefCounts = 6 };

// the options of a launch that the kernel reads: c2b_refine_options without its padding, and a disabled test's tolerance (0
// in the options) as NaN, against which every comparison is false -- the loop tests no "tolerance > 0" beside each tolerance
struct RefOptions {
    int max_rounds;
    double mu0, function_tol, gradient_tol, parameter_tol;
};

// a point's cost and linearisation at one position: V's upper triangle and g
struct RefSums { double F, v00, v01, v02, v11, v12, v22, g0, g1, g2; };

// the point prior a lane holds: weights (0 = off) and targets (0 where the weight is 0: the target is never read)
struct RefPrior { double w0, w1, w2, t0, t1, t2; };

C2B_DEV RefSums refine_walk(const double *__restrict__ camblk, const double x, const double y, const double z, const uint64_t b,
                            const uint64_t e, const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of,
                            const double2 *__restrict__ uv_obs, const int kind, const double a2, const RefPrior &pr) {
    RefSums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double4 X = make_double4(x, y, z, 0.0);
#pragma unroll 1
    for (uint64_t j = b; j < e; ++j) {
        double r0, r1, jc[18], jp[6];
        jacobian_obs(cam_ref(camblk, cam_of[j]), X, uv_obs[obs_of[j]], r0, r1, jc, jp);
        const double sq = r0 * r0 + r1 * r1;
        s.F += loss_rho(kind, a2, sq);
        if (kind != kLossSquared) {                          // (r, Jp) *= sqrt(w), loss_scale_obs without the camera block
            const double sw = sqrt(loss_weight(kind, a2, sq));
            r0 *= sw; r1 *= sw;
#pragma unroll
            for (int k = 0; k < 6; ++k) jp[k] *= sw;
        }
        s.v00 += jp[0] * jp[0] + jp[3] * jp[3];
        s.v01 += jp[0] * jp[1] + jp[3] * jp[4];
        s.v02 += jp[0] * jp[2] + jp[3] * jp[5];
        s.v11 += jp[1] * jp[1] + jp[4] * jp[4];
        s.v12 += jp[1] * jp[2] + jp[4] * jp[5];
        s.v22 += jp[2] * jp[2] + jp[5] * jp[5];
        s.g0 += jp[0] * r0 + jp[3] * r1;
        s.g1 += jp[1] * r0 + jp[4] * r1;
        s.g2 += jp[2] * r0 + jp[5] * r1;
    }
    // the prior's rows, k_prior_points' expressions: r = w (x - x0), V += w^2, g += w r, cost (r0^2 + r1^2) + r2^2.  A weight of 0
    // holds the target 0, so its row is 0 (x - 0) = 0 at every finite position without a select per walk
    const double q0 = pr.w0 * (x - pr.t0), q1 = pr.w1 * (y - pr.t1), q2 = pr.w2 * (z - pr.t2);
    s.v00 += pr.w0 * pr.w0; s.v11 += pr.w1 * pr.w1; s.v22 += pr.w2 * pr.w2;
    s.g0 += pr.w0 * q0; s.g1 += pr.w1 * q1; s.g2 += pr.w2 * q2;
    s.F += (q0 * q0 + q1 * q1) + q2 * q2;
    return s;
}

// A per-launch scalar moved into vector registers (the compiler no longer knows that every lane holds the same one).  The walk
// inherits k_normal_points' scalar registers (the constants of pow and of the losses) and the round loop adds its own masks:
// what the loop only compares against lives in vector registers, of which this kernel has some to spare, so that no scalar
// is spilled.
C2B_DEV double refine_in_vgprs(double v) {
    asm volatile("" : "+v"(v));
    return v;
}
// ... and a kernel argument's pointer (rematch_kernels.hpp has the same move): through an integer and back as a pointer into
// global memory, so its loads and stores stay global_*
template <typename T>
C2B_DEV T *refine_in_vgprs(T *p) {
    unsigned long long u = reinterpret_cast<unsigned long long>(p);
    asm volatile("" : "+v"(u));
    return (T *)reinterpret_cast<__attribute__((address_space(1))) T *>(u);
}

// pt_mask, x0 / xw (the point priors, in pairs) may be NULL.  counts[kRefCounts] must be zero when the kernel starts.
__global__ __launch_bounds__(kRefBlock) void k_refine_points(
    const double *__restrict__ camblk, double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
    const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs, int kind, double a2,
    const double *__restrict__ x0, const double *__restrict__ xw, const RefOptions opt, const uint8_t *__restrict__ pt_mask,
    uint8_t *__restrict__ status, unsigned long long *__restrict__ counts) {
    constexpr int kRunning = kRefCounts;                     // the status of a point still in the round loop (never written)
    __shared__ unsigned sCnt[kRefCounts];
    if (threadIdx.x < kRefCounts) sCnt[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
    // what the tail needs, per lane, formed before the loop (the arguments' scalar registers are free in the loop)
    double4 *const my_pt = refine_in_vgprs(pts4) + p;
    uint8_t *const my_status = refine_in_vgprs(status) + p;
    unsigned long long *const my_count = refine_in_vgprs(counts) + threadIdx.x;
    const double function_tol = refine_in_vgprs(opt.function_tol), gradient_tol = refine_in_vgprs(opt.gradient_tol),
                 parameter_tol = refine_in_vgprs(opt.parameter_tol);
    // ... and what the walk reads through: its addresses are per lane anyway
    const double *const cams = refine_in_vgprs(camblk);
    const uint32_t *const row_obs = refine_in_vgprs(obs_of), *const row_cam = refine_in_vgprs(cam_of);
    const double2 *const uv = refine_in_vgprs(uv_obs);
    const double loss_a2 = refine_in_vgprs(a2);
    // a lane without a point to refine runs the uniform loop idle and touches no memory; past the last point: no status at all
    int st = p < n_pts ? kRefConstant : -1;
    uint64_t b = 0, e = 0;
    RefPrior pr{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double x = 0.0, y = 0.0, z = 0.0;
    if (st >= 0 && (!pt_mask || !pt_mask[p])) {
        b = pt_row_ptr[p]; e = pt_row_ptr[p + 1];
        if (xw) {
            pr.w0 = xw[3 * p]; pr.w1 = xw[3 * p + 1]; pr.w2 = xw[3 * p + 2];
            if (pr.w0 != 0.0) pr.t0 = x0[3 * p];
            if (pr.w1 != 0.0) pr.t1 = x0[3 * p + 1];
            if (pr.w2 != 0.0) pr.t2 = x0[3 * p + 2];
        }
        st = kRefUnobserved;
        if (e > b || pr.w0 != 0.0 || pr.w1 != 0.0 || pr.w2 != 0.0) {
            const double4 X = *my_pt;
            x = X.x; y = X.y; z = X.z;
            st = kRunning;
        }
    }
    // One copy of the walk: pass 0 walks at the start, pass k > 0 is round k - 1's walk at its trial position (tx, ty, tz),
    // whose step and model decrease the pass before it prepared.  Only the trial position and the model cross a walk, not
    // delta.  `stepped` false: the round's factorisation failed, there is nothing to walk at, and the round is a rejection.
    // An accepted step lowers the cost strictly, so `moved` is "the point's cost fell".
    RefSums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double tx = x, ty = y, tz = z, model = 0.0, mu = opt.mu0, nu = 2.0;
    bool stepped = true, moved = false;
#pragma unroll 1
    for (int pass = 0; pass <= opt.max_rounds; ++pass) {
        if (st == kRunning) {
            bool accepted = false;
            if (stepped) {
                const RefSums t = refine_walk(cams, tx, ty, tz, b, e, row_obs, row_cam, uv, kind, loss_a2, pr);
                if (pass == 0) {
                    accepted = isfinite(t.F);
                    if (!accepted) st = kRefFailed;
                } else {
                    const double rho = model > 0.0 ? (s.F - t.F) / model : -1.0;
                    accepted = rho > 0.0 && t.F < s.F && isfinite(t.F);
                    if (accepted) {
                        const double c = 2.0 * rho - 1.0;
                        mu = fmin(fmax(mu * fmax(1.0 / 3.0, 1.0 - (c * c) * c), C2B_STEP_LAMBDA_MIN), C2B_STEP_LAMBDA_MAX);
                        nu = 2.0;
                        moved = true;
                        if (s.F - t.F <= function_tol * s.F) st = kRefConverged;
                    }
                }
                if (accepted) {
                    x = tx; y = ty; z = tz;
                    s = t;
                }
            }
            if (!accepted) {
                mu = fmin(fmax(mu * nu, C2B_STEP_LAMBDA_MIN), C2B_STEP_LAMBDA_MAX);
                nu *= 2.0;
            }
            // round `pass`: the gradient test at the state the step is solved at, the step, the parameter test (the step is not applied)
            if (st == kRunning && pass < opt.max_rounds) {
                if (fmax(fmax(fabs(s.g0), fabs(s.g1)), fabs(s.g2)) <= gradient_tol) {
                    st = kRefConverged;
                } else {
                    const Chol3 L = chol3_factor(damped(s.v00, mu), s.v01, s.v02, damped(s.v11, mu), s.v12, damped(s.v22, mu));
                    double d0, d1, d2;
                    L.solve(-s.g0, -s.g1, -s.g2, d0, d1, d2);
                    stepped = L.positive() && isfinite(d0) && isfinite(d1) && isfinite(d2);
                    if (stepped) {
                        const double dn = sqrt((d0 * d0 + d1 * d1) + d2 * d2), xn = sqrt((x * x + y * y) + z * z);
                        if (dn <= parameter_tol * (xn + parameter_tol)) st = kRefConverged;
                        const double Vd0 = (s.v00 * d0 + s.v01 * d1) + s.v02 * d2;
                        const double Vd1 = (s.v01 * d0 + s.v11 * d1) + s.v12 * d2;
                        const double Vd2 = (s.v02 * d0 + s.v12 * d1) + s.v22 * d2;
                        const double gd = (s.g0 * d0 + s.g1 * d1) + s.g2 * d2;
                        const double dVd = (d0 * Vd0 + d1 * Vd1) + d2 * Vd2;
                        model = -(2.0 * gd + dVd);
                        tx = x + d0; ty = y + d1; tz = z + d2;
                    }
                }
            }
        }
    }
    if (st == kRunning) st = kRefMaxRounds;
    if (st >= 0) {
        if (moved) {
            double2 *out = reinterpret_cast<double2 *>(my_pt);               // x y | z w: the fourth lane keeps its value
            out[0] = make_double2(x, y);
            reinterpret_cast<double *>(out + 1)[0] = z;
            atomicAdd(&sCnt[kRefMoved], 1u);
        }
        *my_status = (uint8_t)st;
        atomicAdd(&sCnt[st], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kRefCounts && sCnt[threadIdx.x]) atomicAdd(my_count, (unsigned long long)sCnt[threadIdx.x]);
}

}  // namespace c2b
