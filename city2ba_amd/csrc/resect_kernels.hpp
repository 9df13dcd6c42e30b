// resect_kernels.hpp -- gfx950 kernel of camera resection (included by capi.hip only, after triangulate_kernels.hpp).
//
// c2b_resect_rows / c2b_problem_resect_cameras: a camera's pose from its points and observations alone, the
// dual of triangulate_kernels.hpp; f, k1 and k2 stay as they are.
//   * k_resect_cameras: camera-major, one wave per camera walking its row in ascending order, 64 observations at a time.
//     Per usable observation the unit ray b of the observed pixel in the camera frame (tri_ray<false>: (pn.x, pn.y, -1)
//     normalised) and P = I - b b^T.  Walk 1: the centroid of the usable points.  Walk 2: the lanes stage the ten monomials
//     1, Y_a, Y_a Y_c of Y = X - centroid and the six entries of P of their observation in wave-private LDS; lane l < 60
//     then owns the sum of monomial l / 6 times entry l % 6 and adds the chunk's 64 terms in row order (one FMA and two
//     LDS reads per term: the lanes that share an address are served by one broadcast, the sixteen distinct addresses lie
//     on distinct banks).  No cross-lane reduction exists, so the order of every sum is the row's own.
//   * everything else is made from those 60 numbers in LDS: S0's 3x3 Cholesky and inverse, the 9x9 M of r^T M r with the
//     translation eliminated, its eigenpairs by cyclic Jacobi in rounds of four disjoint rotations (lane k < 9 owns row k, then
//     column k, of the working copy), the nearest rotation to the eigenvector of lambda_1 by Newton's polar iteration, Gauss-Newton on
//     SO(3) from M alone (lane k < 9 forms row k of M [r J]; the 3x3 solve is redundant in every lane), t.  Walk 3 is the
//     cheirality test.  The 3x3 and 9-vector values are wave-uniform and live in registers with compile-time indices; what
//     is indexed at run time (M, its copy, the eigenvectors, S1) lives in LDS: no scratch memory.
//   * the five status counts: LDS integer atomics per workgroup, then at most five 64-bit integer atomics per workgroup
//     into counts[5] (zeroed by the launcher).
// No float atomics, no robust loss; a camera's result depends on its own row alone, so the same inputs give the same bits.
#pragma once
#include "triangulate_kernels.hpp"

namespace c2b {

constexpr int kResBlock = 256;
constexpr int kResWaves = kResBlock / 64;                    // cameras per workgroup
// C2B_RES_* of include/city2ba_hip_experimental.h
enum { kResOk = 0, kResTooFew = 1, kResDegenerate = 2, kResBehind = 3, kResConstant = 4, kResKinds = 5 };
constexpr int kResMinPoints = 6;                             // the smallest min_points the entries accept
constexpr int kResFields = 16;                               // staged per observation: 10 monomials, 6 entries of P
// doubles between two staged fields: field f of observation k at f * kResPitch + k.  Lane l reads fields l / 6 and
// 10 + l % 6 of one k: the bank of a field is (4 f + 2 k) % 64, sixteen fields on sixteen bank pairs; the writes (one
// field, 64 consecutive k) are consecutive.
constexpr int kResPitch = 66;
constexpr int kResSweeps = 30, kResPolarIters = 40, kResGnIters = 8;

struct ResLds {                                              // one wave's
    double stage[kResFields * kResPitch];                    // after the second walk its head holds M, A and V (below)
    double S0[9], Si[9], S1[27];                             // sum P, its inverse, sum Y_a P (a-major), all as full 3x3
    double T[36];                                            // M r, M J_0, M J_1, M J_2 (and the centroid, the row norms)
};

// what a lane wrote to the wave's LDS is visible to the wave's other lanes
C2B_DEV void res_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// f, k1, k2 of a bal9 row, indexed as tri_ray indexes a camblk record (12, 13, 14)
struct ResIntrinsics {
    double f, k1, k2;
    __device__ __forceinline__ double operator[](int j) const { return j == 12 ? f : (j == 13 ? k1 : k2); }
};

// observation j of the row: the camera-frame ray and the point; false when unusable (tri_ray, or a point that is not finite)
C2B_DEV bool res_observation(const ResIntrinsics in, const double4 *__restrict__ pts4, const uint32_t *__restrict__ pt_idx,
                             const double2 *__restrict__ uv_obs, uint64_t j, double &bx, double &by, double &bz, double &x, double &y, double &z) {
    if (!tri_ray<false>(in, uv_obs[j], bx, by, bz)) return false;
    const double2 *X = reinterpret_cast<const double2 *>(pts4 + pt_idx[j]);
    const double2 xy = X[0];
    x = xy.x; y = xy.y; z = reinterpret_cast<const double *>(X + 1)[0];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    return true;
}

// (i, j), i <= j, of the k-th entry of a symmetric 3x3 in the order 00 01 02 11 12 22
C2B_DEV void res_sym(int k, int &i, int &j) {
    i = k < 3 ? 0 : (k < 5 ? 1 : 2);
    j = k < 3 ? k : (k < 5 ? k - 2 : 2);
}

// det of a column-major 3x3
C2B_DEV double res_det(const double *m) {
    return (m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2])) + m[6] * (m[1] * m[5] - m[4] * m[2]);
}

// o[k] = J_k . w for the 9-vector w, J_k = vec([e_k]x R): the sum over R's columns v of (e_k x v) . w
C2B_DEV void res_jt(const double *R, const double *w, double o[3]) {
    o[0] = o[1] = o[2] = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double x = R[3 * a], y = R[3 * a + 1], z = R[3 * a + 2];
        const double wx = w[3 * a], wy = w[3 * a + 1], wz = w[3 * a + 2];
        o[0] += y * wz - z * wy;                                 // e_0 x v = (0, -z, y)
        o[1] += z * wx - x * wz;                                 // e_1 x v = (z, 0, -x)
        o[2] += x * wy - y * wx;                                 // e_2 x v = (-y, x, 0)
    }
}

// resect_camera's keep predicate of k_resect_cameras: every usable observation counts
struct ResKeepAll {
    __device__ __forceinline__ bool operator()(uint64_t, double, double, double) const { return true; }
};

// The pose of one camera by the wave that calls it (every lane returns the same status; R column-major and t are written
// by lane 0 when it is kResOk).  cam = the camera's bal9 row, [b, e) its row of the observation list.  keep(j, x, y, z) is
// asked about every usable observation j (of the point x y z) in each of the three walks: what it refuses is not in the list
// as far as this routine goes (resect_robust_kernels.hpp restricts the fit to a pose's inliers that way).
template <typename Keep>
C2B_DEV int resect_camera(ResLds &W, const int lane, double *__restrict__ cam, const double4 *__restrict__ pts4, const uint64_t b,
                          const uint64_t e, const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, const int min_points,
                          const double min_gap, const Keep keep) {
    const ResIntrinsics in = {cam[6], cam[7], cam[8]};
    // ---- walk 1: the centroid of the usable points (lanes 0..2 own a component each and add in row order) ----
    double acc = 0.0;
    int n_used = 0;
#pragma unroll 1
    for (uint64_t j0 = b; j0 < e; j0 += 64) {
        const uint64_t j = j0 + lane;
        double bx, by, bz, x = 0.0, y = 0.0, z = 0.0;
        const bool use = j < e && res_observation(in, pts4, pt_idx, uv_obs, j, bx, by, bz, x, y, z) && keep(j, x, y, z);
        W.stage[lane] = use ? x : 0.0;
        W.stage[kResPitch + lane] = use ? y : 0.0;
        W.stage[2 * kResPitch + lane] = use ? z : 0.0;
        n_used += __popcll(__ballot(use));
        res_sync();
        if (lane < 3) {
            const double *s = W.stage + lane * kResPitch;
#pragma unroll 8
            for (int k = 0; k < 64; ++k) acc += s[k];
        }
        res_sync();
    }
    if (n_used < min_points) return kResTooFew;
    if (lane < 3) W.T[lane] = acc / (double)n_used;
    res_sync();
    const double cx = W.T[0], cy = W.T[1], cz = W.T[2];
    res_sync();
    // ---- walk 2: the sixty sums ----
    const int mono = lane < 60 ? lane / 6 : 0, ent = lane % 6;
    double sum = 0.0;
#pragma unroll 1
    for (uint64_t j0 = b; j0 < e; j0 += 64) {
        const uint64_t j = j0 + lane;
        double bx = 0.0, by = 0.0, bz = 0.0, x = 0.0, y = 0.0, z = 0.0;
        const bool use = j < e && res_observation(in, pts4, pt_idx, uv_obs, j, bx, by, bz, x, y, z) && keep(j, x, y, z);
        const double y0 = x - cx, y1 = y - cy, y2 = z - cz;
        double *s = W.stage + lane;
        s[0] = use ? 1.0 : 0.0;
        s[1 * kResPitch] = use ? y0 : 0.0;       s[2 * kResPitch] = use ? y1 : 0.0;       s[3 * kResPitch] = use ? y2 : 0.0;
        s[4 * kResPitch] = use ? y0 * y0 : 0.0;  s[5 * kResPitch] = use ? y0 * y1 : 0.0;  s[6 * kResPitch] = use ? y0 * y2 : 0.0;
        s[7 * kResPitch] = use ? y1 * y1 : 0.0;  s[8 * kResPitch] = use ? y1 * y2 : 0.0;  s[9 * kResPitch] = use ? y2 * y2 : 0.0;
        s[10 * kResPitch] = use ? 1.0 - bx * bx : 0.0;  s[11 * kResPitch] = use ? -(bx * by) : 0.0;  s[12 * kResPitch] = use ? -(bx * bz) : 0.0;
        s[13 * kResPitch] = use ? 1.0 - by * by : 0.0;  s[14 * kResPitch] = use ? -(by * bz) : 0.0;  s[15 * kResPitch] = use ? 1.0 - bz * bz : 0.0;
        res_sync();
        const double *sm = W.stage + mono * kResPitch, *sp = W.stage + (10 + ent) * kResPitch;
#pragma unroll 8
        for (int k = 0; k < 64; ++k) sum = fma(sm[k], sp[k], sum);
        res_sync();
    }
    // the staging area is free now: M, the copy Jacobi diagonalises, and its eigenvectors (columns), 81 doubles each
    double *const M = W.stage, *const A = W.stage + 81, *const V = W.stage + 162;
    // the sums as full matrices: S0, S1[a], and S2 straight into M (row 3 a + i, column 3 c + j)
    if (lane < 60) {
        int i, j;
        res_sym(ent, i, j);
        if (mono == 0) {
            W.S0[3 * i + j] = sum; W.S0[3 * j + i] = sum;
        } else if (mono < 4) {
            double *S = W.S1 + 9 * (mono - 1);
            S[3 * i + j] = sum; S[3 * j + i] = sum;
        } else {
            int a, c;
            res_sym(mono - 4, a, c);
            M[(3 * a + i) * 9 + 3 * c + j] = sum; M[(3 * a + j) * 9 + 3 * c + i] = sum;
            M[(3 * c + i) * 9 + 3 * a + j] = sum; M[(3 * c + j) * 9 + 3 * a + i] = sum;
        }
    }
    res_sync();
    // ---- S0 = L L^T, S0^-1 = L^-T L^-1 (every lane, in registers) ----
    const Chol3 L = chol3_factor(W.S0[0], W.S0[1], W.S0[2], W.S0[4], W.S0[5], W.S0[8]);
    if (!L.positive()) return kResDegenerate;
    const double i0 = L.i0, l10 = L.l10, l20 = L.l20, i1 = L.i1, l21 = L.l21, i2 = L.i2;
    const double m10 = -(l10 * i0) * i1, m20 = -(l20 * i0 + l21 * m10) * i2, m21 = -(l21 * i1) * i2;
    const double si00 = (i0 * i0 + m10 * m10) + m20 * m20, si01 = m10 * i1 + m20 * m21, si02 = m20 * i2;
    const double si11 = i1 * i1 + m21 * m21, si12 = m21 * i2, si22 = i2 * i2;
    if (lane == 0) {
        W.Si[0] = si00; W.Si[1] = si01; W.Si[2] = si02; W.Si[3] = si01; W.Si[4] = si11; W.Si[5] = si12;
        W.Si[6] = si02; W.Si[7] = si12; W.Si[8] = si22;
    }
    res_sync();
    // ---- M[(a,i),(c,j)] = S2[ac][ij] - (S1[a] S0^-1 S1[c])_ij: lane l < 45 owns entry l of the upper triangle and its mirror ----
    if (lane < 45) {
        int u = 0, rem = lane;
        while (rem >= 9 - u) { rem -= 9 - u; ++u; }
        const int v = u + rem;
        const int a = u / 3, i = u % 3, c = v / 3, j = v % 3;
        const double *Sa = W.S1 + 9 * a + 3 * i, *Sc = W.S1 + 9 * c + j;
        const double s0 = Sc[0], s1 = Sc[3], s2 = Sc[6];
        const double w0 = (W.Si[0] * s0 + W.Si[1] * s1) + W.Si[2] * s2;
        const double w1 = (W.Si[3] * s0 + W.Si[4] * s1) + W.Si[5] * s2;
        const double w2 = (W.Si[6] * s0 + W.Si[7] * s1) + W.Si[8] * s2;
        const double val = M[u * 9 + v] - ((Sa[0] * w0 + Sa[1] * w1) + Sa[2] * w2);
        M[u * 9 + v] = val; M[v * 9 + u] = val;
        A[u * 9 + v] = val; A[v * 9 + u] = val;
    }
    for (int k = lane; k < 81; k += 64) V[k] = k / 9 == k % 9 ? 1.0 : 0.0;
    res_sync();
    // ---- eigenpairs of M: cyclic Jacobi on A <- J^T A J, V <- V J.  A rotation is skipped when |a_pq| <= 1e-19 |M|_F. ----
    if (lane < 9) {
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) q += M[lane * 9 + k] * M[lane * 9 + k];
        W.T[lane] = q;
    }
    res_sync();
    double fro = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) fro += W.T[k];
    const double tol = 1e-19 * sqrt(fro);
    res_sync();
#pragma unroll 1
    for (int sweep = 0; sweep < kResSweeps; ++sweep) {
        bool any = false;
        // a sweep is nine rounds; round r rotates the four disjoint pairs ((r + m) % 9, (r - m) % 9), m = 1..4 (index r sits
        // out): every pair once per sweep, four rotations per dependent step
#pragma unroll 1
        for (int r = 0; r < 9; ++r) {
            int pi[4], qi[4];
            double cs[4], sn[4];
            bool on[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {                        // (wave-uniform: every lane reads the same entries)
                const int p = r + m + 1 >= 9 ? r + m + 1 - 9 : r + m + 1, q = r + 8 - m >= 9 ? r + 8 - m - 9 : r + 8 - m;
                const double apq = A[p * 9 + q], d = A[q * 9 + q] - A[p * 9 + p], two = 2.0 * apq;
                on[m] = fabs(apq) > tol;
                // t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = d / (2 a_pq), without the division by a_pq
                const double t = on[m] ? copysign(1.0, d) * two / (fabs(d) + sqrt(d * d + two * two)) : 0.0;
                cs[m] = 1.0 / sqrt(t * t + 1.0);
                sn[m] = t * cs[m];
                pi[m] = p; qi[m] = q;
                any = any || on[m];
            }
            if (lane < 9) {                                      // A <- A J, V <- V J: lane k owns row k
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    double *ap = A + lane * 9 + pi[m], *aq = A + lane * 9 + qi[m], *vp = V + lane * 9 + pi[m], *vq = V + lane * 9 + qi[m];
                    const double x = *ap, y = *aq, vx = *vp, vy = *vq;
                    *ap = cs[m] * x - sn[m] * y; *aq = sn[m] * x + cs[m] * y;
                    *vp = cs[m] * vx - sn[m] * vy; *vq = sn[m] * vx + cs[m] * vy;
                }
            }
            res_sync();
            if (lane < 9) {                                      // A <- J^T A: lane k owns column k; the rotated pair's entry is zero
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    double *ap = A + pi[m] * 9 + lane, *aq = A + qi[m] * 9 + lane;
                    const double x = *ap, y = *aq;
                    *ap = on[m] && lane == qi[m] ? 0.0 : cs[m] * x - sn[m] * y;
                    *aq = on[m] && lane == pi[m] ? 0.0 : sn[m] * x + cs[m] * y;
                }
            }
            res_sync();
        }
        if (!any) break;
    }
    // lambda_1 <= lambda_2, lambda_9 and the column of lambda_1
    double lam[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) lam[k] = A[10 * k];
    double l1 = lam[0], l9 = lam[0];
    int at = 0;
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        if (lam[k] < l1) { l1 = lam[k]; at = k; }
        l9 = fmax(l9, lam[k]);
    }
    double l2 = INFINITY;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        if (k != at && lam[k] < l2) l2 = lam[k];
        finite = finite && isfinite(lam[k]);
    }
    if (!finite || l2 < min_gap * l9 || l1 >= 0.25 * l2) return kResDegenerate;
    // ---- the rotation nearest G (G[i][a] = g[3 a + i]: g is G column-major), by X <- (X + X^-T) / 2 ----
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = V[k * 9 + at];
    {
        const double sg = res_det(R) < 0.0 ? -1.7320508075688772 : 1.7320508075688772;     // |G|_F = 1: a rotation over sqrt 3
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] *= sg;
    }
#pragma unroll 1
    for (int it = 0; it < kResPolarIters; ++it) {
        double C[9];                                             // the cofactors: X^-T = C / det
        C[0] = R[4] * R[8] - R[5] * R[7]; C[1] = R[5] * R[6] - R[3] * R[8]; C[2] = R[3] * R[7] - R[4] * R[6];
        C[3] = R[7] * R[2] - R[8] * R[1]; C[4] = R[8] * R[0] - R[6] * R[2]; C[5] = R[6] * R[1] - R[7] * R[0];
        C[6] = R[1] * R[5] - R[2] * R[4]; C[7] = R[2] * R[3] - R[0] * R[5]; C[8] = R[0] * R[4] - R[1] * R[3];
        const double idet = 1.0 / ((R[0] * C[0] + R[1] * C[1]) + R[2] * C[2]);
        double moved = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double n = 0.5 * (R[k] + C[k] * idet);
            moved = fmax(moved, fabs(n - R[k]));
            R[k] = n;
        }
        if (!(moved > 1e-15)) break;
    }
    // ---- Gauss-Newton on r^T M r over R <- exp([delta]x) R, r = R column-major, J_k = vec([e_k]x R) ----
#pragma unroll 1
    for (int it = 0; it < kResGnIters; ++it) {
        if (lane < 9) {
            const double *Mk = M + lane * 9;
            double mr = 0.0, mj0 = 0.0, mj1 = 0.0, mj2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double x = R[3 * a], y = R[3 * a + 1], z = R[3 * a + 2];
                const double ma = Mk[3 * a], mb = Mk[3 * a + 1], mc = Mk[3 * a + 2];
                mr += (ma * x + mb * y) + mc * z;
                mj0 += mc * y - mb * z;                          // e_0 x v = (0, -z, y)
                mj1 += ma * z - mc * x;                          // e_1 x v = (z, 0, -x)
                mj2 += mb * x - ma * y;                          // e_2 x v = (-y, x, 0)
            }
            W.T[lane] = mr; W.T[9 + lane] = mj0; W.T[18 + lane] = mj1; W.T[27 + lane] = mj2;
        }
        res_sync();
        double g[3], h0[3], h1[3], h2[3];                        // J^T M r and the columns of H = J^T M J
        res_jt(R, W.T, g);
        res_jt(R, W.T + 9, h0);
        res_jt(R, W.T + 18, h1);
        res_jt(R, W.T + 27, h2);
        const double H[6] = {h0[0], h1[0], h2[0], h1[1], h2[1], h2[2]};          // 00 01 02 11 12 22: the upper triangle
        res_sync();
        const Chol3 Lh = chol3_factor(H[0], H[1], H[2], H[3], H[4], H[5]);
        if (!Lh.positive()) return kResDegenerate;
        double dl0, dl1, dl2;
        Lh.solve(-g[0], -g[1], -g[2], dl0, dl1, dl2);
        if (!(isfinite(dl0) && isfinite(dl1) && isfinite(dl2))) return kResDegenerate;
        double E[9], N[9];
        from_rodrigues(dl0, dl1, dl2, E);
        cm_mat_mul(E, R, N);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = N[k];
        if (!(sqrt((dl0 * dl0 + dl1 * dl1) + dl2 * dl2) > 1e-14)) break;
    }
    // ---- t = t'(R) - R centroid, t' = -S0^-1 sum_a S1[a] R[:, a] ----
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double *S = W.S1 + 9 * a;
        const double x = R[3 * a], y = R[3 * a + 1], z = R[3 * a + 2];
        v0 += (S[0] * x + S[1] * y) + S[2] * z;
        v1 += (S[3] * x + S[4] * y) + S[5] * z;
        v2 += (S[6] * x + S[7] * y) + S[8] * z;
    }
    const double t0 = -((si00 * v0 + si01 * v1) + si02 * v2) - ((R[0] * cx + R[3] * cy) + R[6] * cz);
    const double t1 = -((si01 * v0 + si11 * v1) + si12 * v2) - ((R[1] * cx + R[4] * cy) + R[7] * cz);
    const double t2 = -((si02 * v0 + si12 * v1) + si22 * v2) - ((R[2] * cx + R[5] * cy) + R[8] * cz);
    bool good = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) good = good && isfinite(R[k]);
    if (!(good && isfinite(t0) && isfinite(t1) && isfinite(t2))) return kResDegenerate;
    // ---- walk 3: cheirality ----
    bool behind = false;
#pragma unroll 1
    for (uint64_t j0 = b; j0 < e; j0 += 64) {
        const uint64_t j = j0 + lane;
        double bx, by, bz, x = 0.0, y = 0.0, z = 0.0;
        const bool use = j < e && res_observation(in, pts4, pt_idx, uv_obs, j, bx, by, bz, x, y, z) && keep(j, x, y, z);
        const double qz = ((R[2] * x + R[5] * y) + R[8] * z) + t2;
        behind = behind || __ballot(use && qz >= 0.0) != 0ull;
    }
    if (behind) return kResBehind;
    if (lane == 0) {
        double w[3];
        to_rodrigues(R, w);
        cam[0] = w[0]; cam[1] = w[1]; cam[2] = w[2];
        cam[3] = t0; cam[4] = t1; cam[5] = t2;
    }
    return kResOk;
}

// cam_mask == NULL: no camera is constant.  counts[kResKinds] must be zero when the kernel starts.
__global__ __launch_bounds__(kResBlock) void k_resect_cameras(
    double *__restrict__ bal9, const double4 *__restrict__ pts4, const uint64_t *__restrict__ row_ptr, int64_t n_cam,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, int min_points, double min_gap,
    const uint16_t *__restrict__ cam_mask, uint8_t *__restrict__ status, unsigned long long *__restrict__ counts) {
    __shared__ ResLds sW[kResWaves];
    __shared__ unsigned sCnt[kResKinds];
    if (threadIdx.x < kResKinds) sCnt[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * kResWaves + wave;
    if (c < n_cam) {                                             // wave-uniform
        int st = kResConstant;
        if (!cam_mask || !(cam_mask[c] & 0x3f))                  // C2B_CONST_POSE
            st = resect_camera(sW[wave], lane, bal9 + 9 * c, pts4, row_ptr[c], row_ptr[c + 1], pt_idx, uv_obs, min_points, min_gap, ResKeepAll());
        if (lane == 0) {
            status[c] = (uint8_t)st;
            atomicAdd(&sCnt[st], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kResKinds && sCnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)sCnt[threadIdx.x]);
}

}  // namespace c2b
