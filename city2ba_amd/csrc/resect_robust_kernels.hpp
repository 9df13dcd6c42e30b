// resect_robust_kernels.hpp -- gfx950 kernel of consensus resection (included by capi.hip only, after resect_kernels.hpp and
// triangulate_robust_kernels.hpp).
//
// c2b_resect_consensus_rows / c2b_problem_resect_consensus: k_resect_cameras' fit over the observations that
// agree with each other, for a camera whose row also names points its pixels do not belong to (wrong matches).
//   * k_resect_consensus: camera-major, one wave per camera, the row walked 64 entries at a time.
//       count     the usable entries of the whole row (res_observation, ballots): fewer than min_inliers is TOO_FEW;
//       sample    lanes = the row's first 64 entries: the usable rays and points compacted in row order into wave-private
//                 LDS (the head of resect_camera's staging area, 48 B x 64);
//       hypothesis lane k = triple k of the sample, wide gaps first (rrc_triple).  Its three-point poses: the quartic in
//                 v = l3 / l1 (rrc_quartic), all four complex roots at once by Durand-Kerner, every root that is real within
//                 kRrcImag a start with both depths l2 the first equation allows -- more starts than solutions on purpose;
//                 what makes a solution is Newton on the three equations (rrc_polish), its last step, the sign of the depths,
//                 the determinant of the equations' Jacobian and the merge of duplicates.  A lane keeps at most four depth
//                 triples, in registers with compile-time indices;
//       score     the solution number outermost (one pose per lane live): the row again chunk by chunk, the lanes find the
//                 usable entries, then for every set bit every lane projects THAT point through ITS pose -- wave-uniform
//                 addresses and intrinsics, so project_obs' k2 != 0 route is taken by all lanes or none -- and counts the
//                 filter's predicate (trc_fits) in an integer; a lane keeps its best (score, then the smaller l1);
//       select    the wave's maximum of (score, -k); the winning lane rebuilds its pose and leaves it in LDS;
//       refit     resect_camera with "inlier of the winning pose" as its keep predicate, evaluated again in each of its three
//                 walks: bit for bit k_resect_cameras on the list restricted to the inliers;
//       mask      one more walk once the refit is C2B_RES_OK: the zeros of the inlier mask.
//   * the six status counts: LDS integer atomics per workgroup, then at most six 64-bit integer atomics per workgroup.
// Every loop is bounded by the row length, 64, or a fixed iteration cap; no wave waits for another.  No float atomics, no
// scratch memory, nothing stored per row: a camera's result depends on its own row alone.
#pragma once
#include "resect_kernels.hpp"
#include "triangulate_robust_kernels.hpp"

namespace c2b {

constexpr int kRrcSample = 64;                               // the sample window and the most hypotheses: one per lane
enum { kResNoConsensus = 5, kRrcKinds = 6 };                 // C2B_RES_NO_CONSENSUS; the statuses of the consensus pass
constexpr int kRrcRootIters = 48, kRrcNewtonSteps = 8;
constexpr double kRrcImag = 1e-2;                            // a root z is a start when |Im z| <= kRrcImag (1 + |Re z|)
constexpr double kRrcCollinear = 1e-12, kRrcCond = 1e-5, kRrcMerge = 1e-9, kRrcAccept = 1e-9, kRrcNewtonTol = 1e-14;

struct RrcLds {                                              // one wave's
    ResLds res;                                              // the refit's; before it, res.stage holds the sample (field-major, pitch 64)
    double pose[16];                                         // the winning pose as a camblk record: R row-major, t, f, k1, k2
};

// a pose and the camera's intrinsics, indexed as project_obs indexes a camblk record
struct RrcPose {
    double m[12], f, k1, k2;
    __device__ __forceinline__ double operator[](int j) const { return j < 12 ? m[j] : (j == 12 ? f : (j == 13 ? k1 : k2)); }
};

// resect_camera's keep predicate: the observation is an inlier of the pose in LDS
struct RrcKeep {
    const double *pose;
    const double2 *__restrict__ uv_obs;
    double max_err2;
    __device__ __forceinline__ bool operator()(uint64_t j, double x, double y, double z) const {
        return trc_fits(pose, uv_obs[j], x, y, z, max_err2);
    }
};

// Triple number k of a sample of m: the gap g runs from m / 3 down to 1, i over 0 .. m - 1 (3 g == m: i < g only, each
// triple once), the triple is {i, (i + g) mod m, (i + 2 g) mod m} ascending.  false when there is no k-th triple.
C2B_DEV bool rrc_triple(int k, int m, int &i0, int &i1, int &i2) {
    const int third = m / 3;
    const bool exact = third * 3 == m;
    int g, i;
    if (exact && k < third) {
        g = third; i = k;
    } else {
        const int r = exact ? k - third : k;
        g = (exact ? third - 1 : third) - r / (m > 0 ? m : 1);
        i = r % (m > 0 ? m : 1);
    }
    i0 = i1 = i2 = 0;
    if (m < 3 || g < 1) return false;
    int a = i, b = i + g, c = i + 2 * g;
    if (b >= m) b -= m;
    if (c >= m) c -= m;
    if (c >= m) c -= m;
    // (a, b, c) is a rotation of an ascending sequence: sort three
    const int lo = min(a, min(b, c)), hi = max(a, max(b, c));
    i0 = lo; i1 = a + b + c - lo - hi; i2 = hi;
    return true;
}

// The monic quartic q[0] + q[1] v + q[2] v^2 + q[3] v^3 + v^4 in v = l3 / l1, distances over |X1 - X3|: A = |X2 - X3|^2 /
// |X1 - X3|^2, C = |X1 - X2|^2 / |X1 - X3|^2, ca = b2 . b3, cb = b1 . b3, cg = b1 . b2.  The difference of the first two
// equations over the second gives l2 / l1 = N(v) / D(v), N = n0 + n1 v + n2 v^2, D = d0 + d1 v; the first equation over the
// second is then N^2 - 2 cg N D + D^2 = C (1 - 2 cb v + v^2) D^2.
C2B_DEV void rrc_quartic(double A, double C, double ca, double cb, double cg, double q[4]) {
    const double w = C - A;
    const double n0 = w - 1.0, n1 = -2.0 * cb * w, n2 = w + 1.0, d0 = -2.0 * cg, d1 = 2.0 * ca;
    const double D0 = d0 * d0, D1 = 2.0 * d0 * d1, D2 = d1 * d1;
    const double g2 = -2.0 * cg, b2 = -2.0 * cb;
    const double c0 = (n0 * n0 + g2 * (n0 * d0) + D0) - C * D0;
    const double c1 = (2.0 * n0 * n1 + g2 * (n0 * d1 + n1 * d0) + D1) - C * (D1 + b2 * D0);
    const double c2 = ((n1 * n1 + 2.0 * n0 * n2) + g2 * (n1 * d1 + n2 * d0) + D2) - C * ((D2 + b2 * D1) + D0);
    const double c3 = (2.0 * n1 * n2 + g2 * (n2 * d1)) - C * (b2 * D2 + D1);
    const double c4 = n2 * n2 - C * D2;
    const double inv = 1.0 / c4;
    q[0] = c0 * inv; q[1] = c1 * inv; q[2] = c2 * inv; q[3] = c3 * inv;
}

// All four roots of the monic quartic by Durand-Kerner (each root moves by p(z) over the product of its distances to the
// others, the others as already moved), from four points on a circle of Fujiwara's radius; at most kRrcRootIters rounds.
C2B_DEV void rrc_roots(const double q[4], double zr[4], double zi[4]) {
    const double rad = 2.0 * fmax(fmax(fabs(q[3]), sqrt(fabs(q[2]))), fmax(cbrt(fabs(q[1])), sqrt(sqrt(0.5 * fabs(q[0])))));
    // one start per quadrant, at unequal angles and radii: no symmetry of the quartic maps the starts onto themselves
    zr[0] = 0.7648421872844885 * rad; zi[0] = 0.644217687237691 * rad;
    zr[1] = -0.7373937155412454 * rad; zi[1] = 0.675463180551151 * rad;
    zr[2] = -0.6145775846805336 * rad; zi[2] = -0.6574911207042632 * rad;
    zr[3] = 0.4322418446945118 * rad; zi[3] = -0.6731767878463172 * rad;
#pragma unroll 1
    for (int it = 0; it < kRrcRootIters; ++it) {
        double moved = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double x = zr[a], y = zi[a];
            // p(z) by Horner
            double pr = x + q[3], pi = y;
            double tr = pr * x - pi * y + q[2], ti = pr * y + pi * x;
            pr = tr * x - ti * y + q[1]; pi = tr * y + ti * x;
            tr = pr * x - pi * y + q[0]; ti = pr * y + pi * x;
            double dr = 1.0, di = 0.0;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (o == a) continue;
                const double ex = x - zr[o], ey = y - zi[o];
                const double nr = dr * ex - di * ey;
                di = dr * ey + di * ex;
                dr = nr;
            }
            const double den = dr * dr + di * di;
            if (den > 0.0) {
                const double sx = (tr * dr + ti * di) / den, sy = (ti * dr - tr * di) / den;
                zr[a] = x - sx; zi[a] = y - sy;
                moved = fmax(moved, fmax(fabs(sx), fabs(sy)));
            }
        }
        if (!(moved > 1e-15 * rad)) break;                   // (a NaN ends it too)
    }
}

// the three equations l_i^2 + l_j^2 - 2 l_i l_j c_ij = d_ij for the pairs (1, 2), (1, 3), (2, 3)
struct RrcTri { double c12, c13, c23, d12, d13, d23; };

// the determinant of the equations' Jacobian rows (j00 j01 0), (j10 0 j12), (0 j21 j22)
C2B_DEV double rrc_det(double j00, double j01, double j10, double j12, double j21, double j22) {
    return -(j00 * (j12 * j21)) - j01 * (j10 * j22);
}

// Newton on the three equations from (l1, l2, l3): at most kRrcNewtonSteps steps, until max |step| <= kRrcNewtonTol max l.
// true when the run ended at a solution that is formed: every depth finite and > 0, the last step at most kRrcAccept max l,
// |det J| > kRrcCond (2 max l)^3.
C2B_DEV bool rrc_polish(const RrcTri &T, double &l1, double &l2, double &l3) {
    double last = INFINITY;
#pragma unroll 1
    for (int it = 0; it < kRrcNewtonSteps; ++it) {
        const double f0 = ((l1 * l1 + l2 * l2) - 2.0 * l1 * l2 * T.c12) - T.d12;
        const double f1 = ((l1 * l1 + l3 * l3) - 2.0 * l1 * l3 * T.c13) - T.d13;
        const double f2 = ((l2 * l2 + l3 * l3) - 2.0 * l2 * l3 * T.c23) - T.d23;
        const double j00 = 2.0 * (l1 - l2 * T.c12), j01 = 2.0 * (l2 - l1 * T.c12);
        const double j10 = 2.0 * (l1 - l3 * T.c13), j12 = 2.0 * (l3 - l1 * T.c13);
        const double j21 = 2.0 * (l2 - l3 * T.c23), j22 = 2.0 * (l3 - l2 * T.c23);
        const double det = rrc_det(j00, j01, j10, j12, j21, j22);
        // Cramer: column k of J replaced by F
        const double s1 = (-(f0 * (j12 * j21)) - j01 * (f1 * j22 - j12 * f2)) / det;
        const double s2 = (j00 * (f1 * j22 - j12 * f2) - f0 * (j10 * j22)) / det;
        const double s3 = (j00 * (-(f1 * j21)) - j01 * (j10 * f2) + f0 * (j10 * j21)) / det;
        l1 -= s1; l2 -= s2; l3 -= s3;
        last = fmax(fabs(s1), fmax(fabs(s2), fabs(s3)));
        if (last <= kRrcNewtonTol * fmax(l1, fmax(l2, l3))) break;
        if (!(last < INFINITY)) break;                       // (NaN or infinite: nothing comes of this start)
    }
    const double top = fmax(l1, fmax(l2, l3));
    if (!(isfinite(l1) && isfinite(l2) && isfinite(l3) && l1 > 0.0 && l2 > 0.0 && l3 > 0.0 && last <= kRrcAccept * top)) return false;
    const double det = rrc_det(2.0 * (l1 - l2 * T.c12), 2.0 * (l2 - l1 * T.c12), 2.0 * (l1 - l3 * T.c13), 2.0 * (l3 - l1 * T.c13),
                               2.0 * (l2 - l3 * T.c23), 2.0 * (l3 - l2 * T.c23));
    const double two = 2.0 * top;
    return fabs(det) > kRrcCond * (two * two * two);
}

// the orthonormal frame of the triangle p1 p2 p3: e1 along 1 -> 2, e3 along e1 x (1 -> 3), e2 = e3 x e1
C2B_DEV void rrc_frame(const double p1[3], const double p2[3], const double p3[3], double e1[3], double e2[3], double e3[3]) {
    const double ax = p2[0] - p1[0], ay = p2[1] - p1[1], az = p2[2] - p1[2];
    const double ia = 1.0 / sqrt((ax * ax + ay * ay) + az * az);
    e1[0] = ax * ia; e1[1] = ay * ia; e1[2] = az * ia;
    const double bx = p3[0] - p1[0], by = p3[1] - p1[1], bz = p3[2] - p1[2];
    const double cx = e1[1] * bz - e1[2] * by, cy = e1[2] * bx - e1[0] * bz, cz = e1[0] * by - e1[1] * bx;
    const double ic = 1.0 / sqrt((cx * cx + cy * cy) + cz * cz);
    e3[0] = cx * ic; e3[1] = cy * ic; e3[2] = cz * ic;
    e2[0] = e3[1] * e1[2] - e3[2] * e1[1]; e2[1] = e3[2] * e1[0] - e3[0] * e1[2]; e2[2] = e3[0] * e1[1] - e3[1] * e1[0];
}

// the sample's slot s: ray and point
C2B_DEV void rrc_slot(const double *S, int s, double b[3], double X[3]) {
    b[0] = S[s]; b[1] = S[64 + s]; b[2] = S[128 + s];
    X[0] = S[192 + s]; X[1] = S[256 + s]; X[2] = S[320 + s];
}

// R (row-major) = camera frame . (world frame)^T and t = l1 b1 - R X1 of the depths (l1, l2, l3) of the triple in slots i0 i1 i2
C2B_DEV void rrc_pose(const double *S, int i0, int i1, int i2, double l1, double l2, double l3, double m[12]) {
    double b1[3], b2[3], b3[3], X1[3], X2[3], X3[3];
    rrc_slot(S, i0, b1, X1); rrc_slot(S, i1, b2, X2); rrc_slot(S, i2, b3, X3);
    double p1[3], p2[3], p3[3], c1[3], c2[3], c3[3], w1[3], w2[3], w3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { p1[a] = l1 * b1[a]; p2[a] = l2 * b2[a]; p3[a] = l3 * b3[a]; }
    rrc_frame(p1, p2, p3, c1, c2, c3);
    rrc_frame(X1, X2, X3, w1, w2, w3);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) m[3 * r + c] = (c1[r] * w1[c] + c2[r] * w2[c]) + c3[r] * w3[c];
#pragma unroll
    for (int r = 0; r < 3; ++r) m[9 + r] = p1[r] - ((m[3 * r] * X1[0] + m[3 * r + 1] * X1[1]) + m[3 * r + 2] * X1[2]);
}

// entry s of four values, by selects: the index of a register array must be a compile-time constant, or the array is scratch
C2B_DEV double rrc_pick(int s, double a0, double a1, double a2, double a3) { return s == 0 ? a0 : (s == 1 ? a1 : (s == 2 ? a2 : a3)); }

// depth triple s of a lane's four
C2B_DEV void rrc_pick3(const double (&L)[4][3], int s, double &l1, double &l2, double &l3) {
    l1 = rrc_pick(s, L[0][0], L[1][0], L[2][0], L[3][0]);
    l2 = rrc_pick(s, L[0][1], L[1][1], L[2][1], L[3][1]);
    l3 = rrc_pick(s, L[0][2], L[1][2], L[2][2], L[3][2]);
}

// One camera by the wave that calls it; every lane returns the same status.  hyp_out / n_inl_out: the selected triple and its
// inlier count (-1 / 0 when none was selected).  [rb, re) is the camera's row of the list.
C2B_DEV int resect_consensus_camera(RrcLds &W, const int lane, double *__restrict__ cam, const double4 *__restrict__ pts4, const uint64_t rb,
                                    const uint64_t re, const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs,
                                    const double max_err2_, const int min_inliers, const double min_gap_, const int max_hypotheses,
                                    uint8_t *__restrict__ inlier, int &hyp_out, int &n_inl_out) {
    hyp_out = -1;
    n_inl_out = 0;
    // the two thresholds wait in vector registers: as scalars, next to the row's bounds, the pointers and the pow route's
    // constants, they push the score loop's masks out of the scalar file (tests/test_isa_pins.py allows no scalar spill)
    double max_err2 = max_err2_, min_gap = min_gap_;
    uint64_t inlier_at = reinterpret_cast<uint64_t>(inlier);     // (and the mask's address, which only the last walk's lanes use)
    asm volatile("" : "+v"(max_err2), "+v"(min_gap), "+v"(inlier_at));
    // (so do the intrinsics: three more scalar pairs, live from here to the mask walk)
    ResIntrinsics in = {cam[6], cam[7], cam[8]};
    asm volatile("" : "+v"(in.f), "+v"(in.k1), "+v"(in.k2));
    double *const S = W.res.stage;
    // ---- the usable entries of the whole row; the sample: those among the first 64, compacted in row order ----
    int n_used = 0, m = 0;
#pragma unroll 1
    for (uint64_t j0 = rb; j0 < re; j0 += 64) {
        const uint64_t j = j0 + lane;
        double bx = 0.0, by = 0.0, bz = 0.0, x = 0.0, y = 0.0, z = 0.0;
        const bool use = j < re && res_observation(in, pts4, pt_idx, uv_obs, j, bx, by, bz, x, y, z);
        const uint64_t mask = __ballot(use);
        n_used += __popcll(mask);
        if (j0 == rb) {                                      // wave-uniform
            m = __popcll(mask);
            if (use) {
                const int slot = __popcll(mask & ((1ull << lane) - 1ull));
                S[slot] = bx; S[64 + slot] = by; S[128 + slot] = bz;
                S[192 + slot] = x; S[256 + slot] = y; S[320 + slot] = z;
            }
        }
    }
    if (n_used < min_inliers) return kResTooFew;
    res_sync();
    // ---- hypotheses: lane k finds the depth triples of triple k ----
    double L[4][3];
#pragma unroll
    for (int s = 0; s < 4; ++s) L[s][0] = L[s][1] = L[s][2] = 0.0;
    int n_sol = 0, i0, i1, i2;
    if (rrc_triple(lane, m, i0, i1, i2) && lane < max_hypotheses) {
        RrcTri T;
        double A, C;
        bool spread;
        {
            double b1[3], b2[3], b3[3], X1[3], X2[3], X3[3];
            rrc_slot(S, i0, b1, X1); rrc_slot(S, i1, b2, X2); rrc_slot(S, i2, b3, X3);
            T.c12 = (b1[0] * b2[0] + b1[1] * b2[1]) + b1[2] * b2[2];
            T.c13 = (b1[0] * b3[0] + b1[1] * b3[1]) + b1[2] * b3[2];
            T.c23 = (b2[0] * b3[0] + b2[1] * b3[1]) + b2[2] * b3[2];
            const double ux = X2[0] - X1[0], uy = X2[1] - X1[1], uz = X2[2] - X1[2];
            const double vx = X3[0] - X1[0], vy = X3[1] - X1[1], vz = X3[2] - X1[2];
            const double wx = X3[0] - X2[0], wy = X3[1] - X2[1], wz = X3[2] - X2[2];
            T.d12 = (ux * ux + uy * uy) + uz * uz;
            T.d13 = (vx * vx + vy * vy) + vz * vz;
            T.d23 = (wx * wx + wy * wy) + wz * wz;
            const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
            spread = ((cx * cx + cy * cy) + cz * cz) >= kRrcCollinear * T.d12 * T.d13;       // (a NaN forms nothing)
            A = T.d23 / T.d13; C = T.d12 / T.d13;
        }
        if (spread) {
            double q[4], zr[4], zi[4];
            rrc_quartic(A, C, T.c23, T.c13, T.c12, q);
            rrc_roots(q, zr, zi);
#pragma unroll 1
            for (int cand = 0; cand < 8; ++cand) {
                const int a = cand >> 1;
                const double vr = rrc_pick(a, zr[0], zr[1], zr[2], zr[3]), vi = rrc_pick(a, zi[0], zi[1], zi[2], zi[3]);
                if (!(fabs(vi) <= kRrcImag * (1.0 + fabs(vr)))) continue;
                double l1 = sqrt(T.d13 / fmax((1.0 - 2.0 * T.c13 * vr) + vr * vr, 1e-300));
                const double disc = T.d12 - l1 * l1 * (1.0 - T.c12 * T.c12);
                const double root = sqrt(fmax(disc, 0.0));
                double l2 = (cand & 1) ? l1 * T.c12 - root : l1 * T.c12 + root;
                double l3 = vr * l1;
                // rrc_polish tests the conditioning before the merge below, the reference after it: two starts that merge end within
                // 1e-9 of one solution and its determinant, so both orders keep or drop the same solutions (a determinant that
                // close to its threshold is excused).  Positive depths have at most four solutions: the cap below drops nothing.
                if (!rrc_polish(T, l1, l2, l3)) continue;
                const double top = fmax(l1, fmax(l2, l3));
                bool dup = false;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double dist = fmax(fabs(l1 - L[s][0]), fmax(fabs(l2 - L[s][1]), fabs(l3 - L[s][2])));
                    const double other = fmax(L[s][0], fmax(L[s][1], L[s][2]));
                    dup = dup || (s < n_sol && dist <= kRrcMerge * fmax(top, other));
                }
                if (dup || n_sol >= 4) continue;
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (s == n_sol) { L[s][0] = l1; L[s][1] = l2; L[s][2] = l3; }
                ++n_sol;
            }
        }
    }
    const uint64_t formed_mask = __ballot(n_sol > 0);
    if (formed_mask == 0ull) return kResDegenerate;
    int most = n_sol;                                        // the wave's largest solution count
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) most = max(most, __shfl_xor(most, d, 64));
    // ---- score: every usable entry of the row against every lane's pose, one solution number at a time ----
    int best = -1, best_s = 0;
    double best_l1 = 0.0;
    const int n = (int)(re - rb);                            // (the launcher holds n_obs below 2^31 - 64)
#pragma unroll 1
    for (int s = 0; s < most; ++s) {
        const bool mine = s < n_sol;
        double l1, l2, l3;
        rrc_pick3(L, s, l1, l2, l3);
        RrcPose P;
        P.f = in.f; P.k1 = in.k1; P.k2 = in.k2;
        if (mine) {
            rrc_pose(S, i0, i1, i2, l1, l2, l3, P.m);
        } else {
#pragma unroll
            for (int a = 0; a < 12; ++a) P.m[a] = 0.0;
        }
        int score = 0;
#pragma unroll 1
        for (int t0 = 0; t0 < n; t0 += 64) {
            bool use = false;
            if (t0 + lane < n) {
                double bx, by, bz, x, y, z;
                use = res_observation(in, pts4, pt_idx, uv_obs, rb + (uint64_t)(t0 + lane), bx, by, bz, x, y, z);
            }
            uint64_t use_mask = __ballot(use);
#pragma unroll 1
            while (use_mask != 0ull) {                       // wave-uniform
                // the same entry in every lane, but its index held in a vector register: as scalars the point, the pixel and
                // the pow route's constants do not fit the scalar file next to the row's bounds (the hardware serves the one
                // address once)
                uint32_t at = (uint32_t)(t0 + __builtin_ctzll(use_mask));
                asm volatile("" : "+v"(at));
                const uint64_t j = rb + (uint64_t)at;
                use_mask &= use_mask - 1ull;
                const double2 *X = reinterpret_cast<const double2 *>(pts4 + pt_idx[j]);
                const double2 xy = X[0];
                const double z = reinterpret_cast<const double *>(X + 1)[0];
                score += trc_fits(P, uv_obs[j], xy.x, xy.y, z, max_err2) ? 1 : 0;
            }
        }
        if (mine && (score > best || (score == best && l1 < best_l1))) { best = score; best_s = s; best_l1 = l1; }
    }
    // ---- select: the highest score, the lowest k among equals ----
    long long key = n_sol > 0 ? (long long)best * 64 + (63 - lane) : -1ll;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long other = __shfl_xor(key, d, 64);
        key = other > key ? other : key;
    }
    const int win = 63 - (int)(key & 63ll);
    const int n_inl = (int)(key >> 6);
    hyp_out = win;
    n_inl_out = n_inl;
    if (n_inl < min_inliers) return kResNoConsensus;
    if (lane == win) {
        double l1, l2, l3;
        rrc_pick3(L, best_s, l1, l2, l3);
        double mm[12];
        rrc_pose(S, i0, i1, i2, l1, l2, l3, mm);
#pragma unroll
        for (int a = 0; a < 12; ++a) W.pose[a] = mm[a];
        W.pose[12] = in.f; W.pose[13] = in.k1; W.pose[14] = in.k2;
    }
    res_sync();                                              // the pose is in LDS; the sample's slots are staged over below
    // ---- refit: k_resect_cameras' own routine over the winner's inliers ----
    const RrcKeep keep = {W.pose, uv_obs, max_err2};
    const int st = resect_camera(W.res, lane, cam, pts4, rb, re, pt_idx, uv_obs, min_inliers, min_gap, keep);
    if (st != kResOk) return st;
    // ---- the zeros of the mask ----
    if (inlier_at) {
        __attribute__((address_space(1))) uint8_t *const mask_out = reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(inlier_at);
#pragma unroll 1
        for (int t0 = 0; t0 < n; t0 += 64) {
            if (t0 + lane < n) {
                const uint64_t j = rb + (uint64_t)(t0 + lane);
                double bx, by, bz, x = 0.0, y = 0.0, z = 0.0;
                const bool in_set = res_observation(in, pts4, pt_idx, uv_obs, j, bx, by, bz, x, y, z) && keep(j, x, y, z);
                if (!in_set) mask_out[j] = 0;
            }
        }
    }
    return kResOk;
}

// cam_mask == NULL: no camera is constant; hyp, n_inl, inlier may be NULL.  counts[kRrcKinds] must be zero and inlier all
// ones when the kernel starts.
__global__ __launch_bounds__(kResBlock) void k_resect_consensus(
    double *__restrict__ bal9, const double4 *__restrict__ pts4, const uint64_t *__restrict__ row_ptr, int64_t n_cam,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, double max_err2, int min_inliers, double min_gap,
    int max_hypotheses, const uint16_t *__restrict__ cam_mask, uint8_t *__restrict__ status, int32_t *__restrict__ hyp,
    int32_t *__restrict__ n_inl, uint8_t *__restrict__ inlier, unsigned long long *__restrict__ counts) {
    __shared__ RrcLds sW[kResWaves];
    __shared__ unsigned sCnt[kRrcKinds];
    if (threadIdx.x < kRrcKinds) sCnt[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * kResWaves + wave;
    if (c < n_cam) {                                             // wave-uniform
        int st = kResConstant, h = -1, n = 0;
        if (!cam_mask || !(cam_mask[c] & 0x3f))                  // C2B_CONST_POSE
            st = resect_consensus_camera(sW[wave], lane, bal9 + 9 * c, pts4, row_ptr[c], row_ptr[c + 1], pt_idx, uv_obs, max_err2,
                                         min_inliers, min_gap, max_hypotheses, inlier, h, n);
        if (lane == 0) {
            status[c] = (uint8_t)st;
            if (hyp) hyp[c] = h;
            if (n_inl) n_inl[c] = n;
            atomicAdd(&sCnt[st], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kRrcKinds && sCnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)sCnt[threadIdx.x]);
}

}  // namespace c2b
