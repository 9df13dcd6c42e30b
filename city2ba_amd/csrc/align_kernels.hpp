// align_kernels.hpp -- similarity alignment of two problems whose indices correspond (included by capi.hip only).
//
// Both entity tables of a problem are 32-byte rows (cen4: a camera's centre, pts4: a point), so ONE source serves cameras, points and
// the two pooled: correspondence i is (x_i from the estimate, y_i from the reference), cameras first, then points, each kind with an
// optional byte mask (NULL: all on).  The passes are streaming reads in the shape of k_stats_pass1 -- kAlignBlock threads, at most
// kAlignGrid workgroups striding the table, kAlignBatch entities per thread and trip with every load issued before the first use:
//   k_align_means            count and the six coordinate sums of the on-correspondences
//   k_align_moments          the eleven second moments CENTRED on the pivot m = sums / count of the first pass, and the six residual sums
//                            sum (x - mx), sum (y - my).  The pivot is the mean rounded to a double; the residual sums give what the rounding
//                            lost, and the host moves the moments from the pivot to the mean (-n d d^T: second order, 1e-14 of the moment
//                            where the cloud sits 1e9 spreads from the origin).  No raw moment sum xx^T - n mu mu^T is ever formed.
//   k_align_errors<E>        per-entity error after alignment (position: |s R x + t - y|; rotation: the angle between R_c R^T and the
//                            reference's R_c), the next trimmed set, and the summary over a set: count, sum e^2, sum e, max and the LOWEST index
//                            that attains it, bytes that changed against the set, size of the next set
//   k_similarity_apply_*     X <- s R X + t on pts4; R_c <- R_c R^T, t_c <- -R_c' (s R c + t) on cam15
// No float atomics: the sums of the first two go through ticket_fold_n, the summary through records published and counted exactly as
// k_stats_pass1 publishes its own (agent-scope stores, drained, then ticket_arrive) and folded by the last workgroup in a fixed order; the
// maximum and its index are order-free by construction (ties to the lower index).  The same inputs give the same bits.
#pragma once
#include "kernels.hpp"

namespace c2b {

constexpr int kAlignBlock = 256;      // threads per workgroup
constexpr int kAlignGrid = 256;       // most workgroups of a pass: one per CU; each partial set of a fold and every summary record has a slot per workgroup
constexpr int kAlignBatch = 4;        // entities a thread loads before it uses any
constexpr int kAlignWaves = kAlignBlock / 64;
constexpr int kAlignMeans = 7;        // count, sum x (3), sum y (3)
constexpr int kAlignMoments = 17;     // sum |x - mx|^2, sum |y - my|^2, sum (y - my)(x - mx)^T row-major (9), sum (x - mx) (3), sum (y - my) (3)
constexpr int kAlignMomentsOut = kAlignMoments + 6;      // ... and the pivot they are centred on: mx (3), my (3)
constexpr int kAlignSummary = 7;      // count, sum e^2, sum e, max, argmax, changed bytes, size of the next set
constexpr int kAlignRec = 8;          // doubles per summary record (a 64-byte slot)
static_assert(kAlignMoments * kAlignGrid <= kRedBlocks * kStatRec && kAlignRec * kAlignGrid <= kRedBlocks * kStatRec,
              "partials and records live in the workspace's record area");

// a similarity y = s R x + t (R row-major), by value in the kernel arguments
struct AlignSim { double s, R[9], t[3]; };

C2B_DEV void align_map(const AlignSim &T, const double (&x)[3], double (&o)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = T.s * dot3(T.R[3 * r], T.R[3 * r + 1], T.R[3 * r + 2], x[0], x[1], x[2]) + T.t[r];
}

C2B_DEV void align_row(const double *row, double (&v)[3]) {
    const double2 a = *reinterpret_cast<const double2 *>(row);
    v[0] = a.x; v[1] = a.y; v[2] = row[2];
}

// correspondence i of the pooled set: cameras [0, n_cam), then points.  Returns whether it is on.
struct AlignSrc {
    const double *xc, *yc; const uint8_t *uc; int64_t n_cam;
    const double *xp, *yp; const uint8_t *up;
    C2B_DEV bool get(int64_t i, double (&x)[3], double (&y)[3]) const {
        const bool cam = i < n_cam;
        const int64_t k = cam ? i : i - n_cam;
        align_row((cam ? xc : xp) + 4 * k, x);
        align_row((cam ? yc : yp) + 4 * k, y);
        const uint8_t *m = cam ? uc : up;
        return m ? m[k] != 0 : true;
    }
};

__global__ __launch_bounds__(kAlignBlock) void k_align_means(AlignSrc src, int64_t n, double *__restrict__ block_part,
                                                            unsigned *__restrict__ ticket, double *__restrict__ out) {
    __shared__ double sRed[kAlignMeans * kAlignWaves + 1];
    double a[kAlignMeans];
#pragma unroll
    for (int k = 0; k < kAlignMeans; ++k) a[k] = 0.0;
    const int64_t step = (int64_t)gridDim.x * kAlignBlock;
    for (int64_t i = (int64_t)blockIdx.x * kAlignBlock + threadIdx.x; i < n; i += step * kAlignBatch) {
        double x[kAlignBatch][3], y[kAlignBatch][3];
        bool on[kAlignBatch];
#pragma unroll
        for (int u = 0; u < kAlignBatch; ++u) {              // past the end: the last entity again, not counted
            const int64_t j = i + u * step;
            on[u] = src.get(j < n ? j : n - 1, x[u], y[u]) && j < n;
        }
#pragma unroll
        for (int u = 0; u < kAlignBatch; ++u) {
            a[0] += on[u] ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[1 + k] += on[u] ? x[u][k] : 0.0; a[4 + k] += on[u] ? y[u][k] : 0.0; }
        }
    }
#pragma unroll
    for (int k = 0; k < kAlignMeans; ++k) a[k] = wave_sum(a[k]);
    ticket_fold_n<kAlignMeans>(a, sRed, block_part, ticket, out);
}

// means: what k_align_means left (count, sums).  out[0 .. 16]: the sums (kAlignMoments), out[17 .. 22]: the pivot.
__global__ __launch_bounds__(kAlignBlock) void k_align_moments(AlignSrc src, int64_t n, const double *__restrict__ means,
                                                              double *__restrict__ block_part, unsigned *__restrict__ ticket,
                                                              double *__restrict__ out) {
    __shared__ double sRed[kAlignMoments * kAlignWaves + 1];
    const double cnt = means[0];
    double mx[3], my[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { mx[k] = means[1 + k] / cnt; my[k] = means[4 + k] / cnt; }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { out[kAlignMoments + k] = mx[k]; out[kAlignMoments + 3 + k] = my[k]; }
    }
    double a[kAlignMoments];
#pragma unroll
    for (int k = 0; k < kAlignMoments; ++k) a[k] = 0.0;
    const int64_t step = (int64_t)gridDim.x * kAlignBlock;
    for (int64_t i = (int64_t)blockIdx.x * kAlignBlock + threadIdx.x; i < n; i += step * kAlignBatch) {
        double x[kAlignBatch][3], y[kAlignBatch][3];
        bool on[kAlignBatch];
#pragma unroll
        for (int u = 0; u < kAlignBatch; ++u) {
            const int64_t j = i + u * step;
            on[u] = src.get(j < n ? j : n - 1, x[u], y[u]) && j < n;
        }
#pragma unroll
        for (int u = 0; u < kAlignBatch; ++u) {
            double dx[3], dy[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { dx[k] = on[u] ? x[u][k] - mx[k] : 0.0; dy[k] = on[u] ? y[u][k] - my[k] : 0.0; }
            a[0] += dot3(dx[0], dx[1], dx[2], dx[0], dx[1], dx[2]);
            a[1] += dot3(dy[0], dy[1], dy[2], dy[0], dy[1], dy[2]);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) a[2 + 3 * r + c] += dy[r] * dx[c];
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[11 + k] += dx[k]; a[14 + k] += dy[k]; }
        }
    }
#pragma unroll
    for (int k = 0; k < kAlignMoments; ++k) a[k] = wave_sum(a[k]);
    ticket_fold_n<kAlignMoments>(a, sRed, block_part, ticket, out);
}

// ---- the per-entity errors: what k_align_errors is instantiated over --------------------------------------------------------------
// position: e = |s R x + t - y| over a pair of 32-byte row tables
struct AlignPosErr {
    static constexpr int kBatch = 2;                     // (four per trip, as the fitting passes take, costs this kernel scalar registers it does not have)
    const double *x4, *y4;
    AlignSim T;
    C2B_DEV double operator()(int64_t i) const {
        double x[3], y[3], p[3];
        align_row(x4 + 4 * i, x);
        align_row(y4 + 4 * i, y);
        align_map(T, x, p);
        const double d0 = p[0] - y[0], d1 = p[1] - y[1], d2 = p[2] - y[2];
        return sqrt(dot3(d0, d1, d2, d0, d1, d2));
    }
};
// rotation: theta = 2 asin(min(1, |R_c R^T - R_c^ref|_F / (2 sqrt 2))) over a pair of cam15 tables.  The chord keeps a small angle
// (|D|_F = 2 sqrt 2 sin(theta / 2) exactly), where acos((tr - 1) / 2) loses everything below 1e-8.
struct AlignRotErr {
    static constexpr int kBatch = 2;                     // 2 x 2 x 72 bytes in flight per thread, as many as four row pairs
    const double *x15, *y15;
    AlignSim T;
    C2B_DEV double operator()(int64_t i) const {
        double a[9], b[9], m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { a[k] = x15[15 * i + k]; b[k] = y15[15 * i + k]; }
        cm_mat_mul(a, T.R, m);               // (the row-major array of R is the column-major array of R^T)
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) { const double d = m[k] - b[k]; q += d * d; }
        const double h = sqrt(q) * 0.35355339059327378;           // 1 / (2 sqrt 2)
        return 2.0 * asin(h < 1.0 ? h : 1.0);
    }
};

// err [n] (NULL: not kept): every entity's error, on or off.  base / use (NULL: all on): the caller's mask and the set the summary runs
// over.  next (NULL: not kept): base && e <= max_dist (max_dist <= 0: base).  rec: gridDim.x records of kAlignRec doubles.
// out[0 .. 6]: count, sum e^2, sum e, max (-1: nothing on), argmax (-1), bytes of `next` that differ from `use`, size of `next`.
// A NaN error is never the maximum and never an inlier.
template <typename Err>
__global__ __launch_bounds__(kAlignBlock) void k_align_errors(Err f, int64_t n, const uint8_t *__restrict__ base,
                                                             const uint8_t *__restrict__ use, double max_dist, double *__restrict__ err,
                                                             uint8_t *__restrict__ next, double *__restrict__ rec,
                                                             unsigned *__restrict__ ticket, double *__restrict__ out) {
    __shared__ double sh[kAlignWaves + 1][kAlignRec];
    unsigned magic = 0u;
    if (threadIdx.x == 0) magic = ticket[kTicketMagicAt];
    double cnt = 0.0, se2 = 0.0, se = 0.0, mx = -1.0, arg = -1.0, chg = 0.0, nn = 0.0;
    const int64_t step = (int64_t)gridDim.x * kAlignBlock;
    for (int64_t i = (int64_t)blockIdx.x * kAlignBlock + threadIdx.x; i < n; i += step * Err::kBatch) {
        double e[Err::kBatch];
        bool b[Err::kBatch], on[Err::kBatch];
#pragma unroll
        for (int u = 0; u < Err::kBatch; ++u) {              // past the end: the last entity again, neither stored nor counted
            const int64_t j = i + u * step, jc = j < n ? j : n - 1;
            e[u] = f(jc);
            b[u] = j < n && (base ? base[jc] != 0 : true);
            on[u] = j < n && (use ? use[jc] != 0 : true);
        }
#pragma unroll
        for (int u = 0; u < Err::kBatch; ++u) {
            const int64_t j = i + u * step;
            const bool keep = b[u] && (max_dist > 0.0 ? e[u] <= max_dist : true);
            if (err && j < n) err[j] = e[u];
            if (next && j < n) next[j] = keep ? 1 : 0;
            cnt += on[u] ? 1.0 : 0.0;
            se2 += on[u] ? e[u] * e[u] : 0.0;
            se += on[u] ? e[u] : 0.0;
            const bool better = on[u] && e[u] > mx;              // j grows within a thread: the first to attain it stays
            mx = better ? e[u] : mx;
            arg = better ? (double)j : arg;
            chg += keep != on[u] ? 1.0 : 0.0;
            nn += keep ? 1.0 : 0.0;
        }
    }
    // the workgroup's record: sums by the shuffle tree; the maximum, then the lowest index among the lanes that hold it
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double big = 0x1.0p62;
    auto reduce = [&](double (&s)[5], double &m, double &a) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = wave_sum(s[k]);
        const double wm = __shfl(wave_max(m), 0, 64);
        a = wave_min(m == wm && a >= 0.0 ? a : big);
        m = wm;
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) sh[wave][k] = s[k];
            sh[wave][5] = m; sh[wave][6] = a;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) s[k] = 0.0;
            m = -1.0; a = big;
            for (int w = 0; w < kAlignWaves; ++w) {
#pragma unroll
                for (int k = 0; k < 5; ++k) s[k] += sh[w][k];
                if (sh[w][5] > m || (sh[w][5] == m && sh[w][6] < a)) { m = sh[w][5]; a = sh[w][6]; }
            }
        }
    };
    double s[5] = {cnt, se2, se, chg, nn};
    reduce(s, mx, arg);
    if (threadIdx.x == 0) {
        double *o = rec + (int64_t)blockIdx.x * kAlignRec;
        const double t[kAlignSummary] = {s[0], s[1], s[2], s[3], s[4], mx, arg};
#pragma unroll
        for (int k = 0; k < kAlignSummary; ++k) __hip_atomic_store(o + k, t[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0);
        const bool last = ticket_arrive(ticket, magic);
        if (magic != kTicketMagic) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            for (int k = 0; k < kAlignSummary; ++k) out[k] = nan;
        }
        sh[kAlignWaves][0] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    if (sh[kAlignWaves][0] == 0.0) return;             // workgroup-uniform
    // the last workgroup: thread t takes records t, t + kAlignBlock, ... (one each at the shipped grid)
    double g[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, gm = -1.0, ga = big;
    for (unsigned r = threadIdx.x; r < gridDim.x; r += kAlignBlock) {
        const double *q = rec + (int64_t)r * kAlignRec;
#pragma unroll
        for (int k = 0; k < 5; ++k) g[k] += q[k];
        if (q[5] > gm || (q[5] == gm && q[6] < ga)) { gm = q[5]; ga = q[6]; }
    }
    reduce(g, gm, ga);
    if (threadIdx.x != 0) return;
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];
    out[3] = gm; out[4] = gm >= 0.0 ? ga : -1.0;
    out[5] = g[3]; out[6] = g[4];
}

// ---- a similarity applied in place -------------------------------------------------------------------------------------------------
// the fourth lane of a point's row stays
__global__ __launch_bounds__(kBlock) void k_similarity_apply_points(double *__restrict__ pts4, int64_t n, AlignSim T) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x[3], p[3];
    align_row(pts4 + 4 * i, x);
    align_map(T, x, p);
    *reinterpret_cast<double2 *>(pts4 + 4 * i) = make_double2(p[0], p[1]);
    pts4[4 * i + 2] = p[2];
}

// R_c' = R_c R^T, c' = s R c + t, t_c' = -R_c' c'; f, k1, k2 untouched.  R_c'(X' - c') = s R_c (X - c): every projection stays.
__global__ __launch_bounds__(kBlock) void k_similarity_apply_cameras(double *__restrict__ cam15, int64_t n, AlignSim T) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double c[12], ctr[3], q[3], m[9], v[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = cam15[15 * i + k];
    cm_center(c, c[9], c[10], c[11], ctr);
    align_map(T, ctr, q);
    cm_mat_mul(c, T.R, m);
    cm_mat_vec(m, q[0], q[1], q[2], v);
    double *o = cam15 + 15 * i;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = m[k];
    o[9] = -1.0 * v[0]; o[10] = -1.0 * v[1]; o[11] = -1.0 * v[2];
}

}  // namespace c2b
