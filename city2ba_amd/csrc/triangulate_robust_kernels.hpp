// triangulate_robust_kernels.hpp -- gfx950 kernel of consensus triangulation (included by capi.hip only, after
// triangulate_kernels.hpp).
//
// c2b_triangulate_consensus_rows / c2b_problem_triangulate_consensus: k_triangulate_points' midpoint over the
// rays that agree with each other, for a point whose row also holds rays of other points (wrong matches).
//   * k_triangulate_consensus: point-major through the transpose, one wave per point, the row walked 64 entries at a time.
//       sample    lanes = the row's first 64 entries: tri_ray, a ballot, the usable rays and centres compacted in row order
//                 into wave-private LDS (48 B x 64);
//       hypothesis lanes = pairs of the sample, wide gaps first (trc_pair): X_k from tri_add over the two rays, formed
//                 when tri_solve accepts it;
//       score     the row again chunk by chunk: the lanes find the usable entries (tri_ray, ballot), then for every set bit
//                 every lane projects ITS X_k through the SAME camera and pixel -- wave-uniform addresses, so the k2 != 0
//                 route of project_obs is a wave-uniform branch -- and counts the filter's predicate (MODE_RESIDUAL_KEEP with
//                 C2B_FILTER_IN_FRONT) in an integer;
//       select    the wave's maximum of (count, -k); its X is broadcast;
//       refit     lanes = entries again: the winner's inliers by the same predicate, a ballot, the rays staged in LDS and
//                 summed by every lane in ascending row order (the same sums in every lane: no cross-lane reduction), the
//                 parallax test and the Cholesky;
//       cheirality and mask: one more walk, q.z < 0 for the refit X in every inlier's camera; the zeros of the inlier mask
//                 are written here and taken back by a last walk if a camera turns out to see X from behind.
//     The nine-accumulator update, the acceptance test and the solve are k_triangulate_points' own routines (tri_add,
//     tri_solve): the refit is bit for bit k_triangulate_points on the inliers.
//   * the six status counts: LDS integer atomics per workgroup, then at most six 64-bit integer atomics per workgroup.
// Every loop is bounded by the row length, the 16 Newton steps or 64; no wave waits for another.  No float atomics, no
// scratch memory, no robust loss, nothing stored per row: a point's result depends on its own row alone.
#pragma once
#include "triangulate_kernels.hpp"

namespace c2b {

constexpr int kTrcBlock = 256;
constexpr int kTrcWaves = kTrcBlock / 64;                    // points per workgroup
constexpr int kTrcSample = 64;                               // the sample window and the most hypotheses: one per lane
enum { kTriNoConsensus = 5, kTrcKinds = 6 };                 // C2B_TRI_NO_CONSENSUS; the statuses of the consensus pass

struct TrcLds { double f[6][64]; };                          // one wave's: field-major d.x d.y d.z C.x C.y C.z

C2B_DEV void trc_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Pair number k of a sample of m >= 2: the gap g runs from m / 2 down to 1, i over 0 .. m - 1 (2 g == m: i < g only, each
// pair once), the pair is (i, (i + g) mod m), lower index first.  false when k >= m (m - 1) / 2.
C2B_DEV bool trc_pair(int k, int m, int &lo, int &hi) {
    const int half = m >> 1;
    int g, i;
    if (!(m & 1) && k < half) {
        g = half; i = k;
    } else {
        const int r = (m & 1) ? k : k - half;
        g = ((m & 1) ? half : half - 1) - r / m;
        i = r % m;
    }
    if (g < 1) { lo = 0; hi = 0; return false; }
    int j = i + g;
    if (j >= m) j -= m;
    lo = i < j ? i : j; hi = i < j ? j : i;
    return true;
}

// the filter's predicate (MODE_RESIDUAL_KEEP with C2B_FILTER_IN_FRONT) of X in camera `cam` against the observed pixel
template <typename P>
C2B_DEV bool trc_fits(P cam, const double2 ob, double x0, double x1, double x2, double max_err2) {
    const Proj p = project_obs(cam, x0, x1, x2);
    const double du = p.u - ob.x, dv = p.v - ob.y;
    const double r2 = du * du + dv * dv;
    return r2 <= max_err2 && p.qz < 0.0;
}

// One point by the wave that calls it; every lane returns the same status.  hyp_out / n_inl_out: the selected hypothesis
// and its inlier count (-1 / 0 when none was selected).  [b, e) is the point's row of the transpose.
C2B_DEV int triangulate_consensus_point(TrcLds &W, const int lane, const double *__restrict__ camblk, double4 *__restrict__ pt,
                                        const uint64_t b, const uint64_t e, const uint32_t *__restrict__ obs_of,
                                        const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs,
                                        const double one_minus_cos, const double max_err2, const int min_inliers,
                                        const int max_hypotheses, uint8_t *__restrict__ inlier, int &hyp_out, int &n_inl_out) {
    hyp_out = -1;
    n_inl_out = 0;
    const int n = (int)(e - b);                              // (the launcher holds n_obs below 2^31 - 64)
    // ---- the sample: the usable entries among the row's first 64, compacted in row order ----
    uint64_t use0;
    {
        const uint64_t j = b + (uint64_t)lane;
        double dx = 0.0, dy = 0.0, dz = 0.0;
        bool use = false;
        uint32_t c = 0u;
        if (lane < n) {
            c = cam_of[j];
            use = tri_ray(cam_ref(camblk, c), uv_obs[obs_of[j]], dx, dy, dz);
        }
        use0 = __ballot(use);
        if (use) {
            const int slot = __popcll(use0 & ((1ull << lane) - 1ull));
            const double *C = camblk + cam_center_at((int64_t)c);
            W.f[0][slot] = dx; W.f[1][slot] = dy; W.f[2][slot] = dz;
            W.f[3][slot] = C[0]; W.f[4][slot] = C[1]; W.f[5][slot] = C[2];
        }
    }
    const int m = __popcll(use0);
    if (m < 2) return kTriTooFew;                            // (n_used >= m: with m >= 2 the whole row has two usable entries too)
    trc_sync();
    // ---- hypotheses: lane k forms X_k from pair k ----
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    bool formed = false;
    {
        int lo, hi;
        if (trc_pair(lane, m, lo, hi) && lane < max_hypotheses) {
            TriSums s;
            tri_add(s, W.f[0][lo], W.f[1][lo], W.f[2][lo], W.f[3][lo], W.f[4][lo], W.f[5][lo]);
            tri_add(s, W.f[0][hi], W.f[1][hi], W.f[2][hi], W.f[3][hi], W.f[4][hi], W.f[5][hi]);
            formed = tri_solve(s, 2, one_minus_cos, x0, x1, x2);
        }
        if (!formed) { x0 = 0.0; x1 = 0.0; x2 = 0.0; }
    }
    if (__ballot(formed) == 0ull) return kTriDegenerate;
    // ---- score: every usable entry of the row against every lane's X_k ----
    int score = 0;
#pragma unroll 1
    for (int t0 = 0; t0 < n; t0 += 64) {
        uint64_t use_mask = use0;
        if (t0 != 0) {
            double dx, dy, dz;
            bool use = false;
            if (t0 + lane < n) {
                const uint64_t j = b + (uint64_t)(t0 + lane);
                use = tri_ray(cam_ref(camblk, cam_of[j]), uv_obs[obs_of[j]], dx, dy, dz);
            }
            use_mask = __ballot(use);
        }
#pragma unroll 1
        while (use_mask != 0ull) {                           // wave-uniform
            const uint64_t j = b + (uint64_t)(t0 + __builtin_ctzll(use_mask));
            use_mask &= use_mask - 1ull;
            // the same camera and pixel in every lane, but held in vector registers: as scalars the record's 30 registers
            // and the pow route's constants do not fit the scalar file (the hardware serves the one address once)
            uint32_t c = cam_of[j], o = obs_of[j];
            asm volatile("" : "+v"(c), "+v"(o));
            score += trc_fits(cam_ref(camblk, c), uv_obs[o], x0, x1, x2, max_err2) ? 1 : 0;
        }
    }
    // ---- select: the highest score, the lowest k among equals ----
    long long key = formed ? (long long)score * 64 + (63 - lane) : -1ll;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long other = __shfl_xor(key, d, 64);
        key = other > key ? other : key;
    }
    const int win = 63 - (int)(key & 63ll);
    const int n_inl = (int)(key >> 6);
    hyp_out = win;
    n_inl_out = n_inl;
    if (n_inl < min_inliers) return kTriNoConsensus;
    x0 = __shfl(x0, win, 64); x1 = __shfl(x1, win, 64); x2 = __shfl(x2, win, 64);
    trc_sync();                                              // the sample's slots are staged over below
    // ---- refit: the winner's inliers in ascending row order ----
    TriSums s;
#pragma unroll 1
    for (int t0 = 0; t0 < n; t0 += 64) {
        const uint64_t j = b + (uint64_t)(t0 + lane);
        bool in = false;
        if (t0 + lane < n) {
            const uint32_t c = cam_of[j];
            const CamRef cam = cam_ref(camblk, c);
            const double2 ob = uv_obs[obs_of[j]];
            double dx, dy, dz;
            if (tri_ray(cam, ob, dx, dy, dz) && trc_fits(cam, ob, x0, x1, x2, max_err2)) {
                in = true;
                const double *C = camblk + cam_center_at((int64_t)c);
                W.f[0][lane] = dx; W.f[1][lane] = dy; W.f[2][lane] = dz;
                W.f[3][lane] = C[0]; W.f[4][lane] = C[1]; W.f[5][lane] = C[2];
            }
        }
        uint64_t in_mask = __ballot(in);
        trc_sync();
#pragma unroll 1
        while (in_mask != 0ull) {                            // wave-uniform: every lane forms the same sums
            const int t = __builtin_ctzll(in_mask);
            in_mask &= in_mask - 1ull;
            tri_add(s, W.f[0][t], W.f[1][t], W.f[2][t], W.f[3][t], W.f[4][t], W.f[5][t]);
        }
        trc_sync();
    }
    double r0, r1, r2;
    if (!tri_solve(s, n_inl, one_minus_cos, r0, r1, r2)) return kTriDegenerate;
    // ---- cheirality of the refit in every inlier's camera; the mask's zeros ----
    bool behind = false;
#pragma unroll 1
    for (int t0 = 0; t0 < n; t0 += 64) {
        if (t0 + lane < n) {
            const uint64_t j = b + (uint64_t)(t0 + lane);
            const CamRef cam = cam_ref(camblk, cam_of[j]);
            const uint32_t o = obs_of[j];
            const double2 ob = uv_obs[o];
            double dx, dy, dz;
            const bool in = tri_ray(cam, ob, dx, dy, dz) && trc_fits(cam, ob, x0, x1, x2, max_err2);
            if (in) {
                const double qz = dot3(cam[6], cam[7], cam[8], r0, r1, r2) + cam[11];
                if (qz >= 0.0) behind = true;
            } else if (inlier) {
                inlier[o] = 0;
            }
        }
    }
    if (__ballot(behind) != 0ull) {
        if (inlier) {                                        // nothing is claimed about a point that was not triangulated
#pragma unroll 1
            for (int t = lane; t < n; t += 64) inlier[obs_of[b + (uint64_t)t]] = 1;        // (the lane that wrote the zero)
        }
        return kTriBehind;
    }
    if (lane == 0) {
        double2 *out = reinterpret_cast<double2 *>(pt);      // x y | z w: the fourth lane keeps its value
        out[0] = make_double2(r0, r1);
        reinterpret_cast<double *>(out + 1)[0] = r2;
    }
    return kTriOk;
}

// pt_mask == NULL: no point is constant; hyp, n_inl, inlier may be NULL.  counts[kTrcKinds] must be zero and inlier all
// ones when the kernel starts.
__global__ __launch_bounds__(kTrcBlock) void k_triangulate_consensus(
    const double *__restrict__ camblk, double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
    const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs,
    double one_minus_cos, double max_err2, int min_inliers, int max_hypotheses, const uint8_t *__restrict__ pt_mask,
    uint8_t *__restrict__ status, int32_t *__restrict__ hyp, int32_t *__restrict__ n_inl, uint8_t *__restrict__ inlier,
    unsigned long long *__restrict__ counts) {
    __shared__ TrcLds sW[kTrcWaves];
    __shared__ unsigned sCnt[kTrcKinds];
    if (threadIdx.x < kTrcKinds) sCnt[threadIdx.x] = 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;     // (the row's bounds are scalars then)
    const int64_t p = (int64_t)blockIdx.x * kTrcWaves + wave;
    if (p < n_pts) {                                         // wave-uniform
        int st = kTriConstant, h = -1, n = 0;
        if (!pt_mask || !pt_mask[p])
            st = triangulate_consensus_point(sW[wave], lane, camblk, pts4 + p, pt_row_ptr[p], pt_row_ptr[p + 1], obs_of, cam_of, uv_obs,
                                             one_minus_cos, max_err2, min_inliers, max_hypotheses, inlier, h, n);
        if (lane == 0) {
            status[p] = (uint8_t)st;
            if (hyp) hyp[p] = h;
            if (n_inl) n_inl[p] = n;
            atomicAdd(&sCnt[st], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kTrcKinds && sCnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)sCnt[threadIdx.x]);
}

}  // namespace c2b
