// merge_kernels.hpp -- gfx950 kernels of landmark merging (included by capi.hip only, after triangulate_robust_kernels.hpp
// and cell_kernels.hpp).
//
// c2b_merge_partner_rows / c2b_problem_merge_points: two points that are one landmark (split_landmarks, a
// broken track) are found and put back together.  The contract is the header's; the passes:
//   * k_merge_extent: the x / z extent of the finite points for the cell grid.  A double's bits are mapped to an unsigned key of
//     the same order; the wave's minimum and maximum by shuffles, then four 64-bit INTEGER atomics per wave.
//   * k_merge_partner: one wave per point p.
//       candidates   the lanes stride over the entries of the 3 x 3 cells around p's cell (three contiguous ranges of the
//                    cell-sorted list): q takes part, d2(p, q) <= r2, and the key (bits of d2, q) lies above the last key
//                    taken; a lane keeps its smallest, the wave's smallest follows by shuffles.  The order inside a cell
//                    (the arrival order of the cell fill's atomics) does not enter: a minimum over a set.
//       choice       that pair is tested; when it fails the scan repeats above its key.  Every repeat takes one more
//                    candidate, so the loop ends after at most the neighbourhood's population.
//       disjointness the lanes hold the lower row's cameras 64 at a time; the other row's cameras are read one by one at a
//                    wave-uniform address and compared in every lane; a ballot per chunk.
//       verification lanes = the entries of both rows, 64 at a time; each projects m (merge_position) through its own camera
//                    (project_obs) and evaluates the filter's predicate (trc_fits); a ballot per chunk.
//     The four status counts: LDS integer atomics per workgroup, then at most four 64-bit integer atomics per workgroup.
//   * k_merge_apply: one lane per point; the lower point of a mutual pair takes merge_position -- the one expression the
//     partner pass verified -- and into[] says where every point's observations go.
//   * k_merge_remap: one lane per observation, pt_idx[o] = into[pt_idx[o]] (also composes the map over the rounds).
//   * k_merge_held: held = constant under the point mask, or a point prior with a non-zero weight.
// No float atomics, no scratch memory, no LDS beyond the histogram; every loop is bounded by a row length or a cell
// population; no wave waits for another.  A point's partner depends on the state alone, never on the launch shape.
#pragma once
#include "cell_kernels.hpp"
#include "triangulate_robust_kernels.hpp"

namespace c2b {

constexpr int kMrgBlock = 256;
constexpr int kMrgWaves = kMrgBlock / 64;                    // points per workgroup
enum { kMergeNone = 0, kMergeChosen = 1, kMergeUnobserved = 2, kMergeHeld = 3, kMergeKinds = 4 };     // C2B_MERGE_*

// where the pair (a, b), a < b, with rows of na and nb entries goes: a + (b - a) * nb / (na + nb) per coordinate, three
// roundings each (sub, mul, add), the lower index first -- equal bits give a exactly.  The ONE expression of the merged
// position: the partner pass verifies it, the apply pass writes it.
C2B_DEV void merge_position(const double4 A, const double4 B, int na, int nb, double &x, double &y, double &z) {
    const double f = (double)nb / (double)(na + nb);
    x = A.x + (B.x - A.x) * f;
    y = A.y + (B.y - A.y) * f;
    z = A.z + (B.z - A.z) * f;
}

// an unsigned key in the order of the doubles (finite ones; -0 below +0)
C2B_DEV unsigned long long merge_order_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// ext[0..3] = keys of min x, min z, max x, max z over the points whose x and z are finite; on entry ~0, ~0, 0, 0
__global__ __launch_bounds__(256) void k_merge_extent(const double4 *__restrict__ pts4, int64_t n, unsigned long long *__restrict__ ext) {
    unsigned long long lo_x = ~0ull, lo_z = ~0ull, hi_x = 0ull, hi_z = 0ull;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const double4 p = pts4[j];
        if (!(fabs(p.x) <= 1.79769313486231570815e308 && fabs(p.z) <= 1.79769313486231570815e308)) continue;      // NaN, infinite: in no pair
        const unsigned long long kx = merge_order_key(p.x), kz = merge_order_key(p.z);
        lo_x = kx < lo_x ? kx : lo_x; hi_x = kx > hi_x ? kx : hi_x;
        lo_z = kz < lo_z ? kz : lo_z; hi_z = kz > hi_z ? kz : hi_z;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long a = __shfl_xor(lo_x, d, 64), b = __shfl_xor(lo_z, d, 64), c = __shfl_xor(hi_x, d, 64), e = __shfl_xor(hi_z, d, 64);
        lo_x = a < lo_x ? a : lo_x; lo_z = b < lo_z ? b : lo_z;
        hi_x = c > hi_x ? c : hi_x; hi_z = e > hi_z ? e : hi_z;
    }
    if ((threadIdx.x & 63) == 0 && hi_x != 0ull) {           // (a wave without a finite point adds nothing)
        atomicMin(ext + 0, lo_x); atomicMin(ext + 1, lo_z);
        atomicMax(ext + 2, hi_x); atomicMax(ext + 3, hi_z);
    }
}

// held[p] = 1: the point takes no part (constant, or tied to a prior target).  pmask / pxw may be NULL.
__global__ __launch_bounds__(256) void k_merge_held(int64_t n_pts, const uint8_t *__restrict__ pmask, const double *__restrict__ pxw,
                                                   uint8_t *__restrict__ held) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pts) return;
    bool h = pmask && pmask[p];
    if (pxw) h = h || pxw[3 * p] != 0.0 || pxw[3 * p + 1] != 0.0 || pxw[3 * p + 2] != 0.0;
    held[p] = h ? 1 : 0;
}

// Is the pair (p, q) verified?  Every lane returns the same answer.
C2B_DEV bool merge_pair_verified(const int lane, const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint32_t p,
                                 const uint32_t q, const uint64_t *__restrict__ pt_row_ptr, const uint32_t *__restrict__ obs_of,
                                 const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs, const double max_err2) {
    const uint32_t a = p < q ? p : q, b = p < q ? q : p;
    const uint64_t ab = pt_row_ptr[a], bb = pt_row_ptr[b];
    const int na = (int)(pt_row_ptr[a + 1] - ab), nb = (int)(pt_row_ptr[b + 1] - bb);     // (the launcher holds n_obs below 2^31 - 64)
    // ---- (i) no camera in both rows ----
#pragma unroll 1
    for (int t0 = 0; t0 < na; t0 += 64) {
        const bool valid = t0 + lane < na;
        const uint32_t ca = valid ? cam_of[ab + (uint64_t)(t0 + lane)] : 0u;
        bool shared = false;
#pragma unroll 1
        for (int s = 0; s < nb; ++s) {                       // wave-uniform address
            const uint32_t cb = cam_of[bb + (uint64_t)s];
            shared = shared || (valid && ca == cb);
        }
        if (__ballot(shared) != 0ull) return false;
    }
    // ---- (ii) every entry of both rows fits at the merged position ----
    double mx, my, mz;
    merge_position(pts4[a], pts4[b], na, nb, mx, my, mz);
    const int n = na + nb;
#pragma unroll 1
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        bool bad = false;
        if (t < n) {
            const uint64_t j = t < na ? ab + (uint64_t)t : bb + (uint64_t)(t - na);
            bad = !trc_fits(cam_ref(camblk, cam_of[j]), uv_obs[obs_of[j]], mx, my, mz, max_err2);
        }
        if (__ballot(bad) != 0ull) return false;
    }
    return true;
}

// One point by the wave that calls it (it takes part: not held, observed); every lane returns the same partner, -1 for none.
C2B_DEV int merge_choose_partner(const int lane, const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint32_t p,
                                 const uint64_t *__restrict__ pt_row_ptr, const uint32_t *__restrict__ obs_of,
                                 const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs, const CellGrid g,
                                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ sorted, const double r2,
                                 const double max_err2, const uint8_t *__restrict__ held) {
    const double4 P = pts4[p];
    const int ccx = cell_coord(P.x, g.x0, g.inv_cs, g.ncx), ccz = cell_coord(P.z, g.z0, g.inv_cs, g.ncz);
    const int ix0 = ccx > 0 ? ccx - 1 : 0, ix1 = ccx + 1 < g.ncx ? ccx + 1 : g.ncx - 1;
    const int iz0 = ccz > 0 ? ccz - 1 : 0, iz1 = ccz + 1 < g.ncz ? ccz + 1 : g.ncz - 1;
    unsigned long long last_d = 0ull;
    uint32_t last_q = 0u;
    bool have_last = false;
#pragma unroll 1
    for (;;) {                                               // every pass takes one more candidate of a finite set
        unsigned long long best_d = ~0ull;
        uint32_t best_q = 0xffffffffu;
#pragma unroll 1
        for (int ix = ix0; ix <= ix1; ++ix) {
            const uint32_t b = start[ix * g.ncz + iz0], e = start[ix * g.ncz + iz1 + 1];      // three cells, one range
#pragma unroll 1
            for (uint32_t k = b + (uint32_t)lane; k < e; k += 64u) {
                const uint32_t q = sorted[k];
                if (q == p || (held && held[q]) || pt_row_ptr[q] == pt_row_ptr[q + 1]) continue;      // itself, held, unobserved
                const double4 Q = pts4[q];
                const double dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 <= r2)) continue;                   // (a NaN is in no pair)
                const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);          // d2 >= 0: its bits order it
                if (have_last && !(bits > last_d || (bits == last_d && q > last_q))) continue;
                if (bits < best_d || (bits == best_d && q < best_q)) { best_d = bits; best_q = q; }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long od = __shfl_xor(best_d, d, 64);
            const uint32_t oq = (uint32_t)__shfl_xor((int)best_q, d, 64);
            if (od < best_d || (od == best_d && oq < best_q)) { best_d = od; best_q = oq; }
        }
        const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)best_q);
        if (q == 0xffffffffu) return -1;                     // (n_pts < 2^31: no point has this index)
        if (merge_pair_verified(lane, camblk, pts4, p, q, pt_row_ptr, obs_of, cam_of, uv_obs, max_err2)) return (int)q;
        last_d = best_d; last_q = q; have_last = true;
    }
}

// held == NULL: no point is held.  counts[kMergeKinds] must be zero when the kernel starts.
__global__ __launch_bounds__(kMrgBlock) void k_merge_partner(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
    const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs, CellGrid g,
    const uint32_t *__restrict__ start, const uint32_t *__restrict__ sorted, double r2, double max_err2,
    const uint8_t *__restrict__ held, int32_t *__restrict__ partner, uint8_t *__restrict__ status,
    unsigned long long *__restrict__ counts) {
    __shared__ unsigned sCnt[kMergeKinds];
    if (threadIdx.x < kMergeKinds) sCnt[threadIdx.x] = 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kMrgWaves + wave;
    if (p < n_pts) {                                         // wave-uniform
        int st, q = -1;
        if (held && held[p]) {
            st = kMergeHeld;
        } else if (pt_row_ptr[p] == pt_row_ptr[p + 1]) {
            st = kMergeUnobserved;
        } else {
            q = merge_choose_partner(lane, camblk, pts4, (uint32_t)p, pt_row_ptr, obs_of, cam_of, uv_obs, g, start, sorted, r2, max_err2, held);
            st = q >= 0 ? kMergeChosen : kMergeNone;
        }
        if (lane == 0) {
            partner[p] = q;
            status[p] = (uint8_t)st;
            atomicAdd(&sCnt[st], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kMergeKinds && sCnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)sCnt[threadIdx.x]);
}

// The mutual pairs merged: the lower point moves to merge_position, into[p] = where p's observations go (p itself unless
// it is the upper point of a mutual pair); *n_merged counts the upper points (zero on entry).  A lane writes its own
// point alone and reads only its partner's, which no lane writes: the upper point of a pair is the lower point of none.
__global__ __launch_bounds__(256) void k_merge_apply(double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
                                                    const int32_t *__restrict__ partner, uint32_t *__restrict__ into,
                                                    unsigned long long *__restrict__ n_merged) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pts) return;
    const int32_t q = partner[p];
    uint32_t dst = (uint32_t)p;
    if (q >= 0 && (int64_t)partner[q] == p) {
        if (p < (int64_t)q) {
            const double4 A = pts4[p], B = pts4[q];
            double x, y, z;
            merge_position(A, B, (int)(pt_row_ptr[p + 1] - pt_row_ptr[p]), (int)(pt_row_ptr[q + 1] - pt_row_ptr[q]), x, y, z);
            double2 *out = reinterpret_cast<double2 *>(pts4 + p);          // x y | z w: the fourth lane keeps its value
            out[0] = make_double2(x, y);
            reinterpret_cast<double *>(out + 1)[0] = z;
        } else {
            dst = (uint32_t)q;
            atomicAdd(n_merged, 1ull);
        }
    }
    into[p] = dst;
}

// idx[o] = into[idx[o]]: the list's point indices after a round, and the composed map of the rounds
__global__ __launch_bounds__(256) void k_merge_remap(uint32_t *__restrict__ idx, int64_t n, const uint32_t *__restrict__ into) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o < n) idx[o] = into[idx[o]];
}

}  // namespace c2b
