// rematch_kernels.hpp -- gfx950 kernels of guided re-matching (included by capi.hip only, after merge_kernels.hpp).
//
// c2b_rematch_rows / c2b_problem_rematch_observations: an observation whose pixel is right and whose point
// index is wrong (add_incorrect_correspondences swaps two labels of a camera, join_landmarks hands out a neighbour's) is
// given the label it fits instead of being dropped.  THE CONTRACT (tests/_rematchref.py restates it, the tests compare with ==):
//   E2 = max_error * max_error and R2 = radius * radius, each formed once on the host in double.
//   fit(o, q)   the filter's predicate with C2B_FILTER_IN_FRONT of point q through o's camera against o's pixel:
//               r2(o, q) = du * du + dv * dv <= E2 && q.z < 0 (project_obs: five unfused operations after the projection, libm's
//               pow when k2 != 0; a NaN fails).
//   1 fits      fits[o] = fit(o, pt_idx[o]): the byte c2b_residual_keep_rows writes with C2B_FILTER_IN_FRONT.
//   2 trusted   trusted[p] = x, y, z finite && nfit[p] >= min_fits, nfit[p] = the fitting observations of p (k_rematch_trusted).
//   3 classes   observation o of camera c with label p: FITS (0) if fits[o]; else SKIPPED (1) if !trusted[p]; else FAILING.
//               FITS and SKIPPED observations stay as they are; their labels are HELD in c.
//   4 candidates of a failing o: every q with trusted[q], q != p, q not held in c, fit(o, q), and
//               d2(p, q) = (dx * dx + dy * dy) + dz * dz <= R2                                   (a neighbour: the join case)
//               or q is the label of a failing observation of c                                  (the swap case, at any radius).
//   5 choice    choice[o] = the candidate with the smallest key (bits of r2(o, q), q); -1 when there is none.
//   6 conflicts among the failing observations of c with one choice the smallest (bits of r2, o) is REASSIGNED (2); the
//               others, and those without a choice, are REMOVED (3).  A loser is not offered its second candidate.
//   7 apply     pt_idx[o] = choice[o] where REASSIGNED; keep[o] = status != REMOVED, compacted as the filter compacts.
//   8 counts    counts[4] = the histogram of the statuses, by integer atomics.
//   9           cameras are independent; nothing depends on the launch shape, the cell grid or the order of the cell fill.
// The passes:
//   * k_rematch_trusted: one lane per point: the sum of fits[obs_of[j]] over its row of the transpose, and the finite test.
//   * k_rematch_choose: one wave per camera, its row walked 64 entries at a time: the class of every entry (fits, a byte
//     gather of trusted), a ballot of the failing ones, and for every set bit -- a wave-uniform loop --
//       candidates  the lanes stride over the three contiguous ranges of the cell-sorted list that are the 3 x 3 cells around p
//                   (merge_choose_partner's pattern; trusted, q != p and d2 <= R2 before anything is projected) and then
//                   over the row's own failing labels; every lane projects ITS candidate through the SAME camera record
//                   and pixel (the same addresses in every lane: the k2 != 0 route does not diverge);
//       held        a candidate that fits and would be the lane's best is looked up among the row's fitting entries (a
//                   candidate is trusted, so an entry that names it stays exactly when it fits) and passed over when held:
//                   the filter of rule 4 itself, so no scan is ever repeated;
//       choice      a lane keeps its smallest key, the wave's smallest follows by shuffles -- a minimum over a set, so
//                   neither the order inside a cell nor a candidate met twice enters.
//     Whatever is the same in every lane but lives through the loops -- the camera's index, the label, the pixel, the row's
//     base and the arguments the loops use -- is held in vector registers: as scalars they overflow the scalar file next
//     to the pow route's constants (DESIGN 4.11 met the same; tests/test_isa_pins.py allows no scalar spill).
//     The lane of the entry keeps (choice, bits of r2) and writes them, with the class, after the chunk's loop.
//   * k_rematch_resolve: one wave per camera: rule 6, the lanes' claims against every entry of the row read at a wave-uniform
//     address; the four counts by ballots into LDS integer atomics, then at most four 64-bit integer atomics per
//     workgroup.  A launch of its own: no wave relies on seeing its own earlier global writes.
//   * k_rematch_apply: one lane per observation: the new label and the keep byte.
// No float atomics, no scratch memory, no LDS beyond the histogram; every loop is bounded by a row length, a cell
// population or the number of failing entries of a row; no wave waits for another.
#pragma once
#include "merge_kernels.hpp"

namespace c2b {

constexpr int kRmtBlock = 256;
constexpr int kRmtWaves = kRmtBlock / 64;                    // cameras per workgroup
enum { kRematchFits = 0, kRematchSkipped = 1, kRematchReassigned = 2, kRematchRemoved = 3, kRematchKinds = 4 };      // C2B_REMATCH_*
constexpr unsigned long long kRmtNoKey = ~0ull;              // above every r2's bits (r2 >= 0, not a NaN)

// fit(o, q) and r2(o, q): trc_fits with the sum handed out as well
template <typename P>
C2B_DEV bool rematch_fit(P cam, const double2 ob, const double4 Q, const double max_err2, double &r2) {
    const Proj p = project_obs(cam, Q.x, Q.y, Q.z);
    const double du = p.u - ob.x, dv = p.v - ob.y;
    r2 = du * du + dv * dv;
    return r2 <= max_err2 && p.qz < 0.0;
}

// A kernel argument's pointer moved into vector registers (the compiler no longer knows that every lane holds the same one);
// it goes through an integer and comes back as a pointer into global memory, so its loads and stores stay global_*.
template <typename T>
C2B_DEV T *rematch_in_vgprs(T *p) {
    unsigned long long u = reinterpret_cast<unsigned long long>(p);
    asm volatile("" : "+v"(u));
    return (T *)reinterpret_cast<__attribute__((address_space(1))) T *>(u);
}

// rule 2.  pt_row_ptr == NULL: every finite point is trusted (min_fits = 0).
__global__ __launch_bounds__(256) void k_rematch_trusted(const double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
                                                        const uint32_t *__restrict__ obs_of, const uint8_t *__restrict__ fits, int min_fits,
                                                        uint8_t *__restrict__ trusted) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pts) return;
    const double4 P = pts4[p];
    const double big = 1.79769313486231570815e308;
    bool ok = fabs(P.x) <= big && fabs(P.y) <= big && fabs(P.z) <= big;
    if (ok && pt_row_ptr && min_fits > 0) {
        const uint64_t b = pt_row_ptr[p], e = pt_row_ptr[p + 1];
        int n = 0;                                           // the whole row, no early exit: the count leaves the loop in a register
        for (uint64_t j = b; j < e; ++j) n += fits[obs_of[j]] ? 1 : 0;
        ok = n >= min_fits;
    }
    trusted[p] = ok ? 1 : 0;
}

// One failing observation (label p, pixel ob) of the camera whose row is [b, b + n), by the wave that calls it; every lane
// returns the same choice (-1: none) and the same bits of its r2.
C2B_DEV int rematch_choose_one(const int lane, const CamRef cam, const double4 *__restrict__ pts4, const uint32_t p, const double2 ob,
                               const uint64_t b, const int n, const uint32_t *__restrict__ pt_idx, const uint8_t *__restrict__ fits,
                               const uint8_t *__restrict__ trusted, const CellGrid g, const uint32_t *__restrict__ start,
                               const uint32_t *__restrict__ sorted, const double r2lim, const double max_err2, unsigned long long &bits_out) {
    const double4 P = pts4[p];                               // (p arrives in a vector register; the cell is wave-uniform again)
    const int ccx = __builtin_amdgcn_readfirstlane(cell_coord(P.x, g.x0, g.inv_cs, g.ncx));
    const int ccz = __builtin_amdgcn_readfirstlane(cell_coord(P.z, g.z0, g.inv_cs, g.ncz));
    const int ix0 = ccx > 0 ? ccx - 1 : 0, ix1 = ccx + 1 < g.ncx ? ccx + 1 : g.ncx - 1;
    const int iz0 = ccz > 0 ? ccz - 1 : 0, iz1 = ccz + 1 < g.ncz ? ccz + 1 : g.ncz - 1;
    unsigned long long best_r = kRmtNoKey;
    uint32_t best_q = 0xffffffffu;
    // the segments: the columns ix0 .. ix1 of the cell list (three cells, one range), then -- ix == ix1 + 1 -- the row itself
#pragma unroll 1
    for (int ix = ix0; ix <= ix1 + 1; ++ix) {
        const bool row = ix > ix1;
        const uint32_t *__restrict__ src = row ? pt_idx + b : sorted;
        const uint32_t kb = row ? 0u : start[ix * g.ncz + iz0], ke = row ? (uint32_t)n : start[ix * g.ncz + iz1 + 1];
#pragma unroll 1
        for (uint32_t k = kb + (uint32_t)lane; k < ke; k += 64u) {
            const uint32_t q = src[k];
            if (q == p || !trusted[q]) continue;             // itself; a point too few observations agree on (also: not failing)
            if (row && fits[b + k]) continue;                // a label that stays is not given up
            const double4 Q = pts4[q];
            if (!row) {
                const double dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 <= r2lim)) continue;                // (a NaN is nobody's neighbour)
            }
            double r2;
            if (!rematch_fit(cam, ob, Q, max_err2, r2)) continue;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(r2);              // r2 >= 0: its bits order it
            if (!(bits < best_r || (bits == best_r && q < best_q))) continue;
            // held?  q is trusted, so an entry of the row that names it stays exactly when it fits.  Only a candidate that
            // fits and would be the lane's best gets here; the count leaves the loop in a register, no early exit
            int held = 0;
#pragma unroll 1
            for (int s = 0; s < n; ++s) held |= (pt_idx[b + (uint64_t)s] == q && fits[b + (uint64_t)s]) ? 1 : 0;
            if (held) continue;
            best_r = bits; best_q = q;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long orr = __shfl_xor(best_r, d, 64);
        const uint32_t oq = (uint32_t)__shfl_xor((int)best_q, d, 64);
        if (orr < best_r || (orr == best_r && oq < best_q)) { best_r = orr; best_q = oq; }
    }
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)best_q);
    bits_out = best_r;                                       // (kRmtNoKey without a candidate)
    return q == 0xffffffffu ? -1 : (int)q;                   // (n_pts < 2^31: no point has this index)
}

// choice [n_obs], r2bits [n_obs] (the key of rule 6; kRmtNoKey without a choice) and the class in status [n_obs]: FITS,
// SKIPPED, and REMOVED for every failing entry until k_rematch_resolve has decided.
__global__ __launch_bounds__(kRmtBlock) void k_rematch_choose(
    const double *__restrict__ camblk, const double4 *__restrict__ pts4, const uint64_t *__restrict__ row_ptr, int64_t n_cam,
    const uint32_t *__restrict__ pt_idx, const double2 *__restrict__ uv_obs, const uint8_t *__restrict__ fits,
    const uint8_t *__restrict__ trusted, CellGrid g, const uint32_t *__restrict__ start, const uint32_t *__restrict__ sorted, double r2lim,
    double max_err2, int32_t *__restrict__ choice, unsigned long long *__restrict__ r2bits, uint8_t *__restrict__ status) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kRmtWaves + wave;
    if (c >= n_cam) return;                                  // wave-uniform; the kernel has no barrier
    uint64_t b = row_ptr[c];
    const int n = (int)(row_ptr[c + 1] - b);                 // (the launcher holds n_obs below 2^31 - 64)
    // the same camera in every lane, but its index held in a vector register: as scalars the record's 30 registers, next to the
    // pow route's constants, the grid and the row's bounds, do not fit the scalar file (the hardware serves the
    // one address once)
    uint32_t cv = (uint32_t)c;
    asm volatile("" : "+v"(cv));
    const CamRef cam = cam_ref(camblk, cv);
    // and so are the row's base and the arguments the loops below use: sixteen arguments are 38 scalar registers before
    // anything is computed
    pts4 = rematch_in_vgprs(pts4); pt_idx = rematch_in_vgprs(pt_idx); uv_obs = rematch_in_vgprs(uv_obs);
    fits = rematch_in_vgprs(fits); trusted = rematch_in_vgprs(trusted);
    start = rematch_in_vgprs(start); sorted = rematch_in_vgprs(sorted);
    choice = rematch_in_vgprs(choice); r2bits = rematch_in_vgprs(r2bits); status = rematch_in_vgprs(status);
    asm volatile("" : "+v"(r2lim), "+v"(max_err2), "+v"(g.x0), "+v"(g.z0), "+v"(g.inv_cs), "+v"(b));
#pragma unroll 1
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < n;
        const uint32_t lab = valid ? pt_idx[b + (uint64_t)t] : 0u;
        const bool fit = valid && fits[b + (uint64_t)t] != 0;
        const bool failing = valid && !fit && trusted[lab] != 0;
        int my_choice = -1;
        unsigned long long my_bits = kRmtNoKey;
        unsigned long long todo = __ballot(failing);
#pragma unroll 1
        while (todo) {                                       // wave-uniform
            const int k = (int)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            uint32_t p = (uint32_t)__shfl((int)lab, k, 64), at = (uint32_t)(t0 + k);         // the label and the pixel likewise
            asm volatile("" : "+v"(p), "+v"(at));
            const double2 ob = uv_obs[b + (uint64_t)at];
            unsigned long long bits;
            const int q = rematch_choose_one(lane, cam, pts4, p, ob, b, n, pt_idx, fits, trusted, g, start, sorted, r2lim, max_err2, bits);
            if (lane == k) { my_choice = q; my_bits = bits; }
        }
        if (valid) {
            choice[b + (uint64_t)t] = my_choice;
            r2bits[b + (uint64_t)t] = my_bits;
            status[b + (uint64_t)t] = (uint8_t)(fit ? kRematchFits : (failing ? kRematchRemoved : kRematchSkipped));
        }
    }
}

// Rule 6 and the counts.  counts[kRematchKinds] must be zero when the kernel starts.
__global__ __launch_bounds__(kRmtBlock) void k_rematch_resolve(const uint64_t *__restrict__ row_ptr, int64_t n_cam,
                                                              const int32_t *__restrict__ choice, const unsigned long long *__restrict__ r2bits,
                                                              uint8_t *__restrict__ status, unsigned long long *__restrict__ counts) {
    __shared__ unsigned sCnt[kRematchKinds];
    if (threadIdx.x < kRematchKinds) sCnt[threadIdx.x] = 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kRmtWaves + wave;
    if (c < n_cam) {                                         // wave-uniform
        const uint64_t b = row_ptr[c];
        const int n = (int)(row_ptr[c + 1] - b);
#pragma unroll 1
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int t = t0 + lane;
            const bool valid = t < n;
            const int mine = valid ? choice[b + (uint64_t)t] : -1;
            const unsigned long long mb = valid ? r2bits[b + (uint64_t)t] : kRmtNoKey;
            int st = valid ? (int)status[b + (uint64_t)t] : -1;
            const bool claim = mine >= 0;                    // only a failing entry has a choice
            if (__ballot(claim) != 0ull) {
                bool lose = false;
#pragma unroll 1
                for (int s = 0; s < n; ++s) {                // wave-uniform addresses
                    const int cs = choice[b + (uint64_t)s];
                    if (cs < 0) continue;
                    const unsigned long long bs = r2bits[b + (uint64_t)s];
                    lose = lose || (cs == mine && s != t && (bs < mb || (bs == mb && s < t)));
                }
                if (claim && !lose) {
                    st = kRematchReassigned;
                    status[b + (uint64_t)t] = (uint8_t)st;
                }
            }
#pragma unroll
            for (int kind = 0; kind < kRematchKinds; ++kind) {
                const unsigned long long m = __ballot(st == kind);
                if (lane == 0 && m) atomicAdd(&sCnt[kind], (unsigned)__popcll(m));
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < kRematchKinds && sCnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)sCnt[threadIdx.x]);
}

// Rule 7: pt_new[o] = the label after the call (a list of its own), keep[o] = 0 where the observation is removed.
__global__ __launch_bounds__(256) void k_rematch_apply(const uint32_t *__restrict__ pt_idx, int64_t n_obs, const int32_t *__restrict__ choice,
                                                      const uint8_t *__restrict__ status, uint32_t *__restrict__ pt_new,
                                                      uint8_t *__restrict__ keep) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const uint8_t st = status[o];
    pt_new[o] = st == kRematchReassigned ? (uint32_t)choice[o] : pt_idx[o];
    keep[o] = st != kRematchRemoved ? 1 : 0;
}

}  // namespace c2b
