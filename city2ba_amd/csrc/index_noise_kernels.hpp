// index_noise_kernels.hpp -- gfx950 kernels of the index noise (included by capi.hip only, after rematch_kernels.hpp).
//
// noise.rs' index-corruption functions (src/noise.rs:179-378) in place on the resident problem: drop_features,
// add_incorrect_correspondences, split_landmarks, join_landmarks.  host_noise.hpp draws them from one sequential generator; here
// every draw is a Philox4x32-10 block of its own, addressed as normal_pair addresses it (camera_math.hpp):
//   counter = (entity lo, entity hi, slot, stream), key = the seed's halves; a = o1 << 32 | o0, b = o3 << 32 | o2;
//   u(x) = (x >> 11) * 2^-53 in [0, 1).  Streams: 6 drop, 7 mismatch, 8 split, 9 join.
// so a seed fixes the result whatever the launch shape.  tests/_indexnoiseref.py restates every rule below; the tests compare ==.
//   drop      (src/noise.rs:229-251) camera row of len entries keeps l = saturating floor(len * keep_fraction) of them: those
//             with the l smallest (a, index), a = stream 6, entity = observation index, slot 0.  k_drop_keep: one wave per
//             camera finds the l-th smallest a bit by bit (64 counting passes of ballots: no LDS, no scratch, any row
//             length), then marks a < T, and of the entries with a == T the first by index that are still needed.
//   mismatch  (src/noise.rs:180-226) observation i of a row with len > 1 swaps iff u(a) <= chance (stream 7, entity =
//             observation index, slot 0); its partner j is drawn with weight w_k = max_d - d_ik (so w_i = max_d: the reference
//             zeroes weights[i] before it shifts them, :203-205), d_ik = sqrt(dx * dx + dy * dy) unfused: the first k whose
//             cumulative weight exceeds u(b) * total, else len - 1.  k_mismatch_partner: one wave per camera, per swapping
//             entry three walks of the row (max, total, threshold) with the same wave scan in both sums, so the total IS the
//             last cumulative value.  A row with a swapping entry whose total is not positive is counted.  k_mismatch_apply:
//             one lane per camera, the swaps of pt_idx in ascending i (they do not commute).
//   select    the n smallest (a, index) of N entities (points: split, observations: join).  A radix select: eight counting
//             passes over 8-bit digits (k_select_hist: LDS histogram, then 256 integer atomics per workgroup), the digit picked
//             on the host between them; k_select_mark; ties of the full key by index through a scan (k_select_ties).
//   split     (src/noise.rs:255-291) the copy of the r-th selected point in ascending index is row n_pts + r (k_split_points);
//             an observation of a selected point moves to the copy iff bit 0 of a (stream 8, entity = observation index,
//             slot 1) is set (k_split_obs).
//   join      (src/noise.rs:323-378) a selected observation's point q is replaced by entry 1 + floor(u(b) * avail) of the
//             ascending (d2, index) list of the 1 + 10 nearest points of q (q among them), avail = min(10, n_pts - 1), b of
//             stream 9, entity = observation index, slot 0; d2 = (dx * dx + dy * dy) + dz * dz unfused.
//   nearest   k_nearest_points: one wave per query over the x / z cell list of the points.  The lanes stride over the cells of
//             the square ring r around the query's cell; lanes 0 .. 10 hold the best eleven keys (bits of d2, index) in ascending
//             order, a register per lane: a candidate below the eleventh is inserted by one ballot and one shift (no per-lane
//             arrays, no LDS).  After ring r everything unvisited is farther than r cells away, so the walk ends when the
//             k-th key's d2 <= (r * cs * (1 - 2^-20))^2 -- the factor covers the rounding of the cell arithmetic -- or the
//             grid is exhausted.  Every cell is visited once, and a minimum over a set does not depend on the cell fill's order.
// No float atomics, no scratch memory; no wave returns before a wave-wide operation (a wave without work skips a uniform block).
#pragma once
#include "rematch_kernels.hpp"

namespace c2b {

constexpr int kIdxBlock = 256;
constexpr int kIdxWaves = kIdxBlock / 64;
constexpr int kNearest = 11;                                 // the point itself + its ten nearest others

C2B_DEV void index_draw(uint64_t seed, uint32_t stream, uint64_t entity, uint32_t slot, uint64_t &a, uint64_t &b) {
    uint32_t o[4];
    philox4x32_10((uint32_t)entity, (uint32_t)(entity >> 32), slot, stream, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    a = ((uint64_t)o[1] << 32) | o[0];
    b = ((uint64_t)o[3] << 32) | o[2];
}
C2B_DEV double index_uniform(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }

// ---- drop_features -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kIdxBlock) void k_drop_keep(const uint64_t *__restrict__ row_ptr, int64_t n_cam, double keep_fraction,
                                                        uint64_t seed, uint8_t *__restrict__ keep) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kIdxWaves + wave;
    if (c < n_cam) {                                         // wave-uniform; the kernel has no barrier
        const uint64_t b = row_ptr[c], len = row_ptr[c + 1] - b;
        const double kf = (double)len * keep_fraction;
        const uint64_t l = kf > 0.0 ? (kf >= (double)len ? len : (uint64_t)kf) : 0;          // `as usize` saturates
        if (l == 0 || l == len) {
            for (uint64_t t = lane; t < len; t += 64) keep[b + t] = l ? 1 : 0;
        } else {
            uint64_t a0, unused;                             // the first chunk's keys stay in a register: most rows are one chunk
            index_draw(seed, kStreamDrop, b + (uint64_t)lane, 0, a0, unused);
            uint64_t prefix = 0, need = l;
#pragma unroll 1
            for (int bit = 63; bit >= 0; --bit) {            // T = the l-th smallest a, from its top bit down
                uint64_t zeros = 0;
#pragma unroll 1
                for (uint64_t t0 = 0; t0 < len; t0 += 64) {
                    const uint64_t t = t0 + (uint64_t)lane;
                    uint64_t a = a0;
                    if (t0) index_draw(seed, kStreamDrop, b + t, 0, a, unused);
                    zeros += (uint64_t)__popcll(__ballot(t < len && (a >> bit) == (prefix >> bit)));
                }
                if (need > zeros) { need -= zeros; prefix |= 1ull << bit; }
            }
            uint64_t seen = 0;                               // entries equal to T met so far
#pragma unroll 1
            for (uint64_t t0 = 0; t0 < len; t0 += 64) {
                const uint64_t t = t0 + (uint64_t)lane;
                uint64_t a = a0;
                if (t0) index_draw(seed, kStreamDrop, b + t, 0, a, unused);
                const unsigned long long eq = __ballot(t < len && a == prefix);
                const uint64_t before = seen + (uint64_t)__popcll(eq & ((1ull << lane) - 1ull));
                if (t < len) keep[b + t] = (a < prefix || (a == prefix && before < need)) ? 1 : 0;
                seen += (uint64_t)__popcll(eq);
            }
        }
    }
}

// ---- add_incorrect_correspondences -----------------------------------------------------------------------------------------
// the wave's walk of the row for entry i at (xi, yi): pass 0 the largest distance, pass 1 the sum of the weights (cumulative in
// row order: a wave scan per chunk and a carry), pass 2 the first entry whose cumulative weight exceeds thr
C2B_DEV double mismatch_chunk_weight(const double2 *__restrict__ uv, uint64_t b, int n, int s, double xi, double yi, double maxd) {
    if (s >= n) return 0.0;
    const double2 q = uv[b + (uint64_t)s];
    const double dx = xi - q.x, dy = yi - q.y;
    return maxd - sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(kIdxBlock) void k_mismatch_partner(const uint64_t *__restrict__ row_ptr, int64_t n_cam,
                                                               const double2 *__restrict__ uv, double chance, uint64_t seed,
                                                               int32_t *__restrict__ partner, unsigned long long *__restrict__ n_zero) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kIdxWaves + wave;
    if (c < n_cam) {                                         // wave-uniform
        const uint64_t b = row_ptr[c];
        const int n = (int)(row_ptr[c + 1] - b);             // (the launcher holds n_obs below 2^31 - 64)
        bool zero_row = false;
#pragma unroll 1
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int t = t0 + lane;
            const bool valid = t < n;
            uint64_t a = 0, bb = 0;
            if (valid) index_draw(seed, kStreamMismatch, b + (uint64_t)t, 0, a, bb);
            const bool swaps = valid && n > 1 && index_uniform(a) <= chance;
            const double ub = index_uniform(bb);
            int mine = -1;
            unsigned long long todo = __ballot(swaps);
#pragma unroll 1
            while (todo) {                                   // wave-uniform
                const int k = (int)__builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int i = t0 + k;
                const double2 pi = uv[b + (uint64_t)i];
                const double u = __shfl(ub, k, 64);
                double maxd = 0.0;
#pragma unroll 1
                for (int s0 = 0; s0 < n; s0 += 64) {         // (a weight against 0 is minus the distance)
                    const double d = -mismatch_chunk_weight(uv, b, n, s0 + lane, pi.x, pi.y, 0.0);
                    maxd = d > maxd ? d : maxd;
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const double o = __shfl_xor(maxd, d, 64);
                    maxd = o > maxd ? o : maxd;
                }
                double total = 0.0;
#pragma unroll 1
                for (int s0 = 0; s0 < n; s0 += 64) {
                    double w = mismatch_chunk_weight(uv, b, n, s0 + lane, pi.x, pi.y, maxd);
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const double o = __shfl_up(w, off, 64);
                        if (lane >= off) w += o;
                    }
                    total += __shfl(w, 63, 64);
                }
                int j = -1;
                if (total > 0.0) {
                    const double thr = u * total;
                    double carry = 0.0;
                    j = n - 1;
#pragma unroll 1
                    for (int s0 = 0; s0 < n; s0 += 64) {
                        double w = mismatch_chunk_weight(uv, b, n, s0 + lane, pi.x, pi.y, maxd);
#pragma unroll
                        for (int off = 1; off < 64; off <<= 1) {
                            const double o = __shfl_up(w, off, 64);
                            if (lane >= off) w += o;
                        }
                        const unsigned long long over = __ballot(s0 + lane < n && thr < carry + w);
                        if (over) { j = s0 + (int)__builtin_ctzll(over); break; }            // wave-uniform
                        carry += __shfl(w, 63, 64);
                    }
                } else {
                    zero_row = true;                         // WeightedIndex::new(..).unwrap() panics: AllWeightsZero
                }
                if (lane == k) mine = j;
            }
            if (valid) partner[b + (uint64_t)t] = mine;
        }
        if (zero_row && lane == 0) atomicAdd(n_zero, 1ull);
    }
}

// the swaps of one camera in ascending i; *n_swaps += the entries that swapped (one with itself included)
__global__ __launch_bounds__(256) void k_mismatch_apply(const uint64_t *__restrict__ row_ptr, int64_t n_cam, const int32_t *__restrict__ partner,
                                                       uint32_t *__restrict__ pt_idx, unsigned long long *__restrict__ n_swaps) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cam) return;
    const uint64_t b = row_ptr[c], e = row_ptr[c + 1];
    unsigned long long n = 0;
    for (uint64_t i = b; i < e; ++i) {
        const int32_t j = partner[i];
        if (j < 0) continue;
        const uint32_t pi = pt_idx[i], pj = pt_idx[b + (uint64_t)j];
        pt_idx[i] = pj; pt_idx[b + (uint64_t)j] = pi;
        ++n;
    }
    if (n) atomicAdd(n_swaps, n);
}

// ---- the n smallest (key, index) of N entities ---------------------------------------------------------------------------------
// keys == NULL: key(i) = a of (seed; stream, entity_base + i, slot)
C2B_DEV uint64_t select_key(const uint64_t *__restrict__ keys, int64_t i, uint64_t entity_base, uint64_t seed, uint32_t stream, uint32_t slot) {
    if (keys) return keys[i];
    uint64_t a, unused;
    index_draw(seed, stream, entity_base + (uint64_t)i, slot, a, unused);
    return a;
}

// hist[256] += the digit (key >> shift) & 255 of every key that agrees with prefix above that digit
__global__ __launch_bounds__(256) void k_select_hist(const uint64_t *__restrict__ keys, int64_t n, uint64_t entity_base, uint64_t seed,
                                                    uint32_t stream, uint32_t slot, uint64_t prefix, int shift,
                                                    unsigned long long *__restrict__ hist) {
    __shared__ unsigned sHist[256];
    sHist[threadIdx.x] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t a = select_key(keys, i, entity_base, seed, stream, slot);
        const bool in = shift == 56 || (a >> (shift + 8)) == (prefix >> (shift + 8));
        if (in) atomicAdd(&sHist[(unsigned)(a >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (sHist[threadIdx.x]) atomicAdd(hist + threadIdx.x, (unsigned long long)sHist[threadIdx.x]);
}

// sel[i] = key < T, or key <= T with take_equal; eq[i] (may be NULL) = key == T
__global__ __launch_bounds__(256) void k_select_mark(const uint64_t *__restrict__ keys, int64_t n, uint64_t entity_base, uint64_t seed,
                                                    uint32_t stream, uint32_t slot, uint64_t T, int take_equal, uint8_t *__restrict__ sel,
                                                    uint32_t *__restrict__ eq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = select_key(keys, i, entity_base, seed, stream, slot);
    sel[i] = (a < T || (take_equal && a == T)) ? 1 : 0;
    if (eq) eq[i] = a == T ? 1u : 0u;
}

// of the entries equal to T the first `need` by index
__global__ __launch_bounds__(256) void k_select_ties(const uint32_t *__restrict__ eq, const uint32_t *__restrict__ pos, int64_t n, uint32_t need,
                                                    uint8_t *__restrict__ sel) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && eq[i] && pos[i] < need) sel[i] = 1;
}

// list[pos[i]] = i for every selected i (pos: the exclusive scan of sel)
__global__ __launch_bounds__(256) void k_select_list(const uint8_t *__restrict__ sel, const uint32_t *__restrict__ pos, int64_t n,
                                                    uint32_t *__restrict__ list) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && sel[i]) list[pos[i]] = (uint32_t)i;
}

// ---- split_landmarks ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_split_points(const double4 *__restrict__ pts4, int64_t n_pts, const uint8_t *__restrict__ sel,
                                                     const uint32_t *__restrict__ pos, double4 *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pts) return;
    const double4 P = pts4[p];
    out[p] = P;
    if (sel[p]) out[n_pts + (int64_t)pos[p]] = P;            // the same bits, the fourth lane too
}

__global__ __launch_bounds__(256) void k_split_obs(uint32_t *__restrict__ pt_idx, int64_t n_obs, int64_t n_pts, const uint8_t *__restrict__ sel,
                                                  const uint32_t *__restrict__ pos, uint64_t seed) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const uint32_t p = pt_idx[o];
    if (!sel[p]) return;
    uint64_t a, unused;
    index_draw(seed, kStreamSplit, (uint64_t)o, 1, a, unused);
    if (a & 1ull) pt_idx[o] = (uint32_t)(n_pts + (int64_t)pos[p]);
}

// ---- the nearest points ---------------------------------------------------------------------------------------------------------
// nn[r * kNearest + e] = the e-th nearest point of point query[r] by (d2, index), itself included; -1 past the table's size
__global__ __launch_bounds__(kIdxBlock) void k_nearest_points(const double4 *__restrict__ pts4, int64_t n_pts, const uint32_t *__restrict__ query,
                                                             int64_t n_query, CellGrid g, double cs, const uint32_t *__restrict__ start,
                                                             const uint32_t *__restrict__ sorted, int32_t *__restrict__ nn) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t r_q = (int64_t)blockIdx.x * kIdxWaves + wave;
    if (r_q < n_query) {                                     // wave-uniform; the kernel has no barrier
        const uint32_t q = query[r_q];
        const double4 Q = pts4[q];
        const int c0x = __builtin_amdgcn_readfirstlane(cell_coord(Q.x, g.x0, g.inv_cs, g.ncx));
        const int c0z = __builtin_amdgcn_readfirstlane(cell_coord(Q.z, g.z0, g.inv_cs, g.ncz));
        const int want = n_pts < kNearest ? (int)n_pts : kNearest;
        unsigned long long hd = ~0ull;                       // lanes 0 .. 10: the best keys so far, ascending
        uint32_t hi = 0xffffffffu;
        int64_t visited = 0;
        int rmax = c0x > g.ncx - 1 - c0x ? c0x : g.ncx - 1 - c0x;
        rmax = c0z > rmax ? c0z : rmax;
        rmax = g.ncz - 1 - c0z > rmax ? g.ncz - 1 - c0z : rmax;
#pragma unroll 1
        for (int r = 0; r <= rmax; ++r) {
            const int ixa = c0x - r > 0 ? c0x - r : 0, ixb = c0x + r < g.ncx - 1 ? c0x + r : g.ncx - 1;
#pragma unroll 1
            for (int ix = ixa; ix <= ixb; ++ix) {
                const bool edge = ix == c0x - r || ix == c0x + r;         // a whole column of the ring; else its two end cells
#pragma unroll 1
                for (int part = 0; part < 2; ++part) {
                    int za, zb;
                    if (edge) {
                        if (part) break;
                        za = c0z - r > 0 ? c0z - r : 0; zb = c0z + r < g.ncz - 1 ? c0z + r : g.ncz - 1;
                    } else {
                        za = zb = part ? c0z + r : c0z - r;
                        if (za < 0 || za >= g.ncz) continue;
                    }
                    const uint32_t kb = start[ix * g.ncz + za], ke = start[ix * g.ncz + zb + 1];
                    visited += (int64_t)(ke - kb);
#pragma unroll 1
                    for (uint32_t k0 = kb; k0 < ke; k0 += 64u) {          // wave-uniform trip count
                        const uint32_t k = k0 + (uint32_t)lane;
                        bool has = k < ke;
                        unsigned long long cd = ~0ull;
                        uint32_t ci = 0xffffffffu;
                        if (has) {
                            ci = sorted[k];
                            const double4 P = pts4[ci];
                            const double dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
                            cd = (unsigned long long)__double_as_longlong((dx * dx + dy * dy) + dz * dz);      // d2 >= 0: its bits order it
                        }
#pragma unroll 1
                        for (;;) {                           // the chunk's candidates below the eleventh key, smallest first
                            const unsigned long long wd = __shfl(hd, kNearest - 1, 64);
                            const uint32_t wi = (uint32_t)__shfl((int)hi, kNearest - 1, 64);
                            const bool live = has && (cd < wd || (cd == wd && ci < wi));
                            if (__ballot(live) == 0ull) break;
                            unsigned long long md = live ? cd : ~0ull;
                            uint32_t mi = live ? ci : 0xffffffffu;
#pragma unroll
                            for (int d = 32; d >= 1; d >>= 1) {
                                const unsigned long long od = __shfl_xor(md, d, 64);
                                const uint32_t oi = (uint32_t)__shfl_xor((int)mi, d, 64);
                                if (od < md || (od == md && oi < mi)) { md = od; mi = oi; }
                            }
                            if (live && cd == md && ci == mi) has = false;                   // (an index is met once: one lane)
                            const int at = (int)__popcll(__ballot(lane < kNearest && (hd < md || (hd == md && hi < mi))));
                            const unsigned long long ud = __shfl_up(hd, 1, 64);
                            const uint32_t ui = (uint32_t)__shfl_up((int)hi, 1, 64);
                            if (lane < kNearest && lane > at) { hd = ud; hi = ui; }
                            if (lane == at) { hd = md; hi = mi; }
                        }
                    }
                }
            }
            if (visited >= (int64_t)want) {                  // everything unvisited is farther than r cells away
                const double safe = (double)r * cs * (1.0 - 0x1.0p-20);
                const double dk = __longlong_as_double((long long)__shfl(hd, want - 1, 64));
                if (dk <= safe * safe || visited >= n_pts) break;
            }
        }
        if (lane < kNearest) nn[r_q * kNearest + lane] = hi == 0xffffffffu ? -1 : (int32_t)hi;
    }
}

// ---- join_landmarks -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_join_queries(const uint32_t *__restrict__ pt_idx, const uint32_t *__restrict__ list, int64_t n,
                                                     uint32_t *__restrict__ query) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) query[r] = pt_idx[list[r]];
}

__global__ __launch_bounds__(256) void k_join_apply(uint32_t *__restrict__ pt_idx, const uint32_t *__restrict__ list, int64_t n,
                                                   const int32_t *__restrict__ nn, int avail, uint64_t seed) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint32_t o = list[r];
    uint64_t unused, bb;
    index_draw(seed, kStreamJoin, (uint64_t)o, 0, unused, bb);
    int e = (int)(index_uniform(bb) * (double)avail);
    e = e < avail ? e : avail - 1;
    pt_idx[o] = (uint32_t)nn[r * kNearest + 1 + e];
}

}  // namespace c2b
