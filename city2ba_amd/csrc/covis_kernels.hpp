// covis_kernels.hpp -- gfx950 kernels of the camera covisibility graph and of the search over it (included by capi.hip only,
// after scan_kernels.hpp).
//
// c2b_covisibility_degree_rows / c2b_covisibility_fill_rows / c2b_covisibility_expand_rows: cameras are nodes,
// shared(c, c') = the number of DISTINCT points with an observation in row c and one in row c'.  The contract is the header's;
// the passes:
//   * covis_walk: the one walk of a camera's row both paths and both passes share.  The lanes load 64 observations of the row
//     (point, track bounds) at a time; the tracks are then walked one after the other, the lanes striding over a track through
//     the transpose.  A track is ascending in camera index (the list is camera-major and the transpose stable), so
//       - the entries of one camera are adjacent: an entry counts when its camera differs from the entry before it;
//       - the first entry of c itself names ONE observation of (c, p): the observation of row c that it names is the one that
//         walks p's track, every repeat of (c, p) in the row walks nothing.  No sort of the row.
//   * k_covis_bound: one wave per camera, heavy[c] = (bound > kCvSlots), bound = the sum over the row of (track length - 1): every
//     track of the row holds the observation that led to it.  It bounds the number of distinct neighbours from above, so a
//     table of kCvSlots slots always has room (at bound == kCvSlots it may end exactly full).
//   * k_covis_light<FILL>: one wave per camera that is not heavy.  (camera -> count) in a wave-private open-addressing table of
//     kCvSlots slots in LDS, by integer LDS atomics: a count does not depend on the arrival order.  The degree pass counts the
//     slots with count >= min_shared.  The fill pass compacts those slots to the front of the table in place, pads to a power of
//     two, sorts by camera index (a bitonic network over LDS by the one wave) and writes the row out.
//   * k_covis_heavy<FILL>: a workgroup per heavy camera, a few workgroups striding over the list of them, each with a dense
//     u32 [n_cam] counter row in global scratch: the four waves split the row's chunks and add by integer global atomics; the
//     span [lowest, highest] camera touched is then read in ascending order -- counted, or written through a workgroup scan --
//     and zeroed again.  The same integers as the table gives, in the same order.
//   * k_covis_mark / k_covis_level_flags / k_covis_compact / k_covis_score / k_covis_unselect: the breadth-first search, a level a call.
// Integers only: no float atomics, no scratch memory; the same list gives the same bytes whatever the launch shape.
#pragma once
#include "scan_kernels.hpp"

namespace c2b {

constexpr int kCvSlots = C2B_COVIS_WAVE_SLOTS;               // slots of a wave's table
constexpr int kCvWaves = 2;                                  // cameras (tables) per workgroup of the light path: 2 x 16 KiB of LDS
constexpr int kCvBlock = kCvWaves * 64;
constexpr int kCvHeavyBlock = kScanBlock;                    // the heavy path scans with block_excl_scan
constexpr uint32_t kCvEmpty = 0xffffffffu;                   // no camera has this index (n_cam < 2^31)
static_assert(kCvSlots >= 64 && (kCvSlots & (kCvSlots - 1)) == 0, "the table is a power of two of at least a wave");
constexpr int cv_log2(int v) { return v <= 1 ? 0 : 1 + cv_log2(v >> 1); }
constexpr int kCvLog = cv_log2(kCvSlots);

// what the wave's lanes wrote to its table is visible to its other lanes after this (one wave: no workgroup barrier)
__device__ __forceinline__ void covis_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The walk of row [rb, re) of camera c by one wave that takes the chunks part, part + parts, ... of 64 observations: sink(c')
// once for every (distinct point p of the row, distinct camera c' != c of p's track), from whichever lane meets it.
template <class Sink>
__device__ __forceinline__ void covis_walk(const uint32_t c, const uint64_t rb, const uint64_t re, const int lane, const int part, const int parts,
                                           const uint32_t *__restrict__ pt_idx, const uint64_t *__restrict__ pt_row_ptr,
                                           const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, Sink &&sink) {
#pragma unroll 1
    for (uint64_t o0 = rb + 64u * (uint64_t)part; o0 < re; o0 += 64u * (uint64_t)parts) {       // wave-uniform
        const uint64_t o = o0 + (uint64_t)lane;
        unsigned long long tb = 0ull, te = 0ull;
        if (o < re) {
            const uint32_t p = pt_idx[o];
            tb = pt_row_ptr[p];
            te = pt_row_ptr[p + 1];
        }
        const int n = re - o0 < 64u ? (int)(re - o0) : 64;
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            const uint64_t b = __shfl(tb, j, 64), e = __shfl(te, j, 64);
            // the observation of (c, p) that the first entry of c in p's track names walks the track
            uint32_t first = kCvEmpty;
#pragma unroll 1
            for (uint64_t k0 = b; k0 < e; k0 += 64u) {
                const uint64_t k = k0 + (uint64_t)lane;
                const bool mine = k < e && cam_of[k] == c;
                const unsigned long long hit = __ballot(mine);
                if (hit) {
                    const uint32_t ob = mine ? obs_of[k] : 0u;
                    first = (uint32_t)__shfl((int)ob, __ffsll(hit) - 1, 64);
                    break;
                }
            }
            if (first != (uint32_t)(o0 + (uint64_t)j)) continue;                 // a repeat of (c, p): counted at its first
#pragma unroll 1
            for (uint64_t k0 = b; k0 < e; k0 += 64u) {
                const uint64_t k = k0 + (uint64_t)lane;
                if (k < e) {
                    const uint32_t cam = cam_of[k];
                    const uint32_t prev = k > b ? cam_of[k - 1] : kCvEmpty;
                    if (cam != c && cam != prev) sink(cam);
                }
            }
        }
    }
}

// heavy[c] = 1 when the row's bound (the sum of its track lengths, less one each) does not fit the table.  One wave per camera.
__global__ __launch_bounds__(256) void k_covis_bound(const uint64_t *__restrict__ row_ptr, const uint32_t *__restrict__ pt_idx,
                                                    const uint64_t *__restrict__ pt_row_ptr, int64_t n_cam, uint32_t *__restrict__ heavy) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_cam) return;
    const uint64_t rb = row_ptr[c], re = row_ptr[c + 1];
    unsigned long long sum = 0ull;
    for (uint64_t o = rb + (uint64_t)lane; o < re; o += 64u) {
        const uint32_t p = pt_idx[o];
        sum += pt_row_ptr[p + 1] - pt_row_ptr[p] - 1u;          // (the track holds this observation)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) heavy[c] = sum > (unsigned long long)kCvSlots ? 1u : 0u;
}

// one camera into one slot of the wave's table.  Ends: the table holds at most `bound` <= kCvSlots distinct cameras.
__device__ __forceinline__ void covis_insert(uint32_t *keys, uint32_t *cnt, const uint32_t cam) {
    uint32_t h = (cam * 2654435761u) >> (32 - kCvLog);
    for (;;) {
        const uint32_t old = atomicCAS(&keys[h], kCvEmpty, cam);
        if (old == kCvEmpty || old == cam) {
            atomicAdd(&cnt[h], 1u);
            return;
        }
        h = (h + 1u) & (uint32_t)(kCvSlots - 1);
    }
}

// FILL false: deg[c] = the neighbours with shared >= min_shared.  FILL true: the row written at nbr_ptr[c], ascending.
template <bool FILL>
__global__ __launch_bounds__(kCvBlock) void k_covis_light(const uint64_t *__restrict__ row_ptr, const uint32_t *__restrict__ pt_idx,
                                                         const uint64_t *__restrict__ pt_row_ptr, const uint32_t *__restrict__ obs_of,
                                                         const uint32_t *__restrict__ cam_of, int64_t n_cam, uint32_t min_shared,
                                                         const uint32_t *__restrict__ heavy, uint64_t *__restrict__ deg,
                                                         const uint64_t *__restrict__ nbr_ptr, uint32_t *__restrict__ nbr,
                                                         uint32_t *__restrict__ shared) {
    __shared__ uint32_t sKeys[kCvWaves][kCvSlots], sCnt[kCvWaves][kCvSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * kCvWaves + wave;
    if (c >= n_cam || heavy[c]) return;                      // wave-uniform; no workgroup barrier below
    const uint64_t rb = row_ptr[c], re = row_ptr[c + 1];
    if (rb == re) {
        if (!FILL && lane == 0) deg[c] = 0;
        return;
    }
    uint32_t *keys = sKeys[wave], *cnt = sCnt[wave];
    for (int s = lane; s < kCvSlots; s += 64) { keys[s] = kCvEmpty; cnt[s] = 0u; }
    covis_wave_sync();
    covis_walk((uint32_t)c, rb, re, lane, 0, 1, pt_idx, pt_row_ptr, obs_of, cam_of, [&](uint32_t cam) { covis_insert(keys, cnt, cam); });
    covis_wave_sync();
    if (!FILL) {
        uint32_t m = 0;
        for (int s = lane; s < kCvSlots; s += 64) m += keys[s] != kCvEmpty && cnt[s] >= min_shared;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m += __shfl_xor(m, d, 64);
        if (lane == 0) deg[c] = m;
        return;
    }
    // the kept slots to the front, in place: a chunk is in registers before its survivors are written at or below it
    int m = 0;
#pragma unroll 1
    for (int s0 = 0; s0 < kCvSlots; s0 += 64) {
        const uint32_t k = keys[s0 + lane], v = cnt[s0 + lane];
        const bool keep = k != kCvEmpty && v >= min_shared;
        const unsigned long long bal = __ballot(keep);
        covis_wave_sync();
        if (keep) {
            const int at = m + __popcll(bal & ((1ull << lane) - 1ull));
            keys[at] = k;
            cnt[at] = v;
        }
        m += __popcll(bal);
        covis_wave_sync();
    }
    if (m == 0) return;
    int P = 2;
    while (P < m) P <<= 1;
    for (int s = m + lane; s < P; s += 64) keys[s] = kCvEmpty;               // sorts behind every camera
    covis_wave_sync();
#pragma unroll 1
    for (int k = 2; k <= P; k <<= 1) {
#pragma unroll 1
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int x = i ^ j;
                if (x > i) {
                    const uint32_t a = keys[i], b = keys[x];
                    if ((a > b) == ((i & k) == 0)) {
                        const uint32_t va = cnt[i], vb = cnt[x];
                        keys[i] = b; keys[x] = a;
                        cnt[i] = vb; cnt[x] = va;
                    }
                }
            }
            covis_wave_sync();
        }
    }
    const uint64_t at = nbr_ptr[c];
    for (int s = lane; s < m; s += 64) {
        nbr[at + (uint64_t)s] = keys[s];
        shared[at + (uint64_t)s] = cnt[s];
    }
}

// The heavy cameras list[0 .. *n_list), a workgroup each, the workgroups striding over the list.  dense: gridDim.x rows of
// n_cam counters, zero on entry and zero again on exit.
template <bool FILL>
__global__ __launch_bounds__(kCvHeavyBlock) void k_covis_heavy(const uint64_t *__restrict__ row_ptr, const uint32_t *__restrict__ pt_idx,
                                                              const uint64_t *__restrict__ pt_row_ptr, const uint32_t *__restrict__ obs_of,
                                                              const uint32_t *__restrict__ cam_of, int64_t n_cam, uint32_t min_shared,
                                                              const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list,
                                                              uint32_t *__restrict__ dense_all, uint64_t *__restrict__ deg,
                                                              const uint64_t *__restrict__ nbr_ptr, uint32_t *__restrict__ nbr,
                                                              uint32_t *__restrict__ shared) {
    __shared__ uint32_t sSpan[2];
    __shared__ uint32_t sWave[kScanBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *dense = dense_all + (uint64_t)blockIdx.x * (uint64_t)n_cam;
    const uint32_t n_heavy = *n_list;
#pragma unroll 1
    for (uint32_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {             // workgroup-uniform
        const uint32_t c = list[h];
        if (threadIdx.x == 0) { sSpan[0] = kCvEmpty; sSpan[1] = 0u; }
        __syncthreads();
        uint32_t lo = kCvEmpty, hi = 0u;
        covis_walk(c, row_ptr[c], row_ptr[c + 1], lane, wave, kScanBlock / 64, pt_idx, pt_row_ptr, obs_of, cam_of, [&](uint32_t cam) {
            __hip_atomic_fetch_add(&dense[cam], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lo = cam < lo ? cam : lo;
            hi = cam > hi ? cam : hi;
        });
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t a = (uint32_t)__shfl_xor((int)lo, d, 64), b = (uint32_t)__shfl_xor((int)hi, d, 64);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        if (lane == 0 && lo != kCvEmpty) { atomicMin(&sSpan[0], lo); atomicMax(&sSpan[1], hi); }
        __threadfence();                                     // every wave's adds have arrived before the span is read
        __syncthreads();
        const int64_t s_lo = sSpan[0], s_hi = sSpan[1];
        const uint64_t at = FILL ? nbr_ptr[c] : 0;
        uint32_t carry = 0;
#pragma unroll 1
        for (int64_t base = s_lo; base <= s_hi; base += kScanBlock) {        // workgroup-uniform; empty when nothing was touched
            const int64_t i = base + threadIdx.x;
            uint32_t v = 0;
            if (i <= s_hi) {
                v = __hip_atomic_load(&dense[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v) __hip_atomic_store(&dense[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const uint32_t keep = v >= min_shared && v != 0u ? 1u : 0u;
            uint32_t total;
            const uint32_t ex = block_excl_scan(keep, sWave, total);
            if (FILL && keep) {
                nbr[at + carry + ex] = (uint32_t)i;
                shared[at + carry + ex] = v;
            }
            carry += total;
            __syncthreads();                                 // sWave is read
        }
        if (!FILL && threadIdx.x == 0) deg[c] = carry;
        __threadfence();                                     // the row is zero again before the next camera adds to it
        __syncthreads();
    }
}

// counts[0] = the directed edges (the row pointer's last entry), counts[1] = the cameras that took the heavy path
__global__ void k_covis_counts(const uint64_t *__restrict__ nbr_ptr, int64_t n_cam, const uint32_t *__restrict__ n_heavy, int64_t *__restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counts[0] = (int64_t)nbr_ptr[n_cam];
        counts[1] = (int64_t)*n_heavy;
    }
}

// ---- the search: a level a call ----------------------------------------------------------------------------------------
// One wave per camera of the frontier (level h): its neighbours that are not reached yet, lie inside `within` (NULL: all do)
// and share at least min_shared points get level h + 1.  Racing stores write the same value.
__global__ __launch_bounds__(256) void k_covis_mark(const uint64_t *__restrict__ nbr_ptr, const uint32_t *__restrict__ nbr,
                                                   const uint32_t *__restrict__ shared, uint32_t min_shared,
                                                   const uint8_t *__restrict__ within, const uint32_t *__restrict__ frontier,
                                                   int64_t n_frontier, int32_t next_level, int32_t *level) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n_frontier) return;
    const uint32_t c = frontier[f];
    const uint64_t e = nbr_ptr[c + 1];
    for (uint64_t k = nbr_ptr[c] + (uint64_t)lane; k < e; k += 64u) {
        const uint32_t q = nbr[k];
        if (shared[k] < min_shared || (within && !within[q])) continue;
        if (level[q] < 0) level[q] = next_level;
    }
}

// flag[c] = 1 for the cameras of level h
__global__ __launch_bounds__(256) void k_covis_level_flags(const int32_t *__restrict__ level, int64_t n_cam, int32_t h, uint32_t *__restrict__ flag) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n_cam) flag[c] = level[c] == h ? 1u : 0u;
}

// the flagged cameras in ascending index (pos: the exclusive scan of flag)
__global__ __launch_bounds__(256) void k_covis_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t n_cam,
                                                      uint32_t *__restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n_cam && flag[c]) out[pos[c]] = (uint32_t)c;
}

// One wave per candidate (a camera of level h + 1): score = the sum of shared over its edges of at least min_shared into the
// levels 0 .. h, saturating at 2^32 - 1; key[c] = 2^32 - 1 - score, so that the smallest (key, index) is the best candidate.
__global__ __launch_bounds__(256) void k_covis_score(const uint64_t *__restrict__ nbr_ptr, const uint32_t *__restrict__ nbr,
                                                    const uint32_t *__restrict__ shared, uint32_t min_shared,
                                                    const uint32_t *__restrict__ cand, int64_t n_cand, int32_t h,
                                                    const int32_t *__restrict__ level, uint64_t *__restrict__ key) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n_cand) return;
    const uint32_t c = cand[f];
    const uint64_t e = nbr_ptr[c + 1];
    unsigned long long sum = 0ull;
    for (uint64_t k = nbr_ptr[c] + (uint64_t)lane; k < e; k += 64u) {
        const int32_t l = level[nbr[k]];
        const uint32_t s = shared[k];
        if (s >= min_shared && l >= 0 && l <= h) sum += s;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);         // (fewer than 2^31 edges of less than 2^32 each)
    if (lane == 0) key[c] = 0xffffffffull - (sum > 0xffffffffull ? 0xffffffffull : sum);
}

// the candidates that were not selected are not reached after all
__global__ __launch_bounds__(256) void k_covis_unselect(const uint32_t *__restrict__ cand, int64_t n_cand, const uint8_t *__restrict__ select,
                                                       int32_t *__restrict__ level) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_cand) return;
    const uint32_t c = cand[f];
    if (!select || !select[c]) level[c] = -1;
}

// level[c] = 0 for a seed, -1 for every other camera
__global__ __launch_bounds__(256) void k_covis_seed_levels(const uint8_t *__restrict__ seed, int64_t n_cam, int32_t *__restrict__ level) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n_cam) level[c] = seed[c] ? 0 : -1;
}

}  // namespace c2b
