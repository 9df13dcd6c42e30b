// scan_kernels.hpp -- every exclusive prefix sum of the library: one wave / workgroup primitive, one chunk loop, one
// single-workgroup kernel, one tiled path and their launchers (DESIGN: "Scans and bucket fills").  Integers only, so every
// form gives the same numbers; a caller picks the short or the tiled form by the length of its array.
//
//   wave_excl_scan / block_excl_scan   one value per lane of a wave / per thread of a workgroup of kScanBlock
//   block_scan_array                   a whole array by one workgroup, kScanBlock elements a trip, the carry in a register
//   k_scan_short<In, Out>              that loop as a kernel: out[i] = first + in[0] + ... + in[i - 1], *total = first + all
//   scan_short / scan_tiled            the launchers, asynchronous and unchecked like any launch in a sequence; scan_tiled
//                                      is k_scan_tiles, k_scan_short over the tile sums, k_scan_add
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace c2b {

constexpr int kScanBlock = 256;                 // threads of every scanning workgroup
constexpr int kScanPer = 4;                     // elements per thread of the tiled path
constexpr int kScanTile = kScanBlock * kScanPer;

// inclusive scan over the 64 lanes of a wave (T: int, uint32_t or uint64_t)
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive scan over a wave; total = the wave's sum (every lane).  No LDS, no barrier: usable in divergent waves
template <class T>
__device__ __forceinline__ T wave_excl_scan(T v, int lane, T &total) {
    const T inc = wave_incl_scan(v, lane);
    total = __shfl(inc, 63, 64);
    return inc - v;
}

// exclusive scan of one value per thread over a workgroup of kScanBlock threads; total = the workgroup's sum (every
// thread).  sWave: kScanBlock / 64 words of LDS, free again only after the caller's next barrier
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T *sWave, T &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v, lane);
    if (lane == 63) sWave[wave] = inc;
    __syncthreads();
    T base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanBlock / 64; ++w) {
        const T s = sWave[w];
        if (w < wave) base += s;
        all += s;
    }
    total = all;
    return base + inc - v;
}

// The chunk loop of one workgroup of kScanBlock threads over in[0, n): out[i] = first + in[0] + ... + in[i - 1]; returns
// first + every element (every thread).  May run in place (in == out): a thread reads and writes its own element only.
template <class In, class Out>
__device__ __forceinline__ Out block_scan_array(const In *in, int64_t n, Out first, Out *out, Out *sWave) {
    Out carry = first;
    for (int64_t base = 0; base < n; base += kScanBlock) {          // workgroup-uniform
        const int64_t i = base + threadIdx.x;
        const Out v = i < n ? (Out)in[i] : (Out)0;
        Out chunk;
        const Out ex = block_excl_scan(v, sWave, chunk);
        if (i < n) out[i] = carry + ex;
        carry += chunk;
        __syncthreads();                                            // sWave is read; the next trip may write it
    }
    return carry;
}

// one workgroup.  total may be out + n: the row-pointer form, out[0 .. n]
template <class In, class Out>
__global__ __launch_bounds__(kScanBlock) void k_scan_short(const In *in, int64_t n, Out first, Out *out, Out *total) {
    __shared__ Out sWave[kScanBlock / 64];
    const Out all = block_scan_array(in, n, first, out, sWave);
    if (threadIdx.x == 0) *total = all;
}

// ---- the tiled path: a tile's own exclusive scan + its sum, the scan of the sums, the sums added back -----------------
template <class In, class Out>
__global__ __launch_bounds__(kScanBlock) void k_scan_tiles(const In *__restrict__ in, int64_t n, Out *__restrict__ out,
                                                          Out *__restrict__ tile_sum) {
    __shared__ Out sWave[kScanBlock / 64];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    Out f[kScanPer], s = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) { f[k] = base + k < n ? (Out)in[base + k] : (Out)0; s += f[k]; }
    Out total;
    Out ex = block_excl_scan(s, sWave, total);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (base + k < n) out[base + k] = ex;
        ex += f[k];
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

template <class Out>
__global__ __launch_bounds__(kScanBlock) void k_scan_add(Out *__restrict__ out, int64_t n, const Out *__restrict__ tile_off) {
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    const Out off = tile_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanPer; ++k)
        if (base + k < n) out[base + k] += off;
}

// ---- launchers ------------------------------------------------------------------------------------------------------
// elements of Out a scan_tiled over n elements needs as scratch
inline size_t scan_scratch_count(int64_t n) { return (size_t)(n / kScanTile + 2); }

// for arrays of a few thousand elements (cameras): one launch, kScanBlock elements a trip
template <class In, class Out>
inline void scan_short(hipStream_t st, const In *in, int64_t n, Out first, Out *out, Out *total) {
    hipLaunchKernelGGL((k_scan_short<In, Out>), dim3(1), dim3(kScanBlock), 0, st, in, n, first, out, total);
}

// for anything longer (points, cells, observations, histograms, text tiles): three launches, the middle one short
template <class In, class Out>
inline void scan_tiled(hipStream_t st, const In *in, int64_t n, Out first, Out *out, Out *total, Out *scratch) {
    const int64_t tiles = (n + kScanTile - 1) / kScanTile;
    if (n > 0) hipLaunchKernelGGL((k_scan_tiles<In, Out>), dim3((unsigned)tiles), dim3(kScanBlock), 0, st, in, n, out, scratch);
    scan_short(st, (const Out *)scratch, tiles, first, scratch, total);
    if (n > 0) hipLaunchKernelGGL((k_scan_add<Out>), dim3((unsigned)tiles), dim3(kScanBlock), 0, st, out, n, (const Out *)scratch);
}

}  // namespace c2b
