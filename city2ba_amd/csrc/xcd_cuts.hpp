// The step kernel's workgroup -> tile map for its 512-thread x 2-tile shape: eight contiguous ranges of the tile list, one per XCD,
// cut by the XCDs' measured rates instead of in equal eighths (docs/log_r07.md).
//
// The hardware deals workgroups to the eight XCDs round-robin (workgroups b and b + 8 share one), so the split of a one-shot grid
// over the XCDs is static, and the launch ends when the slowest XCD ends.  Measured with a per-workgroup time-stamp probe on two
// devices: the XCDs with an odd id run this store-bound kernel ~9 % slower per workgroup than the even ones from the first
// microsecond to the last (whichever eighth of the list they are given: the rate follows the XCD, not the data), so with equal
// eighths the four even XCDs idle for the launch's last 65-95 of ~700 us.  The map therefore gives the odd XCDs less:
// kXcdOddShare : kXcdEvenShare.  A pure function of blockIdx.x and launch constants -- no atomics, no persistent loop, workgroups
// stay one-shot, and a launch of a given size always has the same grid (the error fold's "same grid => same bits").
//
// Plain C++ (the host tests compile this header on its own); the kernel and its launcher include it too.
#pragma once

#if defined(__HIPCC__)
#define C2B_XCD_HD __host__ __device__ __forceinline__
#else
#define C2B_XCD_HD inline
#endif

namespace c2b {

struct XcdCuts { int cut[9]; };                 // XCD x streams the workgroup tiles [cut[x], cut[x + 1]); cut[0] = 0, cut[8] = all of them

constexpr int kXcdEvenShare = 11, kXcdOddShare = 9;

// Cuts for n_tiles workgroup tiles with XCD x weighted share[x & 1]: every range gets the floor of its share and the (< 8) tiles
// left over go one each to the first ranges -- with equal shares exactly the ranges of xcd_tile32.  Returns the grid that covers
// them: 8 x the longest range (the workgroups past a shorter range's end only fold).
inline int xcd_cuts_make(int n_tiles, int even_share, int odd_share, XcdCuts &m) {
    const long long total = 4ll * (even_share + odd_share);
    int len[8], used = 0, longest = 0;
    for (int x = 0; x < 8; ++x) {
        len[x] = (int)((long long)n_tiles * ((x & 1) ? odd_share : even_share) / total);
        used += len[x];
    }
    m.cut[0] = 0;
    for (int x = 0; x < 8; ++x) {
        if (x < n_tiles - used) ++len[x];
        m.cut[x + 1] = m.cut[x] + len[x];
        if (len[x] > longest) longest = len[x];
    }
    return 8 * longest;
}

// the workgroup tile of workgroup `bid`, or -1 past the end of its XCD's range
C2B_XCD_HD int xcd_cut_tile(int bid, const XcdCuts &m) {
    const int xcd = bid & 7, k = bid >> 3;
    const int lo = m.cut[xcd];
    return k < m.cut[xcd + 1] - lo ? lo + k : -1;
}

}  // namespace c2b
