// subset_kernels.hpp -- a sub-problem cut out of the resident problem and put back: the point map of a
// caller's selection, the marking passes of a window, the lists and roles after the flag scans, the policies that make the
// row compaction of kernels.hpp read its rows through a camera list and renumber its points, and the write-back scatters.
// Integers and copies only: no float arithmetic, no float atomics, so the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace c2b {

// ---- policies of k_keep_row_counts / k_keep_row_scatter (kernels.hpp) ---------------------------------------------------
struct RowVia {                                               // row c of the child is row cam_of[c] of the parent
    const uint32_t *__restrict__ cam_of;
    __device__ __forceinline__ int64_t row(int64_t c) const { return (int64_t)cam_of[c]; }
};
struct KeepMapped {                                           // an entry stays when its point has a slot, and names that slot
    const int32_t *__restrict__ new_of;
    __device__ __forceinline__ bool kept(uint64_t i, const uint32_t *pt_in) const { return new_of[pt_in[i]] >= 0; }
    __device__ __forceinline__ uint32_t index(uint32_t pt) const { return (uint32_t)new_of[pt]; }
};

// ---- the point map of subset: new_of[pt_sel[i]] = i, the LAST slot of a repeated point (HashMap::from_iter) -------------
// new_of starts at -1 everywhere; the integer maximum makes the winner independent of the order the threads arrive in
__global__ __launch_bounds__(256) void k_subset_point_map(const uint32_t *__restrict__ pt_sel, int64_t n_sel, int32_t *__restrict__ new_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_sel) atomicMax(&new_of[pt_sel[i]], (int32_t)i);
}

// ---- window marking: one thread per observation; every racing store writes the same value -------------------------------
// cam_flag[c] = seed[c] != 0, before the passes
__global__ __launch_bounds__(256) void k_window_seed_flags(const uint8_t *__restrict__ seed, int64_t n_cam, uint32_t *__restrict__ cam_flag) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n_cam) cam_flag[c] = seed[c] ? 1u : 0u;
}

// (a) in_P[pt] = 1 where the camera is a seed
__global__ __launch_bounds__(256) void k_window_mark_points(const uint32_t *__restrict__ cam_idx, const uint32_t *__restrict__ pt_idx,
                                                           int64_t n_obs, const uint8_t *__restrict__ seed, uint32_t *__restrict__ in_P) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o < n_obs && seed[cam_idx[o]]) in_P[pt_idx[o]] = 1u;
}

// (b) where the camera is not a seed and the point is in P: the camera is a halo camera (HALO; cam_flag gains it), or the
// point is shared
template <bool HALO>
__global__ __launch_bounds__(256) void k_window_mark_rim(const uint32_t *__restrict__ cam_idx, const uint32_t *__restrict__ pt_idx,
                                                        int64_t n_obs, const uint8_t *__restrict__ seed, const uint32_t *__restrict__ in_P,
                                                        uint32_t *__restrict__ cam_flag, uint8_t *__restrict__ shared) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    const uint32_t c = cam_idx[o], q = pt_idx[o];
    if (seed[c] || !in_P[q]) return;
    if (HALO) cam_flag[c] = 1u;
    else shared[q] = 1;
}

// after the flag scans: cam_of / pt_of (ascending parent index), the roles and the point map; one thread per camera or point
__global__ __launch_bounds__(256) void k_window_lists(const uint32_t *__restrict__ cam_flag, const uint32_t *__restrict__ cam_pos, int64_t n_cam,
                                                     const uint8_t *__restrict__ seed, const uint32_t *__restrict__ in_P,
                                                     const uint32_t *__restrict__ pt_pos, int64_t n_pts, const uint8_t *__restrict__ shared,
                                                     uint32_t *__restrict__ cam_of, uint8_t *__restrict__ cam_role, uint32_t *__restrict__ pt_of,
                                                     uint8_t *__restrict__ pt_role, int32_t *__restrict__ new_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_cam && cam_flag[i]) {
        cam_of[cam_pos[i]] = (uint32_t)i;
        cam_role[cam_pos[i]] = seed[i] ? 0 : 1;
    }
    if (i < n_pts) {
        const bool in = in_P[i] != 0;
        new_of[i] = in ? (int32_t)pt_pos[i] : -1;
        if (in) {
            pt_of[pt_pos[i]] = (uint32_t)i;
            pt_role[pt_pos[i]] = shared[i];
        }
    }
}

// ---- write-back: the child's free entries over the parent's, by the origin lists ----------------------------------------
// parent.bal9[9 cam_of[c] + k] = child.bal9[9 c + k] where bit k of the child's mask word is clear (cmask NULL: every bit)
__global__ __launch_bounds__(256) void k_scatter_free_cameras(const double *__restrict__ child_bal9, const uint32_t *__restrict__ cam_of,
                                                             const uint16_t *__restrict__ cmask, int64_t n_child, double *__restrict__ parent_bal9) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * n_child) return;
    const int64_t c = i / 9;
    const int k = (int)(i - 9 * c);
    if (cmask && ((cmask[c] >> k) & 1)) return;
    parent_bal9[9 * (int64_t)cam_of[c] + k] = child_bal9[i];
}

// xyz of the points whose byte is clear (pmask NULL: all); the fourth lane of the parent's row is untouched (a double2 and a
// scalar store, as k_triangulate_points writes a point)
__global__ __launch_bounds__(256) void k_scatter_free_points(const double4 *__restrict__ child_pts4, const uint32_t *__restrict__ pt_of,
                                                            const uint8_t *__restrict__ pmask, int64_t n_child, double4 *__restrict__ parent_pts4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_child || (pmask && pmask[i])) return;
    const double4 v = child_pts4[i];
    double *row = reinterpret_cast<double *>(parent_pts4 + pt_of[i]);
    *reinterpret_cast<double2 *>(row) = make_double2(v.x, v.y);
    row[2] = v.z;
}

}  // namespace c2b
