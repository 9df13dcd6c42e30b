// triangulate_kernels.hpp -- gfx950 kernel of linear midpoint triangulation (included by capi.hip only, after schur_kernels.hpp).
//
// c2b_triangulate_rows / c2b_problem_triangulate_points: a point from its cameras and observations alone, where
// every other pass refines a point that already exists.
//   * k_triangulate_points: point-major through the transpose, one lane per point walking its observations in ascending
//     index, the walk of k_normal_points and k_schur_points.  Per observation the unit ray d of the observed pixel in the
//     world frame (tri_ray: the pixel undistorted by Newton, the camera's R^T) and A += I - d d^T, b += (I - d d^T) C with C
//     the camera's centre (record doubles 24..26): six + three accumulators in registers.  X = A^-1 b is the point nearest,
//     in the sum of squared distances, to every ray's line (TriSums, tri_add).  Then tri_solve: the parallax test
//     lambda_min(A) >= 1 - cos(min_angle) (tri_lambda_max: lambda_min(A) = n - lambda_max(sum d d^T), in closed form) and
//     the 3x3 Cholesky in registers (Chol3, camera_math.hpp); and a second walk for cheirality (q.z < 0 in every usable
//     observation's camera).  One status byte per point; the point is written only when the status is kTriOk, its fourth
//     lane untouched.
//   * the five status counts: LDS integer atomics per workgroup, then at most five 64-bit integer atomics per workgroup
//     into counts[5] (zeroed by the launcher).  Integer sums carry no order dependence.
// No float atomics, no scratch memory, no robust loss; a point's sums depend on its own list alone, so the same inputs
// give the same bits.
#pragma once
#include "schur_kernels.hpp"

namespace c2b {

constexpr int kTriBlock = 256;
// C2B_TRI_* of include/city2ba_hip_experimental.h
enum { kTriOk = 0, kTriTooFew = 1, kTriDegenerate = 2, kTriBehind = 3, kTriConstant = 4, kTriKinds = 5 };

// The unit ray of the observed pixel `ob` of camera `cam` (a camblk record, or anything indexed like one); false when the
// observation is unusable (f zero or not finite, the derivative of the distortion <= 0 at a Newton iterate, a radius that
// is not finite).
//   m = ob / f, rd = |m|; rho >= 0 with rho (1 + k1 rho^2 + k2 rho^4) = rd by Newton from rho = rd, at most 16 iterations,
//   stopping when the update leaves rho unchanged (k1 == 0 && k2 == 0: rho = rd, no iteration); pn = m rho / rd (0 at rd == 0).
// The projection is p = -q.xy / q.z with the scene at q.z < 0, so the ray in the camera frame is (pn.x, pn.y, -1).  That
// much depends on the intrinsics cam[12..14] alone and is shared by triangulation and resection (resect_kernels.hpp):
//   kWorld      the ray in the world frame: the record's R is row-major, d = R^T ray, normalised (reads cam[0..8]);
//   !kWorld     the ray in the camera frame, normalised: nothing of the pose is read.
template <bool kWorld = true, typename P>
C2B_DEV bool tri_ray(P cam, const double2 ob, double &dx, double &dy, double &dz) {
    const double f = cam[12], k1 = cam[13], k2 = cam[14];
    if (f == 0.0 || !isfinite(f)) return false;
    const double mx = ob.x / f, my = ob.y / f;
    const double rd = sqrt(mx * mx + my * my);
    double rho = rd;
    if (k1 != 0.0 || k2 != 0.0) {
#pragma unroll 1
        for (int it = 0; it < 16; ++it) {
            const double r2 = rho * rho, r4 = r2 * r2;
            const double dg = (1.0 + 3.0 * k1 * r2) + 5.0 * k2 * r4;
            if (!(dg > 0.0)) return false;
            const double g = rho * ((1.0 + k1 * r2) + k2 * r4) - rd;
            const double next = rho - g / dg;
            if (next == rho) break;
            rho = next;
        }
    }
    if (!isfinite(rho)) return false;
    const double s = rd == 0.0 ? 0.0 : rho / rd;
    const double px = mx * s, py = my * s;
    if constexpr (kWorld) {
        const double wx = (cam[0] * px + cam[3] * py) - cam[6];
        const double wy = (cam[1] * px + cam[4] * py) - cam[7];
        const double wz = (cam[2] * px + cam[5] * py) - cam[8];
        const double inv = 1.0 / sqrt((wx * wx + wy * wy) + wz * wz);
        dx = wx * inv; dy = wy * inv; dz = wz * inv;
    } else {
        const double inv = 1.0 / sqrt((px * px + py * py) + 1.0);
        dx = px * inv; dy = py * inv; dz = -inv;
    }
    return true;
}

// cos(x) for x in [0, pi / 3] through sincos_kernel (its interval is [-pi/4, pi/4]: above it, cos x = sin(pi/2 - x))
C2B_DEV double tri_cos(double x) {
    const bool high = x > 0.78539816339744830962;
    double s, c;
    sincos_kernel(high ? 1.57079632679489661923 - x : x, s, c);
    return high ? s : c;
}

// The largest eigenvalue of the symmetric 3x3 M = (m00 m01 m02; . m11 m12; . . m22), in closed form (the trigonometric
// solution of the characteristic cubic): q = tr M / 3, p = sqrt(tr (M - q I)^2 / 6), r = det((M - q I) / p) / 2 in [-1, 1],
// lambda_max = q + 2 p cos(acos(r) / 3).  The largest root is the one the angle's rounding moves least: where r nears 1
// (two small eigenvalues close together, the case of a narrow bundle of rays) cos is flat.  A NaN entry gives NaN.
C2B_DEV double tri_lambda_max(double m00, double m01, double m02, double m11, double m12, double m22) {
    const double q = ((m00 + m11) + m22) / 3.0;
    const double b00 = m00 - q, b11 = m11 - q, b22 = m22 - q;
    const double p1 = (m01 * m01 + m02 * m02) + m12 * m12;
    const double p2 = ((b00 * b00 + b11 * b11) + b22 * b22) + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    if (p == 0.0) return q;                                          // a multiple of the identity
    const double ip = 1.0 / p;
    const double c00 = b00 * ip, c01 = m01 * ip, c02 = m02 * ip, c11 = b11 * ip, c12 = m12 * ip, c22 = b22 * ip;
    const double det = (c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02)) + c02 * (c01 * c12 - c11 * c02);
    const double r = fmin(fmax(0.5 * det, -1.0), 1.0);               // (fmin / fmax drop a NaN: p is NaN then, and so is the result)
    return q + 2.0 * p * tri_cos(acos(r) / 3.0);
}

// The sums over a point's usable rays: A = sum (I - d d^T) (its upper triangle), b = sum (I - d d^T) C
struct TriSums { double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0; };

// the unit ray d through the centre C joins the sums
C2B_DEV void tri_add(TriSums &s, double dx, double dy, double dz, double cx, double cy, double cz) {
    const double dc = (dx * cx + dy * cy) + dz * cz;
    s.a00 += 1.0 - dx * dx; s.a01 -= dx * dy; s.a02 -= dx * dz;
    s.a11 += 1.0 - dy * dy; s.a12 -= dy * dz; s.a22 += 1.0 - dz * dz;
    s.b0 += cx - dx * dc; s.b1 += cy - dy * dc; s.b2 += cz - dz * dc;
}

// The acceptance test and the solve over the sums of n_used rays: X = A^-1 b, true when lambda_min(A) >= one_minus_cos,
// the three pivots are positive and X is finite.  Both triangulation passes accept and solve through this routine, so a
// consensus refit is plain triangulation of its inliers bit for bit.
C2B_DEV bool tri_solve(const TriSums &s, int n_used, double one_minus_cos, double &x0, double &x1, double &x2) {
    const double n = (double)n_used;
    const double lam_min = n - tri_lambda_max(n - s.a00, -s.a01, -s.a02, n - s.a11, -s.a12, n - s.a22);
    const Chol3 L = chol3_factor(s.a00, s.a01, s.a02, s.a11, s.a12, s.a22);
    L.solve(s.b0, s.b1, s.b2, x0, x1, x2);
    const bool solved = L.positive() && isfinite(x0) && isfinite(x1) && isfinite(x2);
    return lam_min >= one_minus_cos && solved;
}

// pt_mask == NULL: no point is constant.  counts[kTriKinds] must be zero when the kernel starts.
__global__ __launch_bounds__(kTriBlock) void k_triangulate_points(
    const double *__restrict__ camblk, double4 *__restrict__ pts4, int64_t n_pts, const uint64_t *__restrict__ pt_row_ptr,
    const uint32_t *__restrict__ obs_of, const uint32_t *__restrict__ cam_of, const double2 *__restrict__ uv_obs,
    double one_minus_cos, const uint8_t *__restrict__ pt_mask, uint8_t *__restrict__ status, unsigned long long *__restrict__ counts) {
    __shared__ unsigned sCnt[kTriKinds];
    if (threadIdx.x < kTriKinds) sCnt[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * kTriBlock + threadIdx.x;
    if (p < n_pts) {
        int st = kTriConstant;
        if (!pt_mask || !pt_mask[p]) {
            const uint64_t b = pt_row_ptr[p], e = pt_row_ptr[p + 1];
            TriSums s;
            int n_used = 0;
#pragma unroll 1
            for (uint64_t j = b; j < e; ++j) {
                const uint32_t c = cam_of[j];
                double dx, dy, dz;
                if (!tri_ray(cam_ref(camblk, c), uv_obs[obs_of[j]], dx, dy, dz)) continue;
                const double *C = camblk + cam_center_at((int64_t)c);
                tri_add(s, dx, dy, dz, C[0], C[1], C[2]);
                ++n_used;
            }
            st = kTriTooFew;
            if (n_used >= 2) {
                st = kTriDegenerate;
                double x0, x1, x2;
                if (tri_solve(s, n_used, one_minus_cos, x0, x1, x2)) {
                    st = kTriOk;
#pragma unroll 1
                    for (uint64_t j = b; j < e; ++j) {
                        const CamRef cam = cam_ref(camblk, cam_of[j]);
                        double dx, dy, dz;
                        if (!tri_ray(cam, uv_obs[obs_of[j]], dx, dy, dz)) continue;
                        const double qz = dot3(cam[6], cam[7], cam[8], x0, x1, x2) + cam[11];
                        if (qz >= 0.0) st = kTriBehind;
                    }
                    if (st == kTriOk) {
                        double2 *out = reinterpret_cast<double2 *>(pts4 + p);       // x y | z w: the fourth lane keeps its value
                        out[0] = make_double2(x0, x1);
                        reinterpret_cast<double *>(out + 1)[0] = x2;
                    }
                }
            }
        }
        status[p] = (uint8_t)st;
        atomicAdd(&sCnt[st], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kTriKinds && sCnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)sCnt[threadIdx.x]);
}

}  // namespace c2b
