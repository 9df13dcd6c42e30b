// Host side of the similarity alignment: Umeyama's closed form from the centred moments the device passes sum
// (align_kernels.hpp), and the checks a caller's similarity has to pass before it is applied.  Plain C++ on a handful of doubles -- the
// 3x3 singular value decomposition is a one-sided Jacobi iteration, no LAPACK -- so the CPU suite holds it without a device.
#pragma once

#include <cmath>
#include <cstdint>
#include <utility>

namespace c2b_host {

struct Similarity { double s, R[9], t[3]; };            // y = s R x + t, R row-major

inline Similarity similarity_identity() { return Similarity{1.0, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}}; }

constexpr int kAlignOk = 0, kAlignTooFew = 1, kAlignDegenerate = 2;
constexpr double kAlignRankTol = 1e-12;                  // second singular value <= this x the first: collinear

// A (row-major 3x3) = U diag(sig) V^T with sig[0] >= sig[1] >= sig[2] >= 0, U and V orthonormal to rounding, both row-major.
// One-sided Jacobi (Hestenes): plane rotations from the right make the columns of B = A V mutually orthogonal; their lengths are
// the singular values.  U's first two columns are B's, normalised; the third is their cross product with the sign of B's third
// column, so U is orthonormal also where sig[2] is zero (a planar cloud) and its column carries no direction.
inline void svd3(const double A[9], double U[9], double sig[3], double V[9]) {
    double B[9], W[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) B[k] = A[k];
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double a = 0, b = 0, c = 0;
                for (int r = 0; r < 3; ++r) { a += B[3 * r + p] * B[3 * r + p]; b += B[3 * r + q] * B[3 * r + q]; c += B[3 * r + p] * B[3 * r + q]; }
                if (c == 0.0 || std::fabs(c) <= 0x1.0p-54 * std::sqrt(a) * std::sqrt(b)) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 3; ++r) {
                    const double bp = B[3 * r + p], bq = B[3 * r + q];
                    B[3 * r + p] = cs * bp - sn * bq; B[3 * r + q] = sn * bp + cs * bq;
                    const double wp = W[3 * r + p], wq = W[3 * r + q];
                    W[3 * r + p] = cs * wp - sn * wq; W[3 * r + q] = sn * wp + cs * wq;
                }
            }
        if (!rotated) break;
    }
    double len[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) len[j] = std::sqrt(B[j] * B[j] + B[3 + j] * B[3 + j] + B[6 + j] * B[6 + j]);
    for (int i = 0; i < 2; ++i)                           // descending, stable
        for (int j = 0; j < 2 - i; ++j)
            if (len[ord[j]] < len[ord[j + 1]]) std::swap(ord[j], ord[j + 1]);
    for (int j = 0; j < 3; ++j) {
        sig[j] = len[ord[j]];
        for (int r = 0; r < 3; ++r) V[3 * r + j] = W[3 * r + ord[j]];
    }
    auto unit = [](double *v) {
        const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (n > 0.0) { v[0] /= n; v[1] /= n; v[2] /= n; }
    };
    double u0[3], u1[3], u2[3], b2[3];
    for (int r = 0; r < 3; ++r) { u0[r] = B[3 * r + ord[0]]; u1[r] = B[3 * r + ord[1]]; b2[r] = B[3 * r + ord[2]]; }
    unit(u0);
    const double d01 = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];       // one Gram-Schmidt step: a no-op to rounding after convergence
    for (int r = 0; r < 3; ++r) u1[r] -= d01 * u0[r];
    unit(u1);
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    unit(u2);
    if (u2[0] * b2[0] + u2[1] * b2[1] + u2[2] * b2[2] < 0.0) { u2[0] = -u2[0]; u2[1] = -u2[1]; u2[2] = -u2[2]; }
    for (int r = 0; r < 3; ++r) { U[3 * r] = u0[r]; U[3 * r + 1] = u1[r]; U[3 * r + 2] = u2[r]; }
}

inline double det3(const double M[9]) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Umeyama (1991): n correspondences with means mean_x, mean_y, var_x = sum |x - mean_x|^2 / n and cov (row-major) =
// sum (y - mean_y)(x - mean_x)^T / n.  R = U diag(1, 1, d) V^T with d = det(U V^T); s = (sig0 + sig1 + d sig2) / var_x, or 1 when
// with_scale is off; t = mean_y - s R mean_x.  Returns the status; on a failure T is the identity.
inline int similarity_from_moments(int64_t n, const double mean_x[3], const double mean_y[3], double var_x, const double cov[9],
                                   bool with_scale, Similarity &T) {
    T = similarity_identity();
    if (n < 3) return kAlignTooFew;
    if (!(var_x > 0.0)) return kAlignDegenerate;
    double U[9], V[9], sig[3];
    svd3(cov, U, sig, V);
    if (!(sig[1] > kAlignRankTol * sig[0])) return kAlignDegenerate;
    const double d = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T.R[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + d * (U[3 * r + 2] * V[3 * c + 2]);
    T.s = with_scale ? ((sig[0] + sig[1]) + d * sig[2]) / var_x : 1.0;
    for (int r = 0; r < 3; ++r)
        T.t[r] = mean_y[r] - T.s * ((T.R[3 * r] * mean_x[0] + T.R[3 * r + 1] * mean_x[1]) + T.R[3 * r + 2] * mean_x[2]);
    return kAlignOk;
}

// What the device passes leave (k_align_means: count and sums; k_align_moments: the sums about the pivot, the residual sums, the
// pivot) moved from the pivot to the mean: mean = pivot + residual / n, and every moment loses n d d^T of the residual means d.
inline void align_finish_moments(const double means[7], const double mom[23], double *n, double mean_x[3], double mean_y[3], double *var_x,
                                 double *var_y, double cov[9]) {
    const double cnt = means[0];
    *n = cnt;
    double dx[3] = {0, 0, 0}, dy[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        if (cnt > 0.0) { dx[k] = mom[11 + k] / cnt; dy[k] = mom[14 + k] / cnt; }
        mean_x[k] = cnt > 0.0 ? mom[17 + k] + dx[k] : 0.0;
        mean_y[k] = cnt > 0.0 ? mom[20 + k] + dy[k] : 0.0;
    }
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;
    *var_x = (mom[0] - cnt * (dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2])) * inv;
    *var_y = (mom[1] - cnt * (dy[0] * dy[0] + dy[1] * dy[1] + dy[2] * dy[2])) * inv;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) cov[3 * r + c] = (mom[2 + 3 * r + c] - cnt * (dy[r] * dx[c])) * inv;
}

// a similarity a caller may apply: finite, s > 0, |R^T R - I|_F <= 1e-9, det R > 0.  NULL, or what is wrong with it.
inline const char *similarity_defect(const Similarity &T) {
    if (!std::isfinite(T.s)) return "the scale is not finite";
    for (int k = 0; k < 9; ++k) if (!std::isfinite(T.R[k])) return "the rotation is not finite";
    for (int k = 0; k < 3; ++k) if (!std::isfinite(T.t[k])) return "the translation is not finite";
    if (!(T.s > 0.0)) return "the scale must be > 0";
    double f = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double g = (T.R[a] * T.R[b] + T.R[3 + a] * T.R[3 + b]) + T.R[6 + a] * T.R[6 + b] - (a == b ? 1.0 : 0.0);
            f += g * g;
        }
    if (!(std::sqrt(f) <= 1e-9)) return "the rotation is not orthonormal (|R^T R - I|_F > 1e-9)";
    if (!(det3(T.R) > 0.0)) return "the rotation is a reflection (det < 0)";
    return nullptr;
}

}  // namespace c2b_host
