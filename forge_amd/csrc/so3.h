// so3.h — the float64 projection of a 3x3 matrix onto SO(3), written once (header only: no translation unit). posesync.hip projects the rotation
// blocks of the synchronised cameras with it, align.hip solves the Kabsch rotation of a cross-covariance with it: U diag(1, 1, det(U V^T)) V^T is
// both. One-sided Jacobi (Hestenes) on the columns, a fixed number of sweeps, no branch on data beyond the rotation threshold: every caller keeps
// its bits.
#pragma once
#include <cmath>

#include "common.h"

namespace forge {

constexpr int PS_SWEEPS = 12;           // one-sided Jacobi sweeps of a 3x3 block: converged (quadratically) after 5 or 6, the rest are no-ops

// Rotate columns p, q of a (and of v) so that they become orthogonal (Hestenes). Nothing happens when they already are, or on NaN.
__device__ __forceinline__ void ps_rotate(double (&ap)[3], double (&aq)[3], double (&vp)[3], double (&vq)[3]) {
    const double alpha = fma(ap[0], ap[0], fma(ap[1], ap[1], ap[2] * ap[2]));
    const double beta = fma(aq[0], aq[0], fma(aq[1], aq[1], aq[2] * aq[2]));
    const double gamma = fma(ap[0], aq[0], fma(ap[1], aq[1], ap[2] * aq[2]));
    if (!(fabs(gamma) > 1e-17 * sqrt(alpha * beta))) return;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
    const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = c * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double x = ap[r], y = aq[r];
        ap[r] = c * x - s * y;
        aq[r] = s * x + c * y;
        const double u = vp[r], w = vq[r];
        vp[r] = c * u - s * w;
        vq[r] = s * u + c * w;
    }
}

__device__ __forceinline__ void ps_swap3(double (&a)[3], double (&b)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double x = a[r];
        a[r] = b[r];
        b[r] = x;
    }
}

__device__ __forceinline__ void ps_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// A unit vector orthogonal to the unit vector a (a's smallest component is crossed out); finite for any finite a.
__device__ __forceinline__ void ps_any_orthogonal(const double (&a)[3], double (&o)[3]) {
    const double x = fabs(a[0]), y = fabs(a[1]), z = fabs(a[2]);
    double e[3] = {0.0, 0.0, 0.0};
    if (x <= y && x <= z) e[0] = 1.0; else if (y <= z) e[1] = 1.0; else e[2] = 1.0;
    ps_cross(a, e, o);
    const double n = sqrt(fma(o[0], o[0], fma(o[1], o[1], o[2] * o[2])));
    if (n > 0.0) {
        o[0] /= n; o[1] /= n; o[2] /= n;
    } else {
        o[0] = 0.0; o[1] = 1.0; o[2] = 0.0;
    }
}

// g [3][3] row-major -> its projection onto SO(3), U diag(1, 1, det(U V^T)) V^T of the SVD g = U S V^T with S descending (torch.svd's order, so
// the sign lands on the smallest singular value), and the singular values s[0] >= s[1] >= s[2]. With u_k, v_k the k-th singular vectors the
// projection is u_0 v_0^T + u_1 v_1^T + (u_0 x u_1)(v_0 x v_1)^T: the one rotation that maps v_0, v_1 to u_0, u_1. It never needs u_2, which
// does not exist when s[2] = 0. Where s[0] or s[1] is 0 the missing direction is replaced by an arbitrary orthogonal one: the result stays a
// finite rotation and the caller reports the block as undetermined.
__device__ void ps_project_so3(const double (&g)[3][3], double (&R)[3][3], double (&s)[3]) {
    double a0[3] = {g[0][0], g[1][0], g[2][0]}, a1[3] = {g[0][1], g[1][1], g[2][1]}, a2[3] = {g[0][2], g[1][2], g[2][2]};   // columns
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < PS_SWEEPS; ++sweep) {
        ps_rotate(a0, a1, v0, v1);
        ps_rotate(a0, a2, v0, v2);
        ps_rotate(a1, a2, v1, v2);
    }
    s[0] = sqrt(fma(a0[0], a0[0], fma(a0[1], a0[1], a0[2] * a0[2])));
    s[1] = sqrt(fma(a1[0], a1[0], fma(a1[1], a1[1], a1[2] * a1[2])));
    s[2] = sqrt(fma(a2[0], a2[0], fma(a2[1], a2[1], a2[2] * a2[2])));
    // descending order with three compare-swaps on static indices (NaN compares false: nothing moves)
    if (s[0] < s[1]) { const double x = s[0]; s[0] = s[1]; s[1] = x; ps_swap3(a0, a1); ps_swap3(v0, v1); }
    if (s[1] < s[2]) { const double x = s[1]; s[1] = s[2]; s[2] = x; ps_swap3(a1, a2); ps_swap3(v1, v2); }
    if (s[0] < s[1]) { const double x = s[0]; s[0] = s[1]; s[1] = x; ps_swap3(a0, a1); ps_swap3(v0, v1); }
    double u0[3], u1[3], u2[3], w2[3];
    if (s[0] > 0.0) {
        u0[0] = a0[0] / s[0]; u0[1] = a0[1] / s[0]; u0[2] = a0[2] / s[0];
    } else {
        u0[0] = (s[0] == 0.0) ? 1.0 : s[0]; u0[1] = 0.0; u0[2] = 0.0;         // zero block: any direction; NaN stays NaN
    }
    if (s[1] > 0.0) {
        u1[0] = a1[0] / s[1]; u1[1] = a1[1] / s[1]; u1[2] = a1[2] / s[1];
        // a1 is orthogonal to a0 only up to the sweeps' threshold relative to |a0| |a1|: re-orthogonalise the weaker direction
        const double d = fma(u0[0], u1[0], fma(u0[1], u1[1], u0[2] * u1[2]));
        u1[0] -= d * u0[0]; u1[1] -= d * u0[1]; u1[2] -= d * u0[2];
        const double n = sqrt(fma(u1[0], u1[0], fma(u1[1], u1[1], u1[2] * u1[2])));
        if (n > 0.0) { u1[0] /= n; u1[1] /= n; u1[2] /= n; }
    } else if (s[1] == 0.0) {
        ps_any_orthogonal(u0, u1);
    } else {
        u1[0] = s[1]; u1[1] = s[1]; u1[2] = s[1];
    }
    ps_cross(u0, u1, u2);
    ps_cross(v0, v1, w2);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = fma(u0[r], v0[c], fma(u1[r], v1[c], u2[r] * w2[c]));
}

}  // namespace forge
