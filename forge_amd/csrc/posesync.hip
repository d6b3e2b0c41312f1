// posesync.hip — camera synchronisation of the evaluation protocol (kubric_eval.py:95-145 `sync_pose` -> utils/sync_utils.py:76-191
// `camera_synchronization(..., so3_projection=True, normalize_confidences=True, double=True)`): the pairwise extrinsics of N views and their
// confidences are laid into the 4N x 4N matrix L, L is raised to the power 2^squares, the block column of one view is divided by its mass
// entries and every 3x3 rotation block is projected onto SO(3).
// One workgroup per batch element; L and its square live in LDS as float64 images. Float64 from the first load on (the reference forms L in
// float32 and widens it afterwards). Every output element of a product is one FMA chain over k in ascending order: no atomics, no allocation,
// no host synchronisation, bitwise reproducible, and independent of the batch size. Plain FMAs, no matrix cores: the launch is ten dependent
// products of at most 32^3, latency-bound whatever computes them.
#include <cmath>

#include "common.h"
#include "so3.h"

namespace forge {

constexpr int PS_MAXN = 8;              // views
constexpr int PS_MAXM = 4 * PS_MAXN;    // rows of L
constexpr int PS_THREADS = 256;

__device__ __forceinline__ bool ps_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and +-inf

__global__ __launch_bounds__(PS_THREADS) void pose_sync_kernel(const float* __restrict__ P, const float* __restrict__ conf, const int* __restrict__ pairs,
                                                               int N, int E, int squares, int center, double rank_tol, float* __restrict__ out,
                                                               double* __restrict__ sv, int* __restrict__ status) {
    __shared__ double La[PS_MAXM * PS_MAXM], Lb[PS_MAXM * PS_MAXM];
    __shared__ double cm[PS_MAXN][PS_MAXN];       // confidence matrix, then column-normalised
    __shared__ double colsum[PS_MAXN];
    __shared__ int bad_input, view_bits[PS_MAXN];
    const int b = blockIdx.x, tid = threadIdx.x, M = 4 * N;
    const float* Pb = P + (long long)b * E * 16;
    const float* cb = conf + (long long)b * E;

    for (int i = tid; i < M * M; i += PS_THREADS) La[i] = 0.0;
    if (tid < PS_MAXN * PS_MAXN) cm[tid / PS_MAXN][tid % PS_MAXN] = 0.0;
    if (tid < PS_MAXN) view_bits[tid] = 0;
    if (tid == 0) bad_input = 0;
    __syncthreads();

    bool bad = false;
    for (int i = tid; i < E * 16; i += PS_THREADS) bad |= !ps_finite((double)Pb[i]);
    for (int i = tid; i < E; i += PS_THREADS) bad |= !ps_finite((double)cb[i]);
    if (bad) bad_input = 4;                       // every writer stores the same value
    if (tid == 0) {                               // the diagonal sums in edge order, as the reference adds them
        for (int e = 0; e < E; ++e) {
            const int i = pairs[2 * e], j = pairs[2 * e + 1];
            if (i < 0 || j < 0 || i >= N || j >= N || i == j) continue;      // memory safety only: ops.pose_sync refuses such lists
            const double c = (double)cb[e];
            cm[i][j] = c;
            cm[j][i] = c;
            cm[i][i] += c / 2;
            cm[j][j] += c / 2;
        }
    }
    __syncthreads();
    if (tid < N) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += cm[i][tid];
        colsum[tid] = s < 1e-9 ? 1e-9 : s;        // clamp(min=1e-9); NaN stays NaN
    }
    __syncthreads();
    if (tid < PS_MAXN * PS_MAXN && tid / PS_MAXN < N && tid % PS_MAXN < N) cm[tid / PS_MAXN][tid % PS_MAXN] /= colsum[tid % PS_MAXN];
    __syncthreads();

    // L[i][i] = conf_ii I, L[i][j] = conf_ij inverse(P_ij), L[j][i] = conf_ji P_ij (SE3_inverse: R^T, -R^T t, P's own bottom row)
    if (tid < M) La[tid * M + tid] = cm[tid / 4][tid / 4];
    for (int x = tid; x < E * 16; x += PS_THREADS) {
        const int e = x >> 4, r = (x >> 2) & 3, c = x & 3;
        const int i = pairs[2 * e], j = pairs[2 * e + 1];
        if (i < 0 || j < 0 || i >= N || j >= N || i == j) continue;
        const float* p = Pb + e * 16;
        La[(4 * j + r) * M + 4 * i + c] = cm[j][i] * (double)p[r * 4 + c];
        double v;
        if (r < 3 && c < 3) v = (double)p[c * 4 + r];
        else if (r < 3) v = fma(-(double)p[8 + r], (double)p[11], fma(-(double)p[4 + r], (double)p[7], -(double)p[r] * (double)p[3]));
        else v = (double)p[12 + c];
        La[(4 * i + r) * M + 4 * j + c] = cm[i][j] * v;
    }
    __syncthreads();

    double* A = La;
    double* C = Lb;
    for (int q = 0; q < squares; ++q) {           // C = A A, every element one FMA chain over ascending k
        for (int x = tid; x < M * M; x += PS_THREADS) {
            const int r = x / M, c = x - r * M;
            double acc = 0.0;
            for (int k = 0; k < M; ++k) acc = fma(A[r * M + k], A[k * M + c], acc);
            C[x] = acc;
        }
        __syncthreads();
        double* t = A;
        A = C;
        C = t;
    }

    if (tid < N) {                                // one thread per view: its block of the kept block column
        const int v = tid;
        double g[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) g[r][c] = A[(4 * v + r) * M + 4 * center + c];
        const double mass = g[3][3];
        int bits = (mass > 0.0) ? 0 : 1;          // mass <= 0 (the reference's assertion); NaN counts
        const double div = mass < 1e-9 ? 1e-9 : mass;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) g[r][c] /= div;
        double G[3][3], R[3][3], s[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) G[r][c] = g[r][c];
        ps_project_so3(G, R, s);
        if (!(s[0] > 0.0) || !(s[2] / s[0] >= rank_tol)) bits |= 2;
        float* o = out + ((long long)b * N + v) * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) o[r * 4 + c] = (float)((r < 3 && c < 3) ? R[r][c] : g[r][c]);
        if (sv != nullptr) {
            double* so = sv + ((long long)b * N + v) * 3;
            so[0] = s[0];
            so[1] = s[1];
            so[2] = s[2];
        }
        view_bits[v] = bits;
    }
    __syncthreads();
    if (tid == 0) {
        int bits = bad_input;
        for (int v = 0; v < N; ++v) bits |= view_bits[v];
        status[b] = bits;
    }
}

}  // namespace forge

extern "C" int forge_pose_sync(const float* P, const float* conf, const int* pairs, int B, int N, int E, int squares, int center, double rank_tol,
                               float* out, double* sv, int* status, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(P && conf && pairs && out && status, FORGE_EINVAL, "forge_pose_sync: null pointer (only sv may be null)");
    FORGE_REQUIRE(B >= 1, FORGE_EINVAL, "forge_pose_sync: B=%d must be positive", B);
    FORGE_REQUIRE(N >= 3 && N <= PS_MAXN, FORGE_ESHAPE, "forge_pose_sync: N=%d outside 3..%d (two views are plain chaining)", N, PS_MAXN);
    FORGE_REQUIRE(E >= N - 1 && E <= N * (N - 1) / 2, FORGE_ESHAPE, "forge_pose_sync: E=%d outside N-1..N(N-1)/2 = %d..%d", E, N - 1, N * (N - 1) / 2);
    FORGE_REQUIRE(squares >= 1 && squares <= 16, FORGE_EINVAL, "forge_pose_sync: squares=%d outside 1..16", squares);
    FORGE_REQUIRE(center >= 0 && center < N, FORGE_EINVAL, "forge_pose_sync: center=%d outside 0..%d", center, N - 1);
    FORGE_REQUIRE(rank_tol >= 0.0 && rank_tol < 1.0, FORGE_EINVAL, "forge_pose_sync: rank_tol=%g outside [0, 1)", rank_tol);
    hipLaunchKernelGGL(pose_sync_kernel, dim3(B), dim3(PS_THREADS), 0, (hipStream_t)stream, P, conf, pairs, N, E, squares, center, rank_tol, out, sv,
                       status);
    FORGE_LAUNCH_CHECK("forge_pose_sync");
    return 0;
}
