// align.hip — estimating the similarity that maps one point set onto another (include/forge_hip.h section g5 states the contract): the closed-form
// least-squares fit of Umeyama / Kabsch from float64 moments, as one step of an ICP whose correspondences come from forge_nn_points, and the choice
// among several starts. No atomics, no allocation, nothing read back: every entry can sit in a captured graph, and every bit of every output is
// reproducible and independent of the batch.
//
// forge_align_step is two launches. The first, grid (ALIGN_BLOCKS, B) x 256 threads, strides over the rows of a pair and leaves ALIGN_PARTIAL float64
// sums per workgroup (the fixed tree of geom_common.h); the second, one workgroup per pair, adds the partials in workgroup order (one thread per
// sum), and thread 0 solves: cross-covariance, its projection onto SO(3) (so3.h: the SVD pose synchronisation uses, not a second one), scale,
// translation, residual statistics, the rejection threshold of the NEXT step, and the convergence test. The moments are those of the UNTRANSFORMED
// queries, so a step solves for the whole transform q -> p and nothing is composed in fp32 from one iteration to the next. A pair that has
// converged is frozen on the device (both launches leave at once), so the caller's loop has no host decision in it.
// The moments pass reads 12 (q) + 4 (idx) + 4 (d2) + 12 (gathered p) bytes per row: 3.2 MB at 1e5 rows, against the 1e10 pairs of the search that
// produced idx (tools/align_probe.py, profiles/r28_align_probe.txt, has both times).
#include "geom_common.h"
#include "so3.h"

namespace forge {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_BLOCKS = 64;                   // workgroups per pair of the moments pass
// per-workgroup partial: n_in | n_valid | sum q (3) | sum p (3) | sum p_r q_c (9, row-major) | sum |q|^2 | sum d2 (inliers) | sum min(d2, clamp2)
// (valid rows) | rows skipped for a non-finite value
constexpr int ALIGN_PARTIAL = 21;
constexpr int AP_NIN = 0, AP_NVALID = 1, AP_SQ = 2, AP_SP = 5, AP_SPQ = 8, AP_SQQ = 17, AP_SD2 = 18, AP_SCLAMP = 19, AP_BAD = 20;

__device__ __forceinline__ int align_count(const int* __restrict__ count, int b, int N) { return count != nullptr ? min(max(count[b], 0), N) : N; }
__device__ __forceinline__ bool align_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }    // false for NaN and +-inf

__global__ __launch_bounds__(ALIGN_THREADS) void align_moments_kernel(const float* __restrict__ q, const float* __restrict__ p,
                                                                      const int* __restrict__ q_count, const int* __restrict__ p_count,
                                                                      const int* __restrict__ idx, const float* __restrict__ d2, int Nq, int Np,
                                                                      double clamp2, const double* __restrict__ state,
                                                                      const int* __restrict__ status, double* __restrict__ partial) {
    const int b = blockIdx.y;
    if (status[b] & FORGE_ALIGN_CONVERGED) return;                     // frozen: workgroup-uniform, before any barrier
    const int nq = align_count(q_count, b, Nq), np = align_count(p_count, b, Np);
    const int rows = idx != nullptr ? nq : min(nq, np);
    const double cut2 = state[(long long)b * FORGE_ALIGN_STATE_DOUBLES + FORGE_ALIGN_CUT2];
    const float* qb = q + 3ll * b * Nq;
    const float* pb = p + 3ll * b * Np;
    const int* ib = idx != nullptr ? idx + (long long)b * Nq : nullptr;
    const float* db = d2 != nullptr ? d2 + (long long)b * Nq : nullptr;
    double acc[ALIGN_PARTIAL];
#pragma unroll
    for (int e = 0; e < ALIGN_PARTIAL; ++e) acc[e] = 0.0;
    for (int i = blockIdx.x * ALIGN_THREADS + (int)threadIdx.x; i < rows; i += ALIGN_BLOCKS * ALIGN_THREADS) {
        const int j = ib != nullptr ? ib[i] : i;
        if ((unsigned)j >= (unsigned)np) continue;                     // no match: skipped, never followed
        const double qx = (double)qb[3ll * i], qy = (double)qb[3ll * i + 1], qz = (double)qb[3ll * i + 2];
        const double px = (double)pb[3ll * j], py = (double)pb[3ll * j + 1], pz = (double)pb[3ll * j + 2];
        const double d = db != nullptr ? (double)db[i] : 0.0;
        if (!(align_finite(qx) && align_finite(qy) && align_finite(qz) && align_finite(px) && align_finite(py) && align_finite(pz)) || d != d) {
            acc[AP_BAD] += 1.0;
            continue;
        }
        acc[AP_NVALID] += 1.0;
        acc[AP_SCLAMP] += fmin(d, clamp2);
        if (d > cut2) continue;                                        // an inlier is a valid row with !(d2 > cut2)
        acc[AP_NIN] += 1.0;
        acc[AP_SQ] += qx;
        acc[AP_SQ + 1] += qy;
        acc[AP_SQ + 2] += qz;
        acc[AP_SP] += px;
        acc[AP_SP + 1] += py;
        acc[AP_SP + 2] += pz;
        acc[AP_SPQ] = fma(px, qx, acc[AP_SPQ]);
        acc[AP_SPQ + 1] = fma(px, qy, acc[AP_SPQ + 1]);
        acc[AP_SPQ + 2] = fma(px, qz, acc[AP_SPQ + 2]);
        acc[AP_SPQ + 3] = fma(py, qx, acc[AP_SPQ + 3]);
        acc[AP_SPQ + 4] = fma(py, qy, acc[AP_SPQ + 4]);
        acc[AP_SPQ + 5] = fma(py, qz, acc[AP_SPQ + 5]);
        acc[AP_SPQ + 6] = fma(pz, qx, acc[AP_SPQ + 6]);
        acc[AP_SPQ + 7] = fma(pz, qy, acc[AP_SPQ + 7]);
        acc[AP_SPQ + 8] = fma(pz, qz, acc[AP_SPQ + 8]);
        acc[AP_SQQ] += fma(qz, qz, fma(qy, qy, qx * qx));
        acc[AP_SD2] += d;
    }
    __shared__ double red[ALIGN_THREADS];
    double* out = partial + ((long long)b * ALIGN_BLOCKS + blockIdx.x) * ALIGN_PARTIAL;
#pragma unroll
    for (int e = 0; e < ALIGN_PARTIAL; ++e) {
        __syncthreads();                                               // `red` is reused back to back
        const double r = block_sum256(acc[e], red);
        if (threadIdx.x == 0) out[e] = r;
    }
}

struct AlignOptions {
    double reject, reject_floor, tol, rank_tol;
    int with_scale, update;
};

// one workgroup of 64 threads per pair: thread e < ALIGN_PARTIAL adds sum e over the workgroups of the first launch in workgroup order, thread 0 solves
__global__ __launch_bounds__(64) void align_solve_kernel(const double* __restrict__ partial, AlignOptions o, double* __restrict__ state,
                                                         float* __restrict__ xf, int* __restrict__ status) {
    // No contraction in the solve (the explicit fma calls of so3.h keep theirs): with it, DELTA = |s R_rc - T_old| becomes fma(s, R_rc, -T_old) on the
    // UNROUNDED product and never reaches 0 at a fixed point where the stored T is the same bit for bit.
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    double* st = state + (long long)b * FORGE_ALIGN_STATE_DOUBLES;
    float* x = xf + 12ll * b;
    const int bits_in = status[b];
    __shared__ double m[ALIGN_PARTIAL];
    if (!(bits_in & FORGE_ALIGN_CONVERGED) && (int)threadIdx.x < ALIGN_PARTIAL) {
        const double* pp = partial + (long long)b * ALIGN_BLOCKS * ALIGN_PARTIAL + threadIdx.x;
        double s = 0.0;
        for (int k = 0; k < ALIGN_BLOCKS; ++k) s += pp[k * ALIGN_PARTIAL];
        m[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (bits_in & FORGE_ALIGN_CONVERGED) {                            // frozen: the state stands, xf is T rounded - as it was
        for (int e = 0; e < 12; ++e) x[e] = (float)st[FORGE_ALIGN_T + e];
        return;
    }
    const double n = m[AP_NIN], nv = m[AP_NVALID];
    int bits = (n < 3.0 ? FORGE_ALIGN_EMPTY : 0) | (m[AP_BAD] > 0.0 ? FORGE_ALIGN_NONFINITE : 0);
    const double mean_d2 = m[AP_SD2] / n;                              // 0 / 0 = NaN without inliers
    st[FORGE_ALIGN_RMSE] = sqrt(mean_d2);
    st[FORGE_ALIGN_N_IN] = n;
    st[FORGE_ALIGN_N_VALID] = nv;
    st[FORGE_ALIGN_SCORE] = m[AP_SCLAMP] / nv;
    double qm[3], pm[3];
    for (int r = 0; r < 3; ++r) {
        qm[r] = m[AP_SQ + r] / n;
        pm[r] = m[AP_SP + r] / n;
        st[FORGE_ALIGN_CQ + r] = qm[r];
        st[FORGE_ALIGN_CP + r] = pm[r];
    }
    if (!o.update) {                                                   // statistics only: T and what belongs to it stand
        status[b] = (bits_in & (FORGE_ALIGN_RANK | FORGE_ALIGN_CONVERGED)) | bits;
        for (int e = 0; e < 12; ++e) x[e] = (float)st[FORGE_ALIGN_T + e];
        return;
    }
    st[FORGE_ALIGN_ITERATIONS] += 1.0;
    if (bits & FORGE_ALIGN_EMPTY) {                                    // fewer than 3 inliers: T is kept, and the pair never counts as converged
        st[FORGE_ALIGN_DELTA] = 0.0;
        status[b] = bits;
        for (int e = 0; e < 12; ++e) x[e] = (float)st[FORGE_ALIGN_T + e];
        return;
    }
    double H[3][3], R[3][3], sv[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[r][c] = m[AP_SPQ + 3 * r + c] - m[AP_SP + r] * m[AP_SQ + c] / n;
    const double vq = m[AP_SQQ] - (m[AP_SQ] * m[AP_SQ] + m[AP_SQ + 1] * m[AP_SQ + 1] + m[AP_SQ + 2] * m[AP_SQ + 2]) / n;
    ps_project_so3(H, R, sv);
    if (!(sv[0] > 0.0) || !(sv[1] / sv[0] >= o.rank_tol)) bits |= FORGE_ALIGN_RANK;
    double s = 1.0;
    if (o.with_scale && vq > 0.0) {
        double tr = 0.0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) tr += R[r][c] * H[r][c];
        s = tr / vq;
    }
    double T[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = s * R[r][c];
        T[4 * r + 3] = pm[r] - (T[4 * r] * qm[0] + T[4 * r + 1] * qm[1] + T[4 * r + 2] * qm[2]);
    }
    double delta = 0.0;
    bool nan = false;
    for (int e = 0; e < 12; ++e) {
        const double d = fabs(T[e] - st[FORGE_ALIGN_T + e]);
        nan |= d != d;
        delta = fmax(delta, d);
        st[FORGE_ALIGN_T + e] = T[e];
        x[e] = (float)T[e];
    }
    if (nan) delta = (double)NAN;                                      // fmax drops a NaN operand: say so instead
    st[FORGE_ALIGN_SCALE] = s;
    st[FORGE_ALIGN_SV] = sv[0];
    st[FORGE_ALIGN_SV + 1] = sv[1];
    st[FORGE_ALIGN_SV + 2] = sv[2];
    st[FORGE_ALIGN_DELTA] = delta;
    st[FORGE_ALIGN_CUT2] = o.reject > 0.0 ? fmax(o.reject * o.reject * mean_d2, o.reject_floor * o.reject_floor) : (double)INFINITY;
    if (delta <= o.tol) bits |= FORGE_ALIGN_CONVERGED;
    status[b] = bits;
}

// one thread per pair: the start of lowest score, strict `<` in increasing k; a NaN score and a start with EMPTY set never win
__global__ void align_select_kernel(const double* __restrict__ state, const int* __restrict__ status, int B, int K, double* __restrict__ T,
                                    float* __restrict__ xf, int* __restrict__ best, double* __restrict__ state_out, int* __restrict__ status_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int win = -1;
    double score = (double)INFINITY;
    for (int k = 0; k < K; ++k) {
        const long long row = (long long)b * K + k;
        const double s = state[row * FORGE_ALIGN_STATE_DOUBLES + FORGE_ALIGN_SCORE];
        if (!(status[row] & FORGE_ALIGN_EMPTY) && s < score) {        // false for NaN; +inf never wins either
            win = k;
            score = s;
        }
    }
    const long long row = (long long)b * K + max(win, 0);              // none won: start 0 is what is reported, best = -1
    const double* st = state + row * FORGE_ALIGN_STATE_DOUBLES;
    for (int e = 0; e < FORGE_ALIGN_STATE_DOUBLES; ++e) state_out[(long long)b * FORGE_ALIGN_STATE_DOUBLES + e] = st[e];
    for (int e = 0; e < 12; ++e) {
        T[16ll * b + e] = st[FORGE_ALIGN_T + e];
        xf[12ll * b + e] = (float)st[FORGE_ALIGN_T + e];
    }
    T[16ll * b + 12] = 0.0;
    T[16ll * b + 13] = 0.0;
    T[16ll * b + 14] = 0.0;
    T[16ll * b + 15] = 1.0;
    best[b] = win;
    status_out[b] = status[row];
}

}  // namespace forge

extern "C" int forge_align_blocks(void) { return forge::ALIGN_BLOCKS; }

extern "C" long long forge_align_partial_doubles(int B) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && B <= 65535, FORGE_EINVAL, "forge_align_partial_doubles: B=%d outside 1 .. 65535", B);
    return (long long)B * ALIGN_BLOCKS * ALIGN_PARTIAL;
}

extern "C" int forge_align_step(const float* q, const float* p, const int* q_count, const int* p_count, const int* idx, const float* d2, int B, int Nq,
                                int Np, int with_scale, int update, double reject, double reject_floor, double tol, double rank_tol, double clamp2,
                                double* partial, double* state, float* xf, int* status, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && Nq >= 1 && Np >= 1, FORGE_EINVAL, "forge_align_step: B=%d Nq=%d Np=%d must be at least 1", B, Nq, Np);
    FORGE_REQUIRE(q && p && partial && state && xf && status, FORGE_EINVAL, "forge_align_step: null pointer (only the counts, idx and d2 may be null)");
    FORGE_REQUIRE((with_scale == 0 || with_scale == 1) && (update == 0 || update == 1), FORGE_EINVAL,
                  "forge_align_step: with_scale=%d and update=%d must be 0 or 1", with_scale, update);
    FORGE_REQUIRE(std::isfinite(reject) && reject >= 0.0 && std::isfinite(reject_floor) && reject_floor >= 0.0, FORGE_EINVAL,
                  "forge_align_step: reject=%g and reject_floor=%g must be finite and not negative", reject, reject_floor);
    FORGE_REQUIRE(std::isfinite(tol) && tol >= 0.0, FORGE_EINVAL, "forge_align_step: tol=%g must be finite and not negative", tol);
    FORGE_REQUIRE(rank_tol >= 0.0 && rank_tol < 1.0, FORGE_EINVAL, "forge_align_step: rank_tol=%g outside [0, 1)", rank_tol);
    FORGE_REQUIRE(clamp2 >= 0.0, FORGE_EINVAL, "forge_align_step: clamp2=%g must not be negative (it may be +inf)", clamp2);
    FORGE_REQUIRE(((unsigned long long)partial & 7ull) == 0 && ((unsigned long long)state & 7ull) == 0, FORGE_EINVAL,
                  "forge_align_step: partial and state must be 8-byte aligned");
    FORGE_REQUIRE(B <= 65535, FORGE_ESHAPE, "forge_align_step: B=%d pairs in one call (at most 65535)", B);
    FORGE_REQUIRE(Nq <= 0x7fffffff - ALIGN_BLOCKS * ALIGN_THREADS && Np <= 0x7fffffff - ALIGN_BLOCKS * ALIGN_THREADS, FORGE_ESHAPE,
                  "forge_align_step: Nq=%d or Np=%d beyond 32-bit rows", Nq, Np);
    hipLaunchKernelGGL(align_moments_kernel, dim3(ALIGN_BLOCKS, (unsigned)B), dim3(ALIGN_THREADS), 0, (hipStream_t)stream, q, p, q_count, p_count, idx, d2,
                       Nq, Np, clamp2, (const double*)state, (const int*)status, partial);
    FORGE_LAUNCH_CHECK("forge_align_step");
    AlignOptions o;
    o.reject = reject; o.reject_floor = reject_floor; o.tol = tol; o.rank_tol = rank_tol;
    o.with_scale = with_scale; o.update = update;
    hipLaunchKernelGGL(align_solve_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (const double*)partial, o, state, xf, status);
    FORGE_LAUNCH_CHECK("forge_align_step");
    return 0;
}

extern "C" int forge_align_select(const double* state, const int* status, int B, int K, double* T, float* xf, int* best, double* state_out,
                                  int* status_out, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && K >= 1, FORGE_EINVAL, "forge_align_select: B=%d K=%d must be at least 1", B, K);
    FORGE_REQUIRE(state && status && T && xf && best && state_out && status_out, FORGE_EINVAL, "forge_align_select: null pointer");
    FORGE_REQUIRE(((unsigned long long)state & 7ull) == 0 && ((unsigned long long)T & 7ull) == 0 && ((unsigned long long)state_out & 7ull) == 0,
                  FORGE_EINVAL, "forge_align_select: state, T and state_out must be 8-byte aligned");
    FORGE_REQUIRE(B <= 65535 && (long long)B * K <= 0x7fffffffll / FORGE_ALIGN_STATE_DOUBLES, FORGE_ESHAPE,
                  "forge_align_select: B=%d pairs (at most 65535) of K=%d starts", B, K);
    hipLaunchKernelGGL(align_select_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, state, status, B, K, T, xf, best, state_out,
                       status_out);
    FORGE_LAUNCH_CHECK("forge_align_select");
    return 0;
}
