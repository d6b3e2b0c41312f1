// token.hip — the token-row layers around the attention kernels of both pose estimators, fp32 on the matrix cores:
//   forge_token_linear_fwd   y[R,N] = act( LN?(x[R,K]) W[N,K]^T + bias ) (+ residual)      LayerNorm prologue, bias / exact-erf GELU / residual epilogue
//   forge_layer_norm_fwd     the same LayerNorm stand-alone (same device code, same bits)
//   forge_token_linear_bwd   dx, dW, dbias, dgamma, dbeta for an upstream dy               no atomics: fixed row chunks, det_reduce in chunk order
//   forge_layer_norm_bwd     the stand-alone counterpart
// The shapes are small (1024 x 256 token rows in the 2-D estimator, 16384 x 64 in the 3-D one), so the tiles are chosen for the number of
// workgroups, not for a large GEMM:
//   forward / dx:  workgroup = 2 waves = 32 rows x 64 output columns, one v_mfma_f32_32x32x2_f32 accumulator per wave (its issue interval equals its
//                  dependent latency: one chain keeps the pipe full). The 32-row tile of the contracted operand is staged ONCE per 256-wide chunk in
//                  LDS (32 x 260 floats = 33 KB: four workgroups per CU), normalised there (two passes over the resident row: mean, then the
//                  centred squares), and the weights stream from global memory / L2 (at most 1 MB, read by every workgroup).
//   dW:            workgroup = 4 waves = 64 x 64 of dW, contraction over one chunk of rows with both operands read straight from global memory
//                  (lanes along the channels: coalesced), the GELU derivative and the normalised rows recomputed on the way; dbias is the
//                  column sum of the A operand the k-tile-0 waves hold anyway.
//   LayerNorm bwd: 8 lanes per row, 32 rows per pass; the row means by a fixed exchange, dgamma / dbeta per chunk through LDS in row order.
// An MFMA result is a k-ordered fmaf chain; every kernel contracts in increasing k with the same pairing, so LN-prologue + linear equals
// forge_layer_norm_fwd followed by the plain linear bit for bit, and a strided y equals a dense one.
#include <cmath>
#include <cstdint>

#include "common.h"

namespace forge {

#pragma clang fp contract(off)      // every fused multiply-add below is spelled fmaf: the arithmetic does not depend on the instantiation

typedef float tk16v __attribute__((ext_vector_type(16)));

constexpr int TK_ROWS = 32;                 // rows of a forward / dx tile
constexpr int TK_KC = 256;                  // contraction chunk resident in LDS (the widest LayerNorm)
constexpr int TK_LD = TK_KC + 4;            // padded LDS row (floats; a multiple of 4: float4 access)
constexpr int TK_THREADS = 128;             // forward / dx / LayerNorm forward: 2 waves
constexpr int TK_MIN_CHUNK_ROWS = 128;      // dW / dbias row chunk: at least this many rows
constexpr int TK_WANT_WORKGROUPS = 512;     // ... and about this many dW workgroups (2 per CU)
constexpr int TK_LN_CHUNKS = 256;           // LayerNorm backward: at most about this many row chunks (one workgroup each)

constexpr float RSQRT2 = 0.70710678118654752440f;
constexpr float RSQRT2PI = 0.39894228040143267794f;

__device__ __forceinline__ float gelu_f(float v) { return (0.5f * v) * (1.f + erff(v * RSQRT2)); }
// GELU'(v) = Phi(v) + v phi(v)
__device__ __forceinline__ float gelu_grad_f(float v) {
    const float cdf = 0.5f * (1.f + erff(v * RSQRT2));
    const float pdf = expf(-0.5f * v * v) * RSQRT2PI;
    return fmaf(v, pdf, cdf);
}

// 32 rows x kw channels (kw <= 256, a multiple of 64) of a row-major matrix into the LDS tile, rows >= R as zeros. MUL: times GELU'(pre) (pre dense, ld N)
template <bool MUL>
__device__ __forceinline__ void tk_stage(float* xs, const float* __restrict__ x, long long ldx, long long row0, int R, int kc, int kw,
                                         const float* __restrict__ pre, int ldp) {
    const int kw4 = kw >> 2;
    for (int i = threadIdx.x; i < TK_ROWS * kw4; i += TK_THREADS) {
        const int r = i / kw4, c = (i - r * kw4) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < R) {
            v = *reinterpret_cast<const float4*>(x + (row0 + r) * ldx + kc + c);
            if constexpr (MUL) {
                const float4 p = *reinterpret_cast<const float4*>(pre + (row0 + r) * (long long)ldp + kc + c);
                v.x *= gelu_grad_f(p.x); v.y *= gelu_grad_f(p.y); v.z *= gelu_grad_f(p.z); v.w *= gelu_grad_f(p.w);
            }
        }
        *reinterpret_cast<float4*>(xs + r * TK_LD + c) = v;
    }
}

// LayerNorm of the 32 resident rows in place (torch's definition: mean and biased variance per row, y = (x - mean) rstd gamma + beta). 4 lanes per
// row, statistics in two passes over the resident row; (mean, rstd) to stats[row] when given. Called by all 128 threads between two barriers.
__device__ __forceinline__ void tk_layer_norm(float* xs, int K, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                              float* __restrict__ stats, long long row0, int R) {
    const int r = threadIdx.x >> 2, sub = threadIdx.x & 3;
    float* row = xs + r * TK_LD;
    float s = 0.f;
    for (int k = sub; k < K; k += 4) s += row[k];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    const float mean = s / (float)K;
    float v = 0.f;
    for (int k = sub; k < K; k += 4) { const float d = row[k] - mean; v = fmaf(d, d, v); }
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    const float rstd = 1.f / sqrtf(v / (float)K + eps);
    for (int k = sub; k < K; k += 4) row[k] = fmaf((row[k] - mean) * rstd, gamma[k], beta[k]);
    if (stats && sub == 0 && row0 + r < R) { stats[2 * (row0 + r)] = mean; stats[2 * (row0 + r) + 1] = rstd; }
}

struct TokFwd {
    const float *x, *w, *bias, *gamma, *beta, *res;
    float *y, *pre, *stats;
    long long ldx, ldr, ldy;
    float eps;
    int R, K, N, act;
};

// y tile = 32 rows x 64 columns; blockIdx.x = row tile * (N / 64) + column tile (the column tiles of a row tile are neighbours: they share x).
// A[i = row][k] from LDS, B[k][j = column] = w[column][k] from global memory; lane (n, h) takes k = 8 g + 4 h + 0..3 of every group of 8 on both.
__global__ __launch_bounds__(TK_THREADS) void token_linear_fwd_kernel(TokFwd a) {
    __shared__ __attribute__((aligned(16))) float xs[TK_ROWS * TK_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, n = lane & 31;
    const int nt = a.N >> 6;
    const int rt = blockIdx.x / nt, ct = blockIdx.x - rt * nt;
    const long long row0 = (long long)rt * TK_ROWS;
    const int col = (ct << 6) + (wave << 5) + n;                        // this lane's output column
    tk16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kc = 0; kc < a.K; kc += TK_KC) {
        const int kw = a.K - kc < TK_KC ? a.K - kc : TK_KC;
        if (kc) __syncthreads();
        tk_stage<false>(xs, a.x, a.ldx, row0, a.R, kc, kw, nullptr, 0);
        __syncthreads();
        if (a.gamma) {                                                  // (K <= 256: one chunk holds the whole row)
            tk_layer_norm(xs, a.K, a.gamma, a.beta, a.eps, ct == 0 ? a.stats : nullptr, row0, a.R);
            __syncthreads();
        }
        const float* wp = a.w + (long long)col * a.K + kc + 4 * h;
        const float* xp = xs + n * TK_LD + 4 * h;
        for (int g0 = 0; g0 < kw; g0 += 64) {                           // (kw is a multiple of 64: eight groups of 8 with their loads in flight)
#pragma unroll
            for (int g = g0; g < g0 + 64; g += 8) {
                const float4 av = *reinterpret_cast<const float4*>(xp + g);
                const float4 bv = *reinterpret_cast<const float4*>(wp + g);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            }
        }
    }
    // accumulator register r of lane (n, h) = row 8 (r / 4) + 4 h + r % 4, column n: a half-wave stores 128 contiguous bytes per row
    const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long row = row0 + 8 * (r >> 2) + 4 * h + (r & 3);
        if (row < a.R) {
            float v = acc[r] + b;
            if (a.pre) a.pre[row * a.N + col] = v;
            if (a.act) v = gelu_f(v);
            if (a.res) v = v + a.res[row * a.ldr + col];
            a.y[row * a.ldy + col] = v;
        }
    }
}

__global__ __launch_bounds__(TK_THREADS) void layer_norm_fwd_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, float* __restrict__ y, long long ldy,
                                                                    float* __restrict__ stats, int R, int K) {
    __shared__ __attribute__((aligned(16))) float xs[TK_ROWS * TK_LD];
    const long long row0 = (long long)blockIdx.x * TK_ROWS;
    tk_stage<false>(xs, x, ldx, row0, R, 0, K, nullptr, 0);
    __syncthreads();
    tk_layer_norm(xs, K, gamma, beta, eps, stats, row0, R);
    __syncthreads();
    const int k4 = K >> 2;
    for (int i = threadIdx.x; i < TK_ROWS * k4; i += TK_THREADS) {
        const int r = i / k4, c = (i - r * k4) << 2;
        if (row0 + r < R) *reinterpret_cast<float4*>(y + (row0 + r) * ldy + c) = *reinterpret_cast<const float4*>(xs + r * TK_LD + c);
    }
}

// dxn[R,K] = g W, g = dy o act'(pre): the forward's walk with the contraction over N. A[i = row][k = n] = g from LDS (the GELU derivative applied
// while staging), B[k = n][j = channel] = w[n][channel]: lanes along the channels, coalesced. out dense [R][K].
__global__ __launch_bounds__(TK_THREADS) void token_linear_dx_kernel(const float* __restrict__ dy, long long lddy, const float* __restrict__ pre,
                                                                     const float* __restrict__ w, float* __restrict__ out, int R, int K, int N) {
    __shared__ __attribute__((aligned(16))) float gs[TK_ROWS * TK_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, n = lane & 31;
    const int kt = K >> 6;
    const int rt = blockIdx.x / kt, ct = blockIdx.x - rt * kt;
    const long long row0 = (long long)rt * TK_ROWS;
    const int col = (ct << 6) + (wave << 5) + n;                        // this lane's channel of dxn
    tk16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int nc = 0; nc < N; nc += TK_KC) {
        const int nw = N - nc < TK_KC ? N - nc : TK_KC;
        if (nc) __syncthreads();
        if (pre) tk_stage<true>(gs, dy, lddy, row0, R, nc, nw, pre, N);
        else tk_stage<false>(gs, dy, lddy, row0, R, nc, nw, nullptr, 0);
        __syncthreads();
        const float* wp = w + (long long)(nc + 4 * h) * K + col;
        const float* gp = gs + n * TK_LD + 4 * h;
        for (int g0 = 0; g0 < nw; g0 += 64) {
#pragma unroll
            for (int g = g0; g < g0 + 64; g += 8) {
                const float4 av = *reinterpret_cast<const float4*>(gp + g);
                const float* q = wp + (long long)g * K;
                const float b0 = q[0], b1 = q[K], b2 = q[2 * (long long)K], b3 = q[3 * (long long)K];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b2, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b3, acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long row = row0 + 8 * (r >> 2) + 4 * h + (r & 3);
        if (row < R) out[row * K + col] = acc[r];
    }
}

// dW[n][k] = sum over the chunk's rows of g[row][n] xn[row][k], and dbias[n] = sum g[row][n]. blockIdx.x = (chunk, n tile, k tile) with the k tile
// fastest; wave w of the 64 x 64 tile: n half w & 1, k half w >> 1. A[i = n][kk = row] = g, B[kk = row][j = k] = xn, lane half h takes rows
// 8 s + 4 h + 0..3 of every group of 8 rows; rows past the chunk contribute zeros. xn is recomputed from x and (mean, rstd): never stored.
// Output to slab `chunk` of dw_out (slab stride N K; one chunk: dW itself) and of db_out (slab stride N).
__global__ __launch_bounds__(256) void token_linear_dw_kernel(const float* __restrict__ dy, long long lddy, const float* __restrict__ pre,
                                                              const float* __restrict__ x, long long ldx, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ stats,
                                                              float* __restrict__ dw_out, float* __restrict__ db_out, int R, int K, int N,
                                                              int chunk_rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, n = lane & 31;
    const int kt = K >> 6, nt = N >> 6;
    const int c = blockIdx.x / (kt * nt), t = blockIdx.x - c * (kt * nt);
    const int tn = t / kt, tk = t - tn * kt;
    const int ncol = (tn << 6) + ((wave & 1) << 5) + n;                 // A operand: this lane's output channel (row of dW)
    const int kcol = (tk << 6) + ((wave >> 1) << 5) + n;                // B operand: this lane's input channel (column of dW)
    const long long rbeg = (long long)c * chunk_rows;
    const long long rend = rbeg + chunk_rows < R ? rbeg + chunk_rows : R;
    const float gm = gamma ? gamma[kcol] : 1.f, bt = gamma ? beta[kcol] : 0.f;
    tk16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bsum = 0.f;
    for (long long r0 = rbeg; r0 < rend; r0 += 8) {
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long row = r0 + 4 * h + j;
            av[j] = 0.f;
            bv[j] = 0.f;
            if (row < rend) {
                float g = dy[row * lddy + ncol];
                if (pre) g *= gelu_grad_f(pre[row * N + ncol]);
                float xv = x[row * ldx + kcol];
                if (gamma) xv = fmaf((xv - stats[2 * row]) * stats[2 * row + 1], gm, bt);      // as tk_layer_norm wrote it
                av[j] = g;
                bv[j] = xv;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
            bsum += av[j];
        }
    }
    // accumulator register r of lane (n, h) = dW row (output channel) 8 (r / 4) + 4 h + r % 4 of the wave's 32, column (input channel) n
    float* dst = dw_out + (long long)c * N * K + (long long)((tn << 6) + ((wave & 1) << 5)) * K + kcol;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[(long long)(8 * (r >> 2) + 4 * h + (r & 3)) * K] = acc[r];
    if (db_out && tk == 0 && (wave >> 1) == 0) {
        bsum += __shfl_xor(bsum, 32);
        if (h == 0) db_out[(long long)c * N + ncol] = bsum;
    }
}

// LayerNorm backward of one chunk of rows: with xh = (x - mean) rstd and t = d gamma (d = the gradient of the normalised rows, dense ld K or by its
// stride), dx = rstd (t - mean_k t - xh mean_k(t xh)); dgamma = sum_rows d xh and dbeta = sum_rows d of the chunk to slab[chunk][2][K].
// 8 lanes per row (lane sub owns the float4s sub, sub + 8, ...), 32 rows per pass; the column sums per lane over the passes, then over the 32 row
// slots through LDS in slot order.
__global__ __launch_bounds__(256) void layer_norm_bwd_kernel(const float* __restrict__ d, long long ldd, const float* __restrict__ x, long long ldx,
                                                             const float* __restrict__ gamma, const float* __restrict__ stats, float* __restrict__ dx,
                                                             float* __restrict__ slab, int R, int K, int chunk_rows) {
    __shared__ float red[32][TK_KC + 1];
    const int slot = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int nf = K >> 5;                                              // float4s per lane: 2 .. 8
    const long long rbeg = (long long)blockIdx.x * chunk_rows;
    const long long rend = rbeg + chunk_rows < R ? rbeg + chunk_rows : R;
    float4 ag[8], ab[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { ag[i] = make_float4(0.f, 0.f, 0.f, 0.f); ab[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
    const float invK = 1.f / (float)K;
    for (long long r0 = rbeg; r0 < rend; r0 += 32) {
        const long long row = r0 + slot;
        const bool ok = row < rend;
        const float mean = ok ? stats[2 * row] : 0.f, rstd = ok ? stats[2 * row + 1] : 0.f;
        float4 t[8], xh[8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < nf) {
                const int k = (sub + 8 * i) << 2;
                float4 dv = make_float4(0.f, 0.f, 0.f, 0.f), xv = dv;
                if (ok) {
                    dv = *reinterpret_cast<const float4*>(d + row * ldd + k);
                    xv = *reinterpret_cast<const float4*>(x + row * ldx + k);
                }
                const float4 gv = *reinterpret_cast<const float4*>(gamma + k);
                xh[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
                t[i] = make_float4(dv.x * gv.x, dv.y * gv.y, dv.z * gv.z, dv.w * gv.w);
                s1 += (t[i].x + t[i].y) + (t[i].z + t[i].w);
                s2 = fmaf(t[i].x, xh[i].x, s2); s2 = fmaf(t[i].y, xh[i].y, s2); s2 = fmaf(t[i].z, xh[i].z, s2); s2 = fmaf(t[i].w, xh[i].w, s2);
                ag[i].x = fmaf(dv.x, xh[i].x, ag[i].x); ag[i].y = fmaf(dv.y, xh[i].y, ag[i].y);
                ag[i].z = fmaf(dv.z, xh[i].z, ag[i].z); ag[i].w = fmaf(dv.w, xh[i].w, ag[i].w);
                ab[i].x += dv.x; ab[i].y += dv.y; ab[i].z += dv.z; ab[i].w += dv.w;
            }
        }
        s1 += __shfl_xor(s1, 4); s1 += __shfl_xor(s1, 2); s1 += __shfl_xor(s1, 1);
        s2 += __shfl_xor(s2, 4); s2 += __shfl_xor(s2, 2); s2 += __shfl_xor(s2, 1);
        const float m1 = s1 * invK, m2 = s2 * invK;
        if (dx && ok) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < nf) {
                    const int k = (sub + 8 * i) << 2;
                    float4 o;
                    o.x = rstd * ((t[i].x - m1) - xh[i].x * m2); o.y = rstd * ((t[i].y - m1) - xh[i].y * m2);
                    o.z = rstd * ((t[i].z - m1) - xh[i].z * m2); o.w = rstd * ((t[i].w - m1) - xh[i].w * m2);
                    *reinterpret_cast<float4*>(dx + row * (long long)K + k) = o;
                }
            }
        }
    }
    if (!slab) return;
    float* out = slab + (long long)blockIdx.x * 2 * K;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < nf) {
                const int k = (sub + 8 * i) << 2;
                const float4 v = pass ? ab[i] : ag[i];
                red[slot][k] = v.x; red[slot][k + 1] = v.y; red[slot][k + 2] = v.z; red[slot][k + 3] = v.w;
            }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += 256) {
            float s = 0.f;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) s += red[r][k];
            out[pass * K + k] = s;
        }
    }
}

// ---- plans: functions of the shape arguments alone ----------------------------------------------------------------------------------------------
// dW / dbias: about TK_WANT_WORKGROUPS workgroups of 64 x 64 tiles, chunks of at least TK_MIN_CHUNK_ROWS rows (a multiple of 32), the slab set
// within DET_SLAB_BYTES. R = 16384, K = N = 64 -> 128 chunks of 128 rows; R = 1024, K = 256, N = 1024 -> 8 chunks of 128.
static void token_rows_plan(int R, int K, int N, int* chunks, int* chunk_rows) {
    const long long tiles = (long long)(K / 64) * (N / 64);
    long long want = (TK_WANT_WORKGROUPS + tiles - 1) / tiles;
    const long long cap = DET_SLAB_BYTES / ((long long)K * N * 4);
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    long long cr = ((R + want - 1) / want + 31) / 32 * 32;
    if (cr < TK_MIN_CHUNK_ROWS) cr = TK_MIN_CHUNK_ROWS;
    *chunk_rows = (int)cr;
    *chunks = (int)((R + cr - 1) / cr);
}

static void layer_norm_rows_plan(int R, int* chunks, int* chunk_rows) {
    const long long cr = (((long long)R + TK_LN_CHUNKS - 1) / TK_LN_CHUNKS + 31) / 32 * 32;
    *chunk_rows = (int)cr;
    *chunks = (int)((R + cr - 1) / cr);
}

// workspace of forge_token_linear_bwd in floats: [dxn R K | LayerNorm slabs chunks 2 K] (ln) then [dW slabs chunks N K | dbias slabs chunks N] (chunks > 1)
struct TokWs {
    long long dxn, lnslab, dw, db, total;
    int chunks, chunk_rows, lchunks, lchunk_rows;
};

static TokWs token_ws(int R, int K, int N, int ln) {
    TokWs p{};
    token_rows_plan(R, K, N, &p.chunks, &p.chunk_rows);
    layer_norm_rows_plan(R, &p.lchunks, &p.lchunk_rows);
    long long o = 0;
    p.dxn = o; o += ln ? (long long)R * K : 0;
    p.lnslab = o; o += ln ? (long long)p.lchunks * 2 * K : 0;
    p.dw = o; o += p.chunks > 1 ? (long long)p.chunks * N * K : 0;
    p.db = o; o += p.chunks > 1 ? (long long)p.chunks * N : 0;
    p.total = o;
    return p;
}

static bool tk_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int token_dims_check(const char* fn, int R, int K, int N, bool ln) {
    FORGE_REQUIRE(R >= 1, FORGE_EINVAL, "%s: R=%d rows (at least one)", fn, R);
    FORGE_REQUIRE(K >= 64 && N >= 64 && K % 64 == 0 && N % 64 == 0 && K <= 1024 && N <= 1024, FORGE_ESHAPE,
                  "%s: K=%d N=%d (multiples of 64, at most 1024)", fn, K, N);
    FORGE_REQUIRE(!ln || K <= TK_KC, FORGE_ESHAPE, "%s: LayerNorm over K=%d channels (at most %d: the normalised tile is LDS-resident)", fn, K, TK_KC);
    return 0;
}

static int token_stride_check(const char* fn, const char* what, long long ld, int width) {
    FORGE_REQUIRE(ld >= width && ld % 4 == 0, FORGE_ESHAPE, "%s: %s row stride %lld floats (a multiple of 4, at least the row's %d)", fn, what, ld, width);
    return 0;
}

static int layer_norm_bwd_launch(const char* fn, const float* d, long long ldd, const float* x, long long ldx, const float* gamma, const float* stats,
                                 float* dx, float* dgamma, float* dbeta, float* slab, int R, int K, hipStream_t st) {
    int chunks, chunk_rows;
    layer_norm_rows_plan(R, &chunks, &chunk_rows);
    const bool sums = dgamma || dbeta;
    hipLaunchKernelGGL(layer_norm_bwd_kernel, dim3((unsigned)chunks), dim3(256), 0, st, d, ldd, x, ldx, gamma, stats, dx, sums ? slab : nullptr, R, K,
                       chunk_rows);
    FORGE_LAUNCH_CHECK(fn);
    if (dgamma)
        if (const int rc = det_reduce(slab, chunks, 2ll * K, 1, 2ll * K, K, dgamma, 0, st, fn)) return rc;
    if (dbeta)
        if (const int rc = det_reduce(slab + K, chunks, 2ll * K, 1, 2ll * K, K, dbeta, 0, st, fn)) return rc;
    return 0;
}

}  // namespace forge

using namespace forge;

extern "C" int forge_token_linear_fwd(const float* x, long long ldx, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                                      const float* residual, long long ldr, float* y, long long ldy, float* pre, float* stats, int R, int K, int N,
                                      int act, forge_stream_t stream) {
    const char* fn = "forge_token_linear_fwd";
    FORGE_REQUIRE(x && w && y, FORGE_EINVAL, "%s: null pointer argument (x, w, y)", fn);
    FORGE_REQUIRE(act == FORGE_TOKEN_ACT_NONE || act == FORGE_TOKEN_ACT_GELU, FORGE_EINVAL, "%s: act=%d (0 = none, 1 = GELU)", fn, act);
    FORGE_REQUIRE((gamma == nullptr) == (beta == nullptr), FORGE_EINVAL, "%s: the LayerNorm prologue needs gamma and beta (or neither)", fn);
    FORGE_REQUIRE(gamma || !stats, FORGE_EINVAL, "%s: stats without a LayerNorm prologue", fn);
    if (const int rc = token_dims_check(fn, R, K, N, gamma != nullptr)) return rc;
    FORGE_REQUIRE(!gamma || (std::isfinite(eps) && eps >= 0.f), FORGE_EINVAL, "%s: eps %g", fn, (double)eps);
    if (const int rc = token_stride_check(fn, "x", ldx, K)) return rc;
    if (const int rc = token_stride_check(fn, "y", ldy, N)) return rc;
    if (residual)
        if (const int rc = token_stride_check(fn, "residual", ldr, N)) return rc;
    FORGE_REQUIRE(tk_aligned(x) && tk_aligned(w) && tk_aligned(y) && tk_aligned(bias) && tk_aligned(gamma) && tk_aligned(beta) && tk_aligned(residual) &&
                      tk_aligned(pre) && tk_aligned(stats), FORGE_EINVAL, "%s: every pointer must be 16-byte aligned", fn);
    const long long wgs = ((long long)R + TK_ROWS - 1) / TK_ROWS * (N / 64);
    FORGE_REQUIRE(wgs < (1ll << 31), FORGE_ESHAPE, "%s: R=%d N=%d: too many tiles", fn, R, N);
    const TokFwd a{x, w, bias, gamma, beta, residual, y, pre, stats, ldx, ldr, ldy, eps, R, K, N, act};
    hipLaunchKernelGGL(token_linear_fwd_kernel, dim3((unsigned)wgs), dim3(TK_THREADS), 0, (hipStream_t)stream, a);
    FORGE_LAUNCH_CHECK(fn);
    return 0;
}

extern "C" int forge_layer_norm_fwd(const float* x, long long ldx, const float* gamma, const float* beta, float eps, float* y, long long ldy, float* stats,
                                    int R, int K, forge_stream_t stream) {
    const char* fn = "forge_layer_norm_fwd";
    FORGE_REQUIRE(x && gamma && beta && y, FORGE_EINVAL, "%s: null pointer argument (x, gamma, beta, y)", fn);
    if (const int rc = token_dims_check(fn, R, K, 64, true)) return rc;
    FORGE_REQUIRE(std::isfinite(eps) && eps >= 0.f, FORGE_EINVAL, "%s: eps %g", fn, (double)eps);
    if (const int rc = token_stride_check(fn, "x", ldx, K)) return rc;
    if (const int rc = token_stride_check(fn, "y", ldy, K)) return rc;
    FORGE_REQUIRE(tk_aligned(x) && tk_aligned(gamma) && tk_aligned(beta) && tk_aligned(y) && tk_aligned(stats), FORGE_EINVAL,
                  "%s: every pointer must be 16-byte aligned", fn);
    hipLaunchKernelGGL(layer_norm_fwd_kernel, dim3((unsigned)((R + TK_ROWS - 1) / TK_ROWS)), dim3(TK_THREADS), 0, (hipStream_t)stream, x, ldx, gamma, beta,
                       eps, y, ldy, stats, R, K);
    FORGE_LAUNCH_CHECK(fn);
    return 0;
}

extern "C" int forge_token_rows_plan(int R, int K, int N, int* chunks, int* chunk_rows) {
    const char* fn = "forge_token_rows_plan";
    FORGE_REQUIRE(chunks && chunk_rows, FORGE_EINVAL, "%s: null pointer argument", fn);
    if (const int rc = token_dims_check(fn, R, K, N, false)) return rc;
    token_rows_plan(R, K, N, chunks, chunk_rows);
    return 0;
}

extern "C" long long forge_token_linear_bwd_ws_bytes(int R, int K, int N, int ln) {
    if (token_dims_check("forge_token_linear_bwd_ws_bytes", R, K, N, ln != 0)) return -1;
    return token_ws(R, K, N, ln).total * 4;
}

extern "C" int forge_token_linear_bwd(const float* dy, long long lddy, const float* x, long long ldx, const float* w, const float* gamma, const float* beta,
                                      const float* stats, const float* pre, float* dx, float* dw, float* dbias, float* dgamma, float* dbeta, float* ws,
                                      long long ws_bytes, int R, int K, int N, int act, forge_stream_t stream) {
    const char* fn = "forge_token_linear_bwd";
    FORGE_REQUIRE(dy && x && w, FORGE_EINVAL, "%s: null pointer argument (dy, x, w)", fn);
    FORGE_REQUIRE(act == FORGE_TOKEN_ACT_NONE || act == FORGE_TOKEN_ACT_GELU, FORGE_EINVAL, "%s: act=%d (0 = none, 1 = GELU)", fn, act);
    FORGE_REQUIRE(act == FORGE_TOKEN_ACT_NONE || pre, FORGE_EINVAL, "%s: the GELU backward needs the saved pre-activation", fn);
    FORGE_REQUIRE((gamma == nullptr) == (beta == nullptr) && (gamma == nullptr) == (stats == nullptr), FORGE_EINVAL,
                  "%s: a LayerNorm prologue needs gamma, beta and the saved stats (or none of them)", fn);
    FORGE_REQUIRE(gamma || (!dgamma && !dbeta), FORGE_EINVAL, "%s: dgamma / dbeta without a LayerNorm prologue", fn);
    FORGE_REQUIRE(dw || !dbias, FORGE_EINVAL, "%s: dbias is a by-product of the dW pass: pass dw as well", fn);
    const bool ln = gamma != nullptr;
    if (const int rc = token_dims_check(fn, R, K, N, ln)) return rc;
    if (const int rc = token_stride_check(fn, "dy", lddy, N)) return rc;
    if (const int rc = token_stride_check(fn, "x", ldx, K)) return rc;
    FORGE_REQUIRE(tk_aligned(dy) && tk_aligned(x) && tk_aligned(w) && tk_aligned(gamma) && tk_aligned(beta) && tk_aligned(stats) && tk_aligned(pre) &&
                      tk_aligned(dx) && tk_aligned(dw) && tk_aligned(dbias) && tk_aligned(dgamma) && tk_aligned(dbeta) && tk_aligned(ws), FORGE_EINVAL,
                  "%s: every pointer must be 16-byte aligned", fn);
    const TokWs p = token_ws(R, K, N, ln);
    FORGE_REQUIRE(p.total == 0 || (ws && ws_bytes >= p.total * 4), FORGE_EINVAL, "%s: workspace of %lld bytes, forge_token_linear_bwd_ws_bytes asks for %lld", fn,
                  ws ? ws_bytes : 0ll, p.total * 4);
    const long long dx_wgs = ((long long)R + TK_ROWS - 1) / TK_ROWS * (K / 64);
    const long long dw_wgs = (long long)p.chunks * (K / 64) * (N / 64);
    FORGE_REQUIRE(dx_wgs < (1ll << 31) && dw_wgs < (1ll << 31), FORGE_ESHAPE, "%s: R=%d K=%d N=%d: too many tiles", fn, R, K, N);
    hipStream_t st = (hipStream_t)stream;
    const float* gpre = act == FORGE_TOKEN_ACT_GELU ? pre : nullptr;
    if (dx || dgamma || dbeta) {
        float* dxn = ln ? ws + p.dxn : dx;
        hipLaunchKernelGGL(token_linear_dx_kernel, dim3((unsigned)dx_wgs), dim3(TK_THREADS), 0, st, dy, lddy, gpre, w, dxn, R, K, N);
        FORGE_LAUNCH_CHECK(fn);
        if (ln)
            if (const int rc = layer_norm_bwd_launch(fn, dxn, K, x, ldx, gamma, stats, dx, dgamma, dbeta, ws + p.lnslab, R, K, st)) return rc;
    }
    if (dw) {
        const bool split = p.chunks > 1;
        hipLaunchKernelGGL(token_linear_dw_kernel, dim3((unsigned)dw_wgs), dim3(256), 0, st, dy, lddy, gpre, x, ldx, gamma, beta, stats,
                           split ? ws + p.dw : dw, dbias ? (split ? ws + p.db : dbias) : nullptr, R, K, N, p.chunk_rows);
        FORGE_LAUNCH_CHECK(fn);
        if (split) {
            if (const int rc = det_reduce(ws + p.dw, p.chunks, (long long)N * K, 1, (long long)N * K, (long long)N * K, dw, 0, st, fn)) return rc;
            if (dbias)
                if (const int rc = det_reduce(ws + p.db, p.chunks, N, 1, N, N, dbias, 0, st, fn)) return rc;
        }
    }
    return 0;
}

extern "C" long long forge_layer_norm_bwd_ws_bytes(int R, int K) {
    if (token_dims_check("forge_layer_norm_bwd_ws_bytes", R, K, 64, true)) return -1;
    int chunks, chunk_rows;
    layer_norm_rows_plan(R, &chunks, &chunk_rows);
    return (long long)chunks * 2 * K * 4;
}

extern "C" int forge_layer_norm_bwd(const float* dy, long long lddy, const float* x, long long ldx, const float* gamma, const float* stats, float* dx,
                                    float* dgamma, float* dbeta, float* ws, long long ws_bytes, int R, int K, forge_stream_t stream) {
    const char* fn = "forge_layer_norm_bwd";
    FORGE_REQUIRE(dy && x && gamma && stats, FORGE_EINVAL, "%s: null pointer argument (dy, x, gamma, stats)", fn);
    if (const int rc = token_dims_check(fn, R, K, 64, true)) return rc;
    if (const int rc = token_stride_check(fn, "dy", lddy, K)) return rc;
    if (const int rc = token_stride_check(fn, "x", ldx, K)) return rc;
    FORGE_REQUIRE(tk_aligned(dy) && tk_aligned(x) && tk_aligned(gamma) && tk_aligned(stats) && tk_aligned(dx) && tk_aligned(dgamma) && tk_aligned(dbeta) &&
                      tk_aligned(ws), FORGE_EINVAL, "%s: every pointer must be 16-byte aligned", fn);
    const long long need = forge_layer_norm_bwd_ws_bytes(R, K);
    FORGE_REQUIRE(!(dgamma || dbeta) || (ws && ws_bytes >= need), FORGE_EINVAL, "%s: workspace of %lld bytes, forge_layer_norm_bwd_ws_bytes asks for %lld", fn,
                  ws ? ws_bytes : 0ll, need);
    if (!dx && !dgamma && !dbeta) return 0;
    return layer_norm_bwd_launch(fn, dy, lddy, x, ldx, gamma, stats, dx, dgamma, dbeta, ws, R, K, (hipStream_t)stream);
}
