// attention.hip — single-head dot-product attention O = softmax(Q K^T) V in fp32 on the matrix cores, for the N = 4096-token attentions of the
// 3-D pose estimator in predicted-pose INFERENCE (models/model_utils.py:207-229 `Attention`, unscaled, one head of 64 channels; called by
// models/pose_estimator_3d.py:116-144: cross attention whose N x N matrix multiplies the positional table, then a self-attention block).
//
// Stock torch materialises the [B, N, N] matrix three times (rocBLAS QK^T, softmax, rocBLAS PV: 268 MB per pass at B = 4, N = 4096); here it
// never leaves registers (online softmax over key tiles, Milakov & Gimelshein / FlashAttention recurrence):
//   workgroup = 4 waves; KS = 2: 64 queries, wave w -> queries 32 (w & 1) .. +31 and key half (w >> 1); KS = 4 (few queries: B Nq / 64 workgroups
//   would leave SIMDs empty): 32 queries, wave w -> key quarter w. The key parts of a query are merged through LDS at the end.
//   per 32-key tile and wave: S^T = K Q^T   (32 v_mfma_f32_32x32x2_f32: lanes = queries, accumulator registers = keys)
//                             running max / sum per query = per lane (+ one exchange between the two half-waves), P = exp(S - max) in place
//                             (Q is pre-multiplied by log2 e, so exp is one v_exp_f32 per element: 2^(s' - max'))
//                             O^T += V^T P^T (32 MFMAs): the S^T accumulator registers ARE the B operand - the contraction runs over the keys in
//                             the order the accumulator holds them, and the A operand (V) is loaded in that order
// Q stays in registers for the whole loop; K / V tiles come straight from global memory (2 MB per batch element: L2-resident, every wave of a
// workgroup and 63 other workgroups read the same tiles), the next K tile is requested before the current tile's MFMAs.
// Bound: MFMA fp32. FLOPs = 4 B Nq Nk 64. The result differs from softmax-then-matmul only in the order of the fp32 additions.
// Training (opt-in on the Python side): the same kernel with the log-sum-exp of each query stored (forge_attention_fwd_lse) and a backward that
// recomputes the softmax from it (forge_attention_bwd), second half of this file.
#include "common.h"

namespace forge {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int ATT_D = 64;          // channels of q / k and of v (one head)
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float LN2 = 0.69314718055994530942f;

// LSE (training, forge_attention_fwd_lse): additionally lse[b][query] = ln sum_keys exp(q . k), from the merged M and den of the last stage.
template <int KS, bool LSE>
__global__ __launch_bounds__(256) void attention_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            long long v_batch_rows, float* __restrict__ out, float* __restrict__ lse, int Nq, int Nk) {
    constexpr int QW = 4 / KS;                             // query groups (of 32) per workgroup
    __shared__ float mrg[3][64][35];                       // key parts 1.. of a query group: (O^T column: 32 floats, max, sum) per lane, padded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, n = lane & 31;
    const int qtiles = Nq / (32 * QW);
    const int b = blockIdx.x / qtiles, qt = blockIdx.x - b * qtiles;
    const int qw = wave % QW, kh = wave / QW;
    const int q0 = (qt * QW + qw) << 5;
    const int kbeg = kh * (Nk / KS), kend = kbeg + Nk / KS;
    const float* Kb = k + (size_t)b * Nk * ATT_D;
    const float* Vb = v + (size_t)b * v_batch_rows * ATT_D;

    // B operand of S^T = K Q^T: lane (query n, half h) holds Q[q0 + n][32 h + s] for MFMA step s (the two channels one step contracts are
    // s and 32 + s: any pairing of the 64 channels is the same sum up to the order of the additions)
    float qr[32], kr[32], kn[32];
    {
        const float4* p = reinterpret_cast<const float4*>(q + ((size_t)b * Nq + q0 + n) * ATT_D + 32 * h);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float4 t = p[i]; qr[4 * i] = t.x * LOG2E; qr[4 * i + 1] = t.y * LOG2E; qr[4 * i + 2] = t.z * LOG2E; qr[4 * i + 3] = t.w * LOG2E; }
        const float4* pk = reinterpret_cast<const float4*>(Kb + (size_t)(kbeg + n) * ATT_D + 32 * h);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float4 t = pk[i]; kr[4 * i] = t.x; kr[4 * i + 1] = t.y; kr[4 * i + 2] = t.z; kr[4 * i + 3] = t.w; }
    }
    f16v o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m = -INFINITY, l = 0.f;

    for (int kt = kbeg; kt < kend; kt += 32) {
        // A operand of O^T += V^T P^T, in the key order of the S^T accumulator: register r of half h holds key 8 (r / 4) + 4 h + r % 4
        float v0[16], v1[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* pv = Vb + (size_t)(kt + 8 * (r >> 2) + 4 * h + (r & 3)) * ATT_D + n;
            v0[r] = pv[0];
            v1[r] = pv[32];
        }
        const int ktn = kt + 32 < kend ? kt + 32 : kbeg;            // (the last iteration re-reads the first tile: no branch around the loads)
        {
            const float4* pk = reinterpret_cast<const float4*>(Kb + (size_t)(ktn + n) * ATT_D + 32 * h);
#pragma unroll
            for (int i = 0; i < 8; ++i) { const float4 t = pk[i]; kn[4 * i] = t.x; kn[4 * i + 1] = t.y; kn[4 * i + 2] = t.z; kn[4 * i + 3] = t.w; }
        }
        f16v s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[i], qr[i], s, 0, 0, 0);
        float tmax = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mn = fmaxf(m, tmax);
        const float sc = __builtin_amdgcn_exp2f(m - mn);                             // first tile: 2^(-inf) = 0
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(s[r] - mn); ps += s[r]; }
        ps += __shfl_xor(ps, 32);
        l = l * sc + ps;
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= sc; o1[r] *= sc; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[r], s[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[r], s[r], o1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) kr[i] = kn[i];
    }

    // merge the key parts of each query: O = sum_p O_p 2^(m_p - M) / sum_p l_p 2^(m_p - M), M = max_p m_p
    if (kh > 0) {
        float* dst = mrg[(kh - 1) * QW + qw][lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) { dst[r] = o0[r]; dst[16 + r] = o1[r]; }
        dst[32] = m;
        dst[33] = l;
    }
    __syncthreads();
    if (kh == 0) {
        float M = m;
#pragma unroll
        for (int p = 1; p < KS; ++p) M = fmaxf(M, mrg[(p - 1) * QW + qw][lane][32]);
        const float a0 = __builtin_amdgcn_exp2f(m - M);
        float den;
        {
            // products rounded, then added in the order of the parts: spelled out (no contraction into fma), so that every instantiation of the
            // kernel - with and without the lse store - divides by the same bits
#pragma clang fp contract(off)
            den = l * a0;
#pragma unroll
            for (int p = 1; p < KS; ++p) {
                const float* src = mrg[(p - 1) * QW + qw][lane];
                den = den + src[33] * __builtin_amdgcn_exp2f(src[32] - M);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= a0; o1[r] *= a0; }
#pragma unroll
        for (int p = 1; p < KS; ++p) {
            const float* src = mrg[(p - 1) * QW + qw][lane];
            const float ap = __builtin_amdgcn_exp2f(src[32] - M);
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] += src[r] * ap; o1[r] += src[16 + r] * ap; }
        }
        const float inv = 1.f / den;
        if constexpr (LSE) {
            // M and den are in base 2 (Q was pre-multiplied by log2 e): ln sum exp = (M + log2 den) ln 2, rounded once at the size of the result;
            // both half-waves hold the same M and den, one of them stores
            if (h == 0) lse[(size_t)b * Nq + q0 + n] = fmaf(M, LN2, __log2f(den) * LN2);
        }
        // accumulator register r of half h = channel 8 (r / 4) + 4 h + r % 4 (o1: + 32) of query n: four consecutive channels per float4
        float* po = out + ((size_t)b * Nq + q0 + n) * ATT_D + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            *reinterpret_cast<float4*>(po + 8 * g) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4*>(po + 32 + 8 * g) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Backward (training, forge_attention_bwd). With P = exp(S - lse) recomputed per tile from the saved log-sum-exp, nothing of size N x N is stored:
//   delta[q] = sum_c dO[q][c] O[q][c]            dP = dO V^T            dS = P o (dP - delta)
//   dQ = dS K            dK = dS^T Q            dV = P^T dO
// No atomics: dQ is accumulated by the wave that owns the queries, dK / dV by the wave that owns the keys (two walks over the tiles, S and dP computed
// in both), and the parts of a split are summed through LDS in a fixed order - the result is bitwise reproducible.
// The logits are recomputed BIT FOR BIT as the forward computed them (Q pre-multiplied by log2 e, the same products accumulated in
// the same MFMA order: s' of magnitude ~90 carries an error of ~1e-5, which cancels in s' - lse' only against the lse' built from the same bits), and
// P = 2^fma(-lse, log2 e, s'): one rounding, of a small number - what is left is the rounding of the saved lse itself (|lse| up to ~60: 2e-6).
// The row residual. delta comes from the forward's fp32 `out`, so sum_keys dS[q][.] = dO . (O_exact - O) =: r[q] instead of 0 to rounding: the forward's
// own rounding, multiplied by the attention-weighted mean key in dQ. Where dQ is the small remainder of cancelling terms (a nearly uniform attention
// over nearly equal keys: the estimator's self attention) that was 4-10 x torch's fp32 error. The dQ pass therefore also accumulates r, Z = sum_keys P
// (row sums of registers it holds anyway) and Bk = P K (one more MFMA chain on the K operand it has loaded), and finishes with
//   rho = r / Z,   dQ -= rho Bk,   delta_ws += rho
// which is dS = P o (dP - delta - rho) with sum_keys dS = 0 exactly as torch's softmax backward has it; the dK / dV pass reads the corrected delta.
// 8 GEMM-sized contractions with dV (S, dP twice; dQ, Bk, dK, dV), 7 without.

// delta[row] = sum_c dout[row][c] out[row][c]: 16 lanes per row, a float4 each, fixed-order exchange. rows is a multiple of 64: every wave is full.
__global__ __launch_bounds__(256) void attention_delta_kernel(const float* __restrict__ out, const float* __restrict__ dout, float* __restrict__ delta,
                                                              long long rows) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = t >> 4;
    if (row >= rows) return;
    const float4 a = *reinterpret_cast<const float4*>(out + row * ATT_D + 4 * (t & 15));
    const float4 g = *reinterpret_cast<const float4*>(dout + row * ATT_D + 4 * (t & 15));
    float s = a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if ((t & 15) == 0) delta[row] = s;
}

// 32 rows x 64 channels of a row-major [.][64] matrix as the A / B operand of a channel contraction: lane (row n, half h) holds x[row0 + n][32 h + s]
// for MFMA step s, times `scale`
__device__ __forceinline__ void load_rows(float (&r)[32], const float* __restrict__ x, size_t row0, int n, int h, float scale = 1.f) {
    const float4* p = reinterpret_cast<const float4*>(x + (row0 + n) * ATT_D + 32 * h);
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float4 t = p[i]; r[4 * i] = t.x * scale; r[4 * i + 1] = t.y * scale; r[4 * i + 2] = t.z * scale; r[4 * i + 3] = t.w * scale; }
}

// the same 32 rows as the A operand of a contraction over the ROWS, in the order an accumulator holds them: register r of half h = row
// 8 (r / 4) + 4 h + r % 4, lane n = channel n (c0) and 32 + n (c1)
__device__ __forceinline__ void load_cols(float (&c0)[16], float (&c1)[16], const float* __restrict__ x, size_t row0, int n, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float* p = x + (row0 + 8 * (r >> 2) + 4 * h + (r & 3)) * ATT_D + n;
        c0[r] = p[0];
        c1[r] = p[32];
    }
}

// store a [channel][row] accumulator pair (lane = row n, register r of half h = channel 8 (r / 4) + 4 h + r % 4, a1: + 32) to row-major x
__device__ __forceinline__ void store_acc(float* __restrict__ x, size_t row0, int n, int h, const f16v& a0, const f16v& a1) {
    float* po = x + (row0 + n) * ATT_D + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(po + 8 * g) = make_float4(a0[4 * g], a0[4 * g + 1], a0[4 * g + 2], a0[4 * g + 3]);
        *reinterpret_cast<float4*>(po + 32 + 8 * g) = make_float4(a1[4 * g], a1[4 * g + 1], a1[4 * g + 2], a1[4 * g + 3]);
    }
}

// dQ pass: the forward's walk (a wave owns 32 queries = lanes, KS key parts per query merged through LDS) plus two GEMMs per tile:
//   S^T = K Q^T, dP^T = V dO^T (accumulator registers = keys), P^T and dS^T = P^T o (dP^T - delta) in place, dQ^T += K^T dS^T and Bk^T += K^T P^T with the
//   dS^T / P^T registers as B operand; row sums r and Z per lane; at the end the residual correction (above), delta updated in place for the next pass
// (launch bounds: 2 waves per SIMD. Left to itself the compiler takes 161 VGPRs + 96 AGPRs for KS = 4, one register over the budget of two waves.)
template <int KS>
__global__ __launch_bounds__(256, 2) void attention_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                               long long v_batch_rows, const float* __restrict__ lse, float* __restrict__ delta,
                                                               const float* __restrict__ dout, float* __restrict__ dq, int Nq, int Nk) {
    constexpr int QW = 4 / KS;
    __shared__ float mrg[3][64][67];                       // key parts 1.. of a query group: (dQ^T, Bk^T columns: 2 x 32 floats, r, Z) per lane, padded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, n = lane & 31;
    const int qtiles = Nq / (32 * QW);
    const int b = blockIdx.x / qtiles, qt = blockIdx.x - b * qtiles;
    const int qw = wave % QW, kh = wave / QW;
    const int q0 = (qt * QW + qw) << 5;
    const int kbeg = kh * (Nk / KS), kend = kbeg + Nk / KS;
    const float* Kb = k + (size_t)b * Nk * ATT_D;
    const float* Vb = v + (size_t)b * v_batch_rows * ATT_D;
    const size_t qrow0 = (size_t)b * Nq + q0;

    float qr[32], gr[32];
    load_rows(qr, q, qrow0, n, h, LOG2E);                  // as the forward: S^T in base 2
    load_rows(gr, dout, qrow0, n, h);
    const float ls = lse[qrow0 + n], dl = delta[qrow0 + n];
    f16v a0, a1, b0, b1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a0[r] = 0.f; a1[r] = 0.f; b0[r] = 0.f; b1[r] = 0.f; }
    float rs = 0.f, zs = 0.f;                              // this lane's keys (its half-wave's registers): the halves are added after the walk

    for (int kt = kbeg; kt < kend; kt += 32) {
        float kr[32], vr[32], k0[16], k1[16];
        load_rows(kr, Kb, kt, n, h);
        load_rows(vr, Vb, kt, n, h);
        load_cols(k0, k1, Kb, kt, n, h);
        f16v s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int i = 0; i < 32; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[i], qr[i], s, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 32; ++i) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[i], gr[i], dp, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(fmaf(-ls, LOG2E, s[r]));
            dp[r] = s[r] * (dp[r] - dl);
        }
        float tz = 0.f, tr = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { tz += s[r]; tr += dp[r]; }
        zs += tz;
        rs += tr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[r], dp[r], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[r], dp[r], a1, 0, 0, 0);
            b0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[r], s[r], b0, 0, 0, 0);
            b1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[r], s[r], b1, 0, 0, 0);
        }
    }
    rs += __shfl_xor(rs, 32);                              // both half-waves now hold the sums over the part's keys
    zs += __shfl_xor(zs, 32);

    // the key parts of a query are plain partial sums (lse is the whole row's): added in the order of the parts
    if (kh > 0) {
        float* dst = mrg[(kh - 1) * QW + qw][lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) { dst[r] = a0[r]; dst[16 + r] = a1[r]; dst[32 + r] = b0[r]; dst[48 + r] = b1[r]; }
        dst[64] = rs;
        dst[65] = zs;
    }
    __syncthreads();                                       // (every wave has read its delta before this point: the update below is safe)
    if (kh == 0) {
#pragma unroll
        for (int p = 1; p < KS; ++p) {
            const float* src = mrg[(p - 1) * QW + qw][lane];
#pragma unroll
            for (int r = 0; r < 16; ++r) { a0[r] += src[r]; a1[r] += src[16 + r]; b0[r] += src[32 + r]; b1[r] += src[48 + r]; }
            rs += src[64];
            zs += src[65];
        }
        const float rho = rs / zs;                         // Z = 1 up to the rounding of lse: never near 0
#pragma unroll
        for (int r = 0; r < 16; ++r) { a0[r] = fmaf(-rho, b0[r], a0[r]); a1[r] = fmaf(-rho, b1[r], a1[r]); }
        store_acc(dq, qrow0, n, h, a0, a1);
        if (h == 0) delta[qrow0 + n] = dl + rho;
    }
}

// dK / dV pass: the transposed walk. A wave owns 32 keys (= lanes; K and V rows resident as B operands) and walks the query tiles of its part (QS
// parts per key group, merged through LDS in the order of the parts):
//   S = Q K^T, dP = dO V^T (accumulator registers = queries: lse and delta are indexed by register), dS = P o (dP - delta) in place,
//   dV^T += dO^T P, dK^T += Q^T dS with the P / dS registers as B operand. DV = false (one value table for the whole batch, not trained): no dV chain.
template <int QS, bool DV>
__global__ __launch_bounds__(256) void attention_bwd_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                long long v_batch_rows, const float* __restrict__ lse, const float* __restrict__ delta,
                                                                const float* __restrict__ dout, float* __restrict__ dk, float* __restrict__ dv, int Nq,
                                                                int Nk) {
    constexpr int KW = 4 / QS;                             // key groups (of 32) per workgroup
    constexpr int MW = DV ? 65 : 33;                       // dK^T (and dV^T) column of a lane, padded
    __shared__ float mrg[3][64][MW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, n = lane & 31;
    const int ktiles = Nk / (32 * KW);
    const int b = blockIdx.x / ktiles, kt = blockIdx.x - b * ktiles;
    const int kw = wave % KW, qh = wave / KW;
    const int k0 = (kt * KW + kw) << 5;
    const int qbeg = qh * (Nq / QS), qend = qbeg + Nq / QS;
    const float* Qb = q + (size_t)b * Nq * ATT_D;
    const float* Gb = dout + (size_t)b * Nq * ATT_D;
    const float* Lb = lse + (size_t)b * Nq;
    const float* Db = delta + (size_t)b * Nq;

    float kr[32], vr[32];
    load_rows(kr, k, (size_t)b * Nk + k0, n, h);
    load_rows(vr, v, (size_t)b * v_batch_rows + k0, n, h);
    f16v dk0, dk1, dv0, dv1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }

    for (int qt = qbeg; qt < qend; qt += 32) {
        float qr[32], gr[32], q0[16], q1[16], g0[16], g1[16], ls[16], dl[16];
        load_rows(qr, Qb, qt, n, h, LOG2E);                // the forward's products (q log2 e) k, with A and B operand exchanged
        load_rows(gr, Gb, qt, n, h);
        load_cols(q0, q1, Qb, qt, n, h);
        if constexpr (DV) load_cols(g0, g1, Gb, qt, n, h);
#pragma unroll
        for (int g = 0; g < 4; ++g) {                      // register r = query 8 (r / 4) + 4 h + r % 4 of the tile
            const float4 a = *reinterpret_cast<const float4*>(Lb + qt + 8 * g + 4 * h);
            const float4 d = *reinterpret_cast<const float4*>(Db + qt + 8 * g + 4 * h);
            ls[4 * g] = a.x; ls[4 * g + 1] = a.y; ls[4 * g + 2] = a.z; ls[4 * g + 3] = a.w;
            dl[4 * g] = d.x; dl[4 * g + 1] = d.y; dl[4 * g + 2] = d.z; dl[4 * g + 3] = d.w;
        }
        f16v s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int i = 0; i < 32; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[i], kr[i], s, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 32; ++i) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[i], vr[i], dp, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(fmaf(-ls[r], LOG2E, s[r]));
            dp[r] = s[r] * (dp[r] - dl[r]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if constexpr (DV) {
                dv0 = __builtin_amdgcn_mfma_f32_32x32x2f32(g0[r], s[r], dv0, 0, 0, 0);
                dv1 = __builtin_amdgcn_mfma_f32_32x32x2f32(g1[r], s[r], dv1, 0, 0, 0);
            }
            dk0 = __builtin_amdgcn_mfma_f32_32x32x2f32(q0[r], dp[r], dk0, 0, 0, 0);
            dk1 = __builtin_amdgcn_mfma_f32_32x32x2f32(q1[r], dp[r], dk1, 0, 0, 0);
        }
    }

    if (qh > 0) {
        float* dst = mrg[(qh - 1) * KW + kw][lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) { dst[r] = dk0[r]; dst[16 + r] = dk1[r]; }
        if constexpr (DV) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { dst[32 + r] = dv0[r]; dst[48 + r] = dv1[r]; }
        }
    }
    __syncthreads();
    if (qh == 0) {
#pragma unroll
        for (int p = 1; p < QS; ++p) {
            const float* src = mrg[(p - 1) * KW + kw][lane];
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk0[r] += src[r]; dk1[r] += src[16 + r]; }
            if constexpr (DV) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { dv0[r] += src[32 + r]; dv1[r] += src[48 + r]; }
            }
        }
        store_acc(dk, (size_t)b * Nk + k0, n, h, dk0, dk1);
        if constexpr (DV) store_acc(dv, (size_t)b * Nk + k0, n, h, dv0, dv1);
    }
}

}  // namespace forge

using namespace forge;

// parts per row group: 4 when two-part workgroups (64 rows each) would not give every CU two workgroups (MI355X in SPX mode: 256 CUs -> fewer than
// 512 tiles). MI355X only, as the whole library: the constant is not derived from the device properties. `split` is the walked dimension.
static bool attention_split4(int B, int rows, int split) { return split % 128 == 0 && (long long)B * (rows / 64) < 2 * 256; }

static int attention_fwd_launch(const char* name, const float* q, const float* k, const float* v, long long v_batch_rows, float* out, float* lse, int B,
                                int Nq, int Nk, int d, forge_stream_t stream) {
    FORGE_REQUIRE(q && k && v && out, FORGE_EINVAL, "%s: null pointer argument", name);
    FORGE_REQUIRE(d == ATT_D, FORGE_ESHAPE, "%s: one head of %d channels (got d=%d)", name, ATT_D, d);
    FORGE_REQUIRE(B > 0 && Nq > 0 && Nk > 0 && Nq % 64 == 0 && Nk % 64 == 0, FORGE_ESHAPE, "%s: B=%d Nq=%d Nk=%d (Nq and Nk must be multiples of 64)", name, B,
                  Nq, Nk);
    const bool ks4 = attention_split4(B, Nq, Nk);
    FORGE_REQUIRE(v_batch_rows == 0 || v_batch_rows >= Nk, FORGE_EINVAL, "%s: v batch stride %lld rows (0 = one v for every batch element, else >= Nk)", name,
                  v_batch_rows);
    FORGE_REQUIRE((long long)B * (Nq / 64) < (1ll << 31), FORGE_ESHAPE, "%s: too many query tiles", name);
    const dim3 g4((unsigned)(B * (Nq / 32))), g2((unsigned)(B * (Nq / 64)));
    if (lse) {
        if (ks4)
            hipLaunchKernelGGL((attention_fwd_kernel<4, true>), g4, dim3(256), 0, (hipStream_t)stream, q, k, v, v_batch_rows, out, lse, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_fwd_kernel<2, true>), g2, dim3(256), 0, (hipStream_t)stream, q, k, v, v_batch_rows, out, lse, Nq, Nk);
    } else {
        if (ks4)
            hipLaunchKernelGGL((attention_fwd_kernel<4, false>), g4, dim3(256), 0, (hipStream_t)stream, q, k, v, v_batch_rows, out, lse, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_fwd_kernel<2, false>), g2, dim3(256), 0, (hipStream_t)stream, q, k, v, v_batch_rows, out, lse, Nq, Nk);
    }
    FORGE_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int forge_attention_fwd(const float* q, const float* k, const float* v, long long v_batch_rows, float* out, int B, int Nq, int Nk, int d,
                                   forge_stream_t stream) {
    return attention_fwd_launch("forge_attention_fwd", q, k, v, v_batch_rows, out, nullptr, B, Nq, Nk, d, stream);
}

extern "C" int forge_attention_fwd_lse(const float* q, const float* k, const float* v, long long v_batch_rows, float* out, float* lse, int B, int Nq, int Nk,
                                       int d, forge_stream_t stream) {
    FORGE_REQUIRE(lse, FORGE_EINVAL, "forge_attention_fwd_lse: null pointer argument");
    return attention_fwd_launch("forge_attention_fwd_lse", q, k, v, v_batch_rows, out, lse, B, Nq, Nk, d, stream);
}

extern "C" int forge_attention_bwd(const float* q, const float* k, const float* v, long long v_batch_rows, const float* out, const float* lse,
                                   const float* dout, float* dq, float* dk, float* dv, float* delta_ws, int B, int Nq, int Nk, int d,
                                   forge_stream_t stream) {
    FORGE_REQUIRE(q && k && v && out && lse && dout && dq && dk && delta_ws, FORGE_EINVAL, "forge_attention_bwd: null pointer argument");
    FORGE_REQUIRE(d == ATT_D, FORGE_ESHAPE, "forge_attention_bwd: one head of %d channels (got d=%d)", ATT_D, d);
    FORGE_REQUIRE(B > 0 && Nq > 0 && Nk > 0 && Nq % 64 == 0 && Nk % 64 == 0, FORGE_ESHAPE,
                  "forge_attention_bwd: B=%d Nq=%d Nk=%d (Nq and Nk must be multiples of 64)", B, Nq, Nk);
    FORGE_REQUIRE(v_batch_rows == 0 || v_batch_rows >= Nk, FORGE_EINVAL,
                  "forge_attention_bwd: v batch stride %lld rows (0 = one v for every batch element, else >= Nk)", v_batch_rows);
    FORGE_REQUIRE(v_batch_rows != 0 || !dv, FORGE_EINVAL,
                  "forge_attention_bwd: dv with one v shared by the batch (v_batch_rows = 0): the shared table is not trained, pass dv = NULL");
    FORGE_REQUIRE((long long)B * (Nq / 32) < (1ll << 31) && (long long)B * (Nk / 32) < (1ll << 31), FORGE_ESHAPE, "forge_attention_bwd: too many tiles");
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(attention_delta_kernel, dim3((unsigned)(rows / 16)), dim3(256), 0, st, out, dout, delta_ws, rows);
    FORGE_LAUNCH_CHECK("forge_attention_bwd (delta)");
    if (attention_split4(B, Nq, Nk))
        hipLaunchKernelGGL(attention_bwd_dq_kernel<4>, dim3((unsigned)(B * (Nq / 32))), dim3(256), 0, st, q, k, v, v_batch_rows, lse, delta_ws, dout, dq, Nq, Nk);
    else
        hipLaunchKernelGGL(attention_bwd_dq_kernel<2>, dim3((unsigned)(B * (Nq / 64))), dim3(256), 0, st, q, k, v, v_batch_rows, lse, delta_ws, dout, dq, Nq, Nk);
    FORGE_LAUNCH_CHECK("forge_attention_bwd (dq)");
    const bool qs4 = attention_split4(B, Nk, Nq);
    const dim3 grid((unsigned)(B * (Nk / (qs4 ? 32 : 64))));
    if (dv) {
        if (qs4)
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<4, true>), grid, dim3(256), 0, st, q, k, v, v_batch_rows, lse, delta_ws, dout, dk, dv, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<2, true>), grid, dim3(256), 0, st, q, k, v, v_batch_rows, lse, delta_ws, dout, dk, dv, Nq, Nk);
    } else {
        if (qs4)
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<4, false>), grid, dim3(256), 0, st, q, k, v, v_batch_rows, lse, delta_ws, dout, dk, dv, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<2, false>), grid, dim3(256), 0, st, q, k, v, v_batch_rows, lse, delta_ws, dout, dk, dv, Nq, Nk);
    }
    FORGE_LAUNCH_CHECK("forge_attention_bwd (dk, dv)");
    return 0;
}
