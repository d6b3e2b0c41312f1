// attention.hip — dot-product attention O = softmax(scale Q K^T) V, one head of 64 channels per batch index, in fp32 on the matrix cores, for the N = 4096-token attentions of the
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
// Multi-head (opt-in on the Python side: forge_attention_mh_fwd / forge_attention_mh_bwd, the six attention blocks of the 2-D pose estimator,
// models/model_utils.py:258-342): the SAME kernels. A batch index is (b, head) = (bh / H, bh % H) and finds row r of its head inside a
// [B, N, H 64] row at x + b x_bs + r x_rs + 64 head (AttAddr, strides in floats) - the head split / merge copies of the stock module are
// addressing here - and the logit scale rides on the one multiply Q gets anyway: q (scale log2 e). The single-head entry points are H = 1, row
// stride 64, scale = 1 (1.0f * LOG2E is LOG2E: their bits do not move).
#include <cmath>
#include <cstdint>

#include "common.h"

namespace forge {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int ATT_D = 64;          // channels of q / k and of v (one head)
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float LN2 = 0.69314718055994530942f;

// where batch index bh = b H + head finds its rows: row r of q at q + b q_bs + r q_rs + 64 head; k, v and out alike. In floats; multiples of 4
// (float4 loads and stores). lse / delta are [B][H][N] dense, dout / dq / dk / dv [B][N][H 64] dense.
struct AttAddr {
    long long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;
};

// LSE (training, forge_attention_fwd_lse): additionally lse[bh][query] = ln sum_keys exp(scale q . k), from the merged M and den of the last stage.
// qscale = scale log2 e.
template <int KS, bool LSE>
__global__ __launch_bounds__(256) void attention_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            AttAddr ad, int H, float qscale, float* __restrict__ out, float* __restrict__ lse, int Nq,
                                                            int Nk) {
    constexpr int QW = 4 / KS;                             // query groups (of 32) per workgroup
    __shared__ float mrg[3][64][35];                       // key parts 1.. of a query group: (O^T column: 32 floats, max, sum) per lane, padded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, n = lane & 31;
    const int qtiles = Nq / (32 * QW);
    const int bh = blockIdx.x / qtiles, qt = blockIdx.x - bh * qtiles;
    const int b = bh / H, hd = bh - b * H;
    const int qw = wave % QW, kh = wave / QW;
    const int q0 = (qt * QW + qw) << 5;
    const int kbeg = kh * (Nk / KS), kend = kbeg + Nk / KS;
    const float* Kb = k + b * ad.k_bs + ATT_D * hd;
    const float* Vb = v + b * ad.v_bs + ATT_D * hd;

    // B operand of S^T = K Q^T: lane (query n, half h) holds Q[q0 + n][32 h + s] for MFMA step s (the two channels one step contracts are
    // s and 32 + s: any pairing of the 64 channels is the same sum up to the order of the additions)
    float qr[32], kr[32], kn[32];
    {
        const float4* p = reinterpret_cast<const float4*>(q + b * ad.q_bs + (q0 + n) * ad.q_rs + ATT_D * hd + 32 * h);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float4 t = p[i]; qr[4 * i] = t.x * qscale; qr[4 * i + 1] = t.y * qscale; qr[4 * i + 2] = t.z * qscale; qr[4 * i + 3] = t.w * qscale; }
        const float4* pk = reinterpret_cast<const float4*>(Kb + (kbeg + n) * ad.k_rs + 32 * h);
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
            const float* pv = Vb + (kt + 8 * (r >> 2) + 4 * h + (r & 3)) * ad.v_rs + n;
            v0[r] = pv[0];
            v1[r] = pv[32];
        }
        const int ktn = kt + 32 < kend ? kt + 32 : kbeg;            // (the last iteration re-reads the first tile: no branch around the loads)
        {
            const float4* pk = reinterpret_cast<const float4*>(Kb + (ktn + n) * ad.k_rs + 32 * h);
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
            // M and den are in base 2 (Q was pre-multiplied by scale log2 e): ln sum exp = (M + log2 den) ln 2, rounded once at the size of the result;
            // both half-waves hold the same M and den, one of them stores
            if (h == 0) lse[(size_t)bh * Nq + q0 + n] = fmaf(M, LN2, __log2f(den) * LN2);
        }
        // accumulator register r of half h = channel 8 (r / 4) + 4 h + r % 4 (o1: + 32) of query n: four consecutive channels per float4
        float* po = out + b * ad.o_bs + (q0 + n) * ad.o_rs + ATT_D * hd + 4 * h;
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
// With a logit scale c (S = c Q K^T): P and dS = P o (dP - delta) are functions of the scaled logits alone - P is recomputed from q (c log2 e) and
// the lse of the scaled logits, dP and delta do not see c - and the chain rule puts c on the two gradients that pass through S:
//   dQ = c dS K            dK = c dS^T Q            (dV = P^T dO unchanged)
// The residual lives in the dS domain as well: r = sum_keys dS, Z = sum_keys P and Bk = P K are what they were, rho = r / Z is the same shift of
// delta, and the corrected gradient is dQ = c (dS - rho P) K = c (A - rho Bk) with A = dS K: the correction is applied first, c multiplies the
// corrected accumulator once at the store (and dK's at its store). c = 1 multiplies by 1.0f: the single-head bits do not move.

// delta[b][head][r] = sum_c dout[b][r][head][c] out[b][r][head][c]: 16 lanes per (row, head), a float4 each, fixed-order exchange, in the order
// dout lies in memory ([B][Nq][H 64] dense; out by its strides). rows = B Nq H is a multiple of 64 and below 2^31: every wave is full.
__global__ __launch_bounds__(256) void attention_delta_kernel(const float* __restrict__ out, long long o_bs, long long o_rs,
                                                              const float* __restrict__ dout, float* __restrict__ delta, int rows, int Nq, int H) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(t >> 4);
    if (row >= rows) return;
    const int br = row / H, hd = row - br * H;
    const int b = br / Nq, r = br - b * Nq;
    const float4 a = *reinterpret_cast<const float4*>(out + b * o_bs + r * o_rs + ATT_D * hd + 4 * (t & 15));
    const float4 g = *reinterpret_cast<const float4*>(dout + (long long)row * ATT_D + 4 * (t & 15));
    float s = a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if ((t & 15) == 0) delta[((long long)b * H + hd) * Nq + r] = s;
}

// 32 rows x 64 channels of a row-major matrix (row stride rs floats; x = channel 0 of the head) as the A / B operand of a channel contraction:
// lane (row n, half h) holds x[row0 + n][32 h + s] for MFMA step s, times `scale`
__device__ __forceinline__ void load_rows(float (&r)[32], const float* __restrict__ x, long long rs, int row0, int n, int h, float scale = 1.f) {
    const float4* p = reinterpret_cast<const float4*>(x + (row0 + n) * rs + 32 * h);
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float4 t = p[i]; r[4 * i] = t.x * scale; r[4 * i + 1] = t.y * scale; r[4 * i + 2] = t.z * scale; r[4 * i + 3] = t.w * scale; }
}

// the same 32 rows as the A operand of a contraction over the ROWS, in the order an accumulator holds them: register r of half h = row
// 8 (r / 4) + 4 h + r % 4, lane n = channel n (c0) and 32 + n (c1)
__device__ __forceinline__ void load_cols(float (&c0)[16], float (&c1)[16], const float* __restrict__ x, long long rs, int row0, int n, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float* p = x + (row0 + 8 * (r >> 2) + 4 * h + (r & 3)) * rs + n;
        c0[r] = p[0];
        c1[r] = p[32];
    }
}

// store a [channel][row] accumulator pair (lane = row n, register r of half h = channel 8 (r / 4) + 4 h + r % 4, a1: + 32) to row-major x
__device__ __forceinline__ void store_acc(float* __restrict__ x, long long rs, int row0, int n, int h, const f16v& a0, const f16v& a1) {
    float* po = x + (row0 + n) * rs + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(po + 8 * g) = make_float4(a0[4 * g], a0[4 * g + 1], a0[4 * g + 2], a0[4 * g + 3]);
        *reinterpret_cast<float4*>(po + 32 + 8 * g) = make_float4(a1[4 * g], a1[4 * g + 1], a1[4 * g + 2], a1[4 * g + 3]);
    }
}

// dQ pass: the forward's walk (a wave owns 32 queries = lanes, KS key parts per query merged through LDS) plus two GEMMs per tile:
//   S^T = K Q^T, dP^T = V dO^T (accumulator registers = keys), P^T and dS^T = P^T o (dP^T - delta) in place, dQ^T += K^T dS^T and Bk^T += K^T P^T with the
//   dS^T / P^T registers as B operand; row sums r and Z per lane; at the end the residual correction (above) and the logit scale, delta updated in
//   place for the next pass
// (launch bounds: 2 waves per SIMD. Left to itself the compiler takes 161 VGPRs + 96 AGPRs for KS = 4, one register over the budget of two waves.)
template <int KS>
__global__ __launch_bounds__(256, 2) void attention_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                               AttAddr ad, int H, float scale, float qscale, const float* __restrict__ lse,
                                                               float* __restrict__ delta, const float* __restrict__ dout, float* __restrict__ dq, int Nq,
                                                               int Nk) {
    constexpr int QW = 4 / KS;
    __shared__ float mrg[3][64][67];                       // key parts 1.. of a query group: (dQ^T, Bk^T columns: 2 x 32 floats, r, Z) per lane, padded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, n = lane & 31;
    const int qtiles = Nq / (32 * QW);
    const int bh = blockIdx.x / qtiles, qt = blockIdx.x - bh * qtiles;
    const int b = bh / H, hd = bh - b * H;
    const int qw = wave % QW, kh = wave / QW;
    const int q0 = (qt * QW + qw) << 5;
    const int kbeg = kh * (Nk / KS), kend = kbeg + Nk / KS;
    const float* Kb = k + b * ad.k_bs + ATT_D * hd;
    const float* Vb = v + b * ad.v_bs + ATT_D * hd;
    const long long gs = (long long)H * ATT_D;             // row stride of the dense dout / dq
    const size_t qrow0 = (size_t)bh * Nq + q0;             // in lse / delta

    float qr[32], gr[32];
    load_rows(qr, q + b * ad.q_bs + ATT_D * hd, ad.q_rs, q0, n, h, qscale);      // as the forward: S^T in base 2
    load_rows(gr, dout + (long long)b * Nq * gs + ATT_D * hd, gs, q0, n, h);
    const float ls = lse[qrow0 + n], dl = delta[qrow0 + n];
    f16v a0, a1, b0, b1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a0[r] = 0.f; a1[r] = 0.f; b0[r] = 0.f; b1[r] = 0.f; }
    float rs = 0.f, zs = 0.f;                              // this lane's keys (its half-wave's registers): the halves are added after the walk

    for (int kt = kbeg; kt < kend; kt += 32) {
        float kr[32], vr[32], k0[16], k1[16];
        load_rows(kr, Kb, ad.k_rs, kt, n, h);
        load_rows(vr, Vb, ad.v_rs, kt, n, h);
        load_cols(k0, k1, Kb, ad.k_rs, kt, n, h);
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
        for (int r = 0; r < 16; ++r) { a0[r] = fmaf(-rho, b0[r], a0[r]) * scale; a1[r] = fmaf(-rho, b1[r], a1[r]) * scale; }
        store_acc(dq + (long long)b * Nq * gs + ATT_D * hd, gs, q0, n, h, a0, a1);
        if (h == 0) delta[qrow0 + n] = dl + rho;
    }
}

// dK / dV pass: the transposed walk. A wave owns 32 keys (= lanes; K and V rows resident as B operands) and walks the query tiles of its part (QS
// parts per key group, merged through LDS in the order of the parts):
//   S = Q K^T, dP = dO V^T (accumulator registers = queries: lse and delta are indexed by register), dS = P o (dP - delta) in place,
//   dV^T += dO^T P, dK^T += Q^T dS with the P / dS registers as B operand, dK times the logit scale at the store. DV = false (one value table for the whole batch, not trained): no dV chain.
template <int QS, bool DV>
__global__ __launch_bounds__(256) void attention_bwd_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                AttAddr ad, int H, float scale, float qscale, const float* __restrict__ lse,
                                                                const float* __restrict__ delta, const float* __restrict__ dout,
                                                                float* __restrict__ dk, float* __restrict__ dv, int Nq, int Nk) {
    constexpr int KW = 4 / QS;                             // key groups (of 32) per workgroup
    constexpr int MW = DV ? 65 : 33;                       // dK^T (and dV^T) column of a lane, padded
    __shared__ float mrg[3][64][MW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, n = lane & 31;
    const int ktiles = Nk / (32 * KW);
    const int bh = blockIdx.x / ktiles, kt = blockIdx.x - bh * ktiles;
    const int b = bh / H, hd = bh - b * H;
    const int kw = wave % KW, qh = wave / KW;
    const int k0 = (kt * KW + kw) << 5;
    const int qbeg = qh * (Nq / QS), qend = qbeg + Nq / QS;
    const long long gs = (long long)H * ATT_D;             // row stride of the dense dout / dk / dv
    const float* Qb = q + b * ad.q_bs + ATT_D * hd;
    const float* Gb = dout + (long long)b * Nq * gs + ATT_D * hd;
    const float* Lb = lse + (size_t)bh * Nq;
    const float* Db = delta + (size_t)bh * Nq;

    float kr[32], vr[32];
    load_rows(kr, k + b * ad.k_bs + ATT_D * hd, ad.k_rs, k0, n, h);
    load_rows(vr, v + b * ad.v_bs + ATT_D * hd, ad.v_rs, k0, n, h);
    f16v dk0, dk1, dv0, dv1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }

    for (int qt = qbeg; qt < qend; qt += 32) {
        float qr[32], gr[32], q0[16], q1[16], g0[16], g1[16], ls[16], dl[16];
        load_rows(qr, Qb, ad.q_rs, qt, n, h, qscale);        // the forward's products (q scale log2 e) k, with A and B operand exchanged
        load_rows(gr, Gb, gs, qt, n, h);
        load_cols(q0, q1, Qb, ad.q_rs, qt, n, h);
        if constexpr (DV) load_cols(g0, g1, Gb, gs, qt, n, h);
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
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk0[r] *= scale; dk1[r] *= scale; }
        store_acc(dk + (long long)b * Nk * gs + ATT_D * hd, gs, k0, n, h, dk0, dk1);
        if constexpr (DV) store_acc(dv + (long long)b * Nk * gs + ATT_D * hd, gs, k0, n, h, dv0, dv1);
    }
}

}  // namespace forge

using namespace forge;

// parts per row group: 4 when two-part workgroups (64 rows each) would not give every CU two workgroups (MI355X in SPX mode: 256 CUs -> fewer than
// 512 tiles). MI355X only, as the whole library: the constant is not derived from the device properties. `split` is the walked dimension, B the
// number of batch indices (batch elements x heads).
static bool attention_split4(int B, int rows, int split) { return split % 128 == 0 && (long long)B * (rows / 64) < 2 * 256; }

static bool att_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the argument checks every entry point makes after its null-pointer check and before its launcher: head width, token counts, head count, strides, scale
static int attention_check(const char* name, const float* q, const float* k, const float* v, const float* out, const AttAddr& ad, int B, int H, int Nq,
                           int Nk, int d, float scale) {
    FORGE_REQUIRE(d == ATT_D, FORGE_ESHAPE, "%s: one head of %d channels (got d=%d)", name, ATT_D, d);
    FORGE_REQUIRE(B > 0 && Nq > 0 && Nk > 0 && Nq % 64 == 0 && Nk % 64 == 0, FORGE_ESHAPE, "%s: B=%d Nq=%d Nk=%d (Nq and Nk must be multiples of 64)", name, B,
                  Nq, Nk);
    FORGE_REQUIRE(H >= 1, FORGE_ESHAPE, "%s: H=%d heads (at least one)", name, H);
    FORGE_REQUIRE((long long)B * H * Nq < (1ll << 31) && (long long)B * H * Nk < (1ll << 31), FORGE_ESHAPE, "%s: B=%d H=%d Nq=%d Nk=%d: too many rows", name, B, H,
                  Nq, Nk);
    const long long st[8] = {ad.q_bs, ad.q_rs, ad.k_bs, ad.k_rs, ad.v_bs, ad.v_rs, ad.o_bs, ad.o_rs};
    for (int i = 0; i < 8; ++i)
        FORGE_REQUIRE(st[i] >= 0 && st[i] % 4 == 0, FORGE_ESHAPE, "%s: %c %s stride %lld floats (strides must be non-negative multiples of 4: float4 access)", name,
                      "qkvo"[i / 2], i % 2 ? "row" : "batch", st[i]);
    FORGE_REQUIRE(ad.o_rs >= (long long)H * ATT_D && (B == 1 || ad.o_bs >= Nq * ad.o_rs), FORGE_ESHAPE,
                  "%s: out row stride %lld / batch stride %lld floats: rows of H*%d = %d floats would overlap", name, ad.o_rs, ad.o_bs, ATT_D, H * ATT_D);
    FORGE_REQUIRE(att_aligned(q) && att_aligned(k) && att_aligned(v) && att_aligned(out), FORGE_EINVAL, "%s: q, k, v and out must be 16-byte aligned (float4 access)",
                  name);
    FORGE_REQUIRE(std::isfinite(scale) && scale > 0.f, FORGE_EINVAL, "%s: scale %g (a finite positive logit scale)", name, (double)scale);
    return 0;
}

static int attention_fwd_launch(const char* name, const float* q, const float* k, const float* v, const AttAddr& ad, float* out, float* lse, int B, int H,
                                int Nq, int Nk, int d, float scale, forge_stream_t stream) {
    const int BH = B * H;
    const bool ks4 = attention_split4(BH, Nq, Nk);
    const float qscale = scale * LOG2E;
    const dim3 g4((unsigned)(BH * (Nq / 32))), g2((unsigned)(BH * (Nq / 64)));
    if (lse) {
        if (ks4)
            hipLaunchKernelGGL((attention_fwd_kernel<4, true>), g4, dim3(256), 0, (hipStream_t)stream, q, k, v, ad, H, qscale, out, lse, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_fwd_kernel<2, true>), g2, dim3(256), 0, (hipStream_t)stream, q, k, v, ad, H, qscale, out, lse, Nq, Nk);
    } else {
        if (ks4)
            hipLaunchKernelGGL((attention_fwd_kernel<4, false>), g4, dim3(256), 0, (hipStream_t)stream, q, k, v, ad, H, qscale, out, lse, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_fwd_kernel<2, false>), g2, dim3(256), 0, (hipStream_t)stream, q, k, v, ad, H, qscale, out, lse, Nq, Nk);
    }
    FORGE_LAUNCH_CHECK(name);
    return 0;
}

static int attention_bwd_launch(const char* name, const float* q, const float* k, const float* v, const AttAddr& ad, const float* out, const float* lse,
                                const float* dout, float* dq, float* dk, float* dv, float* delta_ws, int B, int H, int Nq, int Nk, int d, float scale,
                                forge_stream_t stream) {
    FORGE_REQUIRE(att_aligned(dout) && att_aligned(dq) && att_aligned(dk) && att_aligned(dv) && att_aligned(lse) && att_aligned(delta_ws), FORGE_EINVAL,
                  "%s: lse, dout, dq, dk, dv and delta_ws must be 16-byte aligned (float4 access)", name);
    hipStream_t st = (hipStream_t)stream;
    const int BH = B * H, rows = BH * Nq;
    const float qscale = scale * LOG2E;
    hipLaunchKernelGGL(attention_delta_kernel, dim3((unsigned)(rows / 16)), dim3(256), 0, st, out, ad.o_bs, ad.o_rs, dout, delta_ws, rows, Nq, H);
    FORGE_LAUNCH_CHECK(name);
    if (attention_split4(BH, Nq, Nk))
        hipLaunchKernelGGL(attention_bwd_dq_kernel<4>, dim3((unsigned)(BH * (Nq / 32))), dim3(256), 0, st, q, k, v, ad, H, scale, qscale, lse, delta_ws, dout, dq, Nq,
                           Nk);
    else
        hipLaunchKernelGGL(attention_bwd_dq_kernel<2>, dim3((unsigned)(BH * (Nq / 64))), dim3(256), 0, st, q, k, v, ad, H, scale, qscale, lse, delta_ws, dout, dq, Nq,
                           Nk);
    FORGE_LAUNCH_CHECK(name);
    const bool qs4 = attention_split4(BH, Nk, Nq);
    const dim3 grid((unsigned)(BH * (Nk / (qs4 ? 32 : 64))));
    if (dv) {
        if (qs4)
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<4, true>), grid, dim3(256), 0, st, q, k, v, ad, H, scale, qscale, lse, delta_ws, dout, dk, dv, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<2, true>), grid, dim3(256), 0, st, q, k, v, ad, H, scale, qscale, lse, delta_ws, dout, dk, dv, Nq, Nk);
    } else {
        if (qs4)
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<4, false>), grid, dim3(256), 0, st, q, k, v, ad, H, scale, qscale, lse, delta_ws, dout, dk, dv, Nq, Nk);
        else
            hipLaunchKernelGGL((attention_bwd_dkv_kernel<2, false>), grid, dim3(256), 0, st, q, k, v, ad, H, scale, qscale, lse, delta_ws, dout, dk, dv, Nq, Nk);
    }
    FORGE_LAUNCH_CHECK(name);
    return 0;
}

// the single-head layout [B][N][64] dense, v with its batch stride in rows (0 = shared)
static AttAddr attention_dense(int Nq, int Nk, long long v_batch_rows) {
    return AttAddr{(long long)Nq * ATT_D, ATT_D, (long long)Nk * ATT_D, ATT_D, v_batch_rows * ATT_D, ATT_D, (long long)Nq * ATT_D, ATT_D};
}

#define ATT_REQUIRE_V_ROWS(name)                                                                                                                  \
    FORGE_REQUIRE(v_batch_rows == 0 || v_batch_rows >= Nk, FORGE_EINVAL, name ": v batch stride %lld rows (0 = one v for every batch element, else >= Nk)", \
                  v_batch_rows)

extern "C" int forge_attention_fwd(const float* q, const float* k, const float* v, long long v_batch_rows, float* out, int B, int Nq, int Nk, int d,
                                   forge_stream_t stream) {
    FORGE_REQUIRE(q && k && v && out, FORGE_EINVAL, "forge_attention_fwd: null pointer argument");
    const AttAddr ad = attention_dense(Nq, Nk, v_batch_rows);
    if (const int rc = attention_check("forge_attention_fwd", q, k, v, out, ad, B, 1, Nq, Nk, d, 1.f)) return rc;
    ATT_REQUIRE_V_ROWS("forge_attention_fwd");
    return attention_fwd_launch("forge_attention_fwd", q, k, v, ad, out, nullptr, B, 1, Nq, Nk, d, 1.f, stream);
}

extern "C" int forge_attention_fwd_lse(const float* q, const float* k, const float* v, long long v_batch_rows, float* out, float* lse, int B, int Nq, int Nk,
                                       int d, forge_stream_t stream) {
    FORGE_REQUIRE(q && k && v && out && lse, FORGE_EINVAL, "forge_attention_fwd_lse: null pointer argument");
    const AttAddr ad = attention_dense(Nq, Nk, v_batch_rows);
    if (const int rc = attention_check("forge_attention_fwd_lse", q, k, v, out, ad, B, 1, Nq, Nk, d, 1.f)) return rc;
    ATT_REQUIRE_V_ROWS("forge_attention_fwd_lse");
    return attention_fwd_launch("forge_attention_fwd_lse", q, k, v, ad, out, lse, B, 1, Nq, Nk, d, 1.f, stream);
}

extern "C" int forge_attention_bwd(const float* q, const float* k, const float* v, long long v_batch_rows, const float* out, const float* lse,
                                   const float* dout, float* dq, float* dk, float* dv, float* delta_ws, int B, int Nq, int Nk, int d,
                                   forge_stream_t stream) {
    FORGE_REQUIRE(q && k && v && out && lse && dout && dq && dk && delta_ws, FORGE_EINVAL, "forge_attention_bwd: null pointer argument");
    const AttAddr ad = attention_dense(Nq, Nk, v_batch_rows);
    if (const int rc = attention_check("forge_attention_bwd", q, k, v, out, ad, B, 1, Nq, Nk, d, 1.f)) return rc;
    ATT_REQUIRE_V_ROWS("forge_attention_bwd");
    FORGE_REQUIRE(v_batch_rows != 0 || !dv, FORGE_EINVAL,
                  "forge_attention_bwd: dv with one v shared by the batch (v_batch_rows = 0): the shared table is not trained, pass dv = NULL");
    return attention_bwd_launch("forge_attention_bwd", q, k, v, ad, out, lse, dout, dq, dk, dv, delta_ws, B, 1, Nq, Nk, d,
                                1.f, stream);
}

extern "C" int forge_attention_mh_fwd(const float* q, const float* k, const float* v, float* out, float* lse, int B, int H, int Nq, int Nk, int d,
                                      long long q_bs, long long q_rs, long long k_bs, long long k_rs, long long v_bs, long long v_rs, long long out_bs,
                                      long long out_rs, float scale, forge_stream_t stream) {
    FORGE_REQUIRE(q && k && v && out, FORGE_EINVAL, "forge_attention_mh_fwd: null pointer argument");
    const AttAddr ad{q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, out_bs, out_rs};
    if (const int rc = attention_check("forge_attention_mh_fwd", q, k, v, out, ad, B, H, Nq, Nk, d, scale)) return rc;
    FORGE_REQUIRE(att_aligned(lse), FORGE_EINVAL, "forge_attention_mh_fwd: lse must be 16-byte aligned");
    return attention_fwd_launch("forge_attention_mh_fwd", q, k, v, ad, out, lse, B, H, Nq, Nk, d, scale,
                                stream);
}

extern "C" int forge_attention_mh_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* dout, float* dq,
                                      float* dk, float* dv, float* delta_ws, int B, int H, int Nq, int Nk, int d, long long q_bs, long long q_rs,
                                      long long k_bs, long long k_rs, long long v_bs, long long v_rs, long long out_bs, long long out_rs, float scale,
                                      forge_stream_t stream) {
    FORGE_REQUIRE(q && k && v && out && lse && dout && dq && dk && delta_ws, FORGE_EINVAL, "forge_attention_mh_bwd: null pointer argument");
    const AttAddr ad{q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, out_bs, out_rs};
    if (const int rc = attention_check("forge_attention_mh_bwd", q, k, v, out, ad, B, H, Nq, Nk, d, scale)) return rc;
    return attention_bwd_launch("forge_attention_mh_bwd", q, k, v, ad, out, lse, dout, dq, dk, dv,
                                delta_ws, B, H, Nq, Nk, d, scale, stream);
}
