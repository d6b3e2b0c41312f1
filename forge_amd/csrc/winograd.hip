// winograd.hip — the 3x3x3 convolutions of the ConvGRU fusion (models/fusion.py:29-35, 61-68, 88-95) with 2.25x fewer multiplies:
// Winograd F(2x2, 3x3) over (H, W), the three depth taps kept as a direct sum.
//
//   y[z, 2th + i, 2tw + j] = sum_kd  A^T [ (G w[kd] G^T) (.) (B^T d[z + kd - 1] B) ] A,    d = the 4x4 input patch at rows 2th - 1 .., cols 2tw - 1 ..
//
//   B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]    G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]    A^T = [1 1 1 0; 0 1 -1 -1]
//
// so that the channel contraction becomes 16 independent GEMMs (one per transformed point p = 4 i + j) over the TILE grid
// (n, D, H/2, W/2) with K = 3 C_in: 12 multiplies per output and channel pair instead of 27. Three launches per convolution:
//   wino_input_kernel    V[p][r][c]  = (B^T d B)[p]           HBM-bound: reads each input row ~once (4x through L2), writes 4x its size
//   forge_wino_gemm      Mm[p] = V[p] (x) U[p]                conv_igemm_kernel, 16 batched 3-tap problems (conv_igemm.hip); fp32 MFMA
//   wino_output_kernel   y = epilogue(A^T Mm A)               HBM-bound: reads 4x the output size, fuses the same element-wise tails
//                                                             as the direct kernel (bias, folded BN + LeakyReLU, GRU gates / state update)
// B^T and A^T hold only 0 / +-1: the transforms are exact additions; the only extra rounding relative to the direct kernel is in
// U = G w G^T (rounded once from a float64 product) and in the order of the fp32 additions. Measured against a float64 convolution the
// fp32 error is 0.43-1.47x (maximum) / 0.60-1.51x (rms) that of the direct fp32 kernel (tests/test_gpu_wino_matrix.py, profiles/r11_wino_matrix.txt).
#include "common.h"

namespace forge {

__device__ __forceinline__ float4 add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float add(float a, float b) { return a + b; }
__device__ __forceinline__ float sub(float a, float b) { return a - b; }
__device__ __forceinline__ float4 fma4(float k, float4 a, float4 b) { return make_float4(fmaf(k, a.x, b.x), fmaf(k, a.y, b.y), fmaf(k, a.z, b.z), fmaf(k, a.w, b.w)); }

// The six lines of B^T of F(4, 3) = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1] on six values p0 .. p5 (q may be p itself), in this
// order (every multiplier is a power of two, so each line is two rounded additions and one fused multiply-add whose product is exact - a plain multiply and
// add gives the same bits):
//   q0 = 4 (p0 - p2) - (p2 - p4)      q1 = (p3 + p4) - 4 (p1 + p2)      q2 = (p4 - p3) + 4 (p1 - p2)
//   q3 = (p4 - p2) + 2 (p3 - p1)      q4 = (p4 - p2) - 2 (p3 - p1)      q5 = 4 (p1 - p3) - (p3 - p5)
// The depth stage of both F(4, 3) nests and the row stage of forge_wino_input_dn4h.
__device__ __forceinline__ void f43_six_lines(float p0, float p1, float p2, float p3, float p4, float p5, float& q0, float& q1, float& q2, float& q3, float& q4,
                                              float& q5) {
    const float a02 = p0 - p2, a24 = p2 - p4, s34 = p3 + p4, s12 = p1 + p2, d43 = p4 - p3, d12 = p1 - p2;
    const float d42 = p4 - p2, d31 = p3 - p1, d13 = p1 - p3, d35 = p3 - p5;
    q0 = fmaf(4.f, a02, -a24);
    q1 = fmaf(-4.f, s12, s34);
    q2 = fmaf(4.f, d12, d43);
    q3 = fmaf(2.f, d31, d42);
    q4 = fmaf(-2.f, d31, d42);
    q5 = fmaf(4.f, d13, -d35);
}

// ---- the pieces the kernels below are written on. Free functions whose arguments are formed where the kernels formed them before they were shared:
// the signatures (a row and its stride instead of a pointer, a shift instead of a factor) keep the compiler's instruction order
// (profiles/r20_wino_forms_isa.txt).
// idx -> (r, c, tw, th, t): thread idx of a [tile rows][per] grid works on tile row r = idx / per and channel c = (idx % per) << cs;
// r = (t Ht + th) Wt + tw with t the plane index (batch element x depth). 32-bit divisions: the launchers refuse 2^31 tile rows.
__device__ __forceinline__ void tile_decode(long long idx, int per, int cs, int Ht, int Wt, unsigned& r, int& c, int& tw, int& th, unsigned& t) {
    r = (unsigned)(idx / per);
    c = (int)(idx - (long long)r * per) << cs;
    unsigned q = r;
    t = q / (unsigned)Wt;
    tw = (int)(q - t * (unsigned)Wt); q = t; t = q / (unsigned)Ht;
    th = (int)(q - t * (unsigned)Ht);
}

// V[4i + j] = (B^T d B)[i][j] of one 4 x 4 patch d (T = float4: four channels; float: one): point p goes to V + row ld + c + p ptv
// the column stage w B of one row w of B^T d: the four points 4 i + j of point row i go to vp + (4 i + j) ptv
template <typename T>
__device__ __forceinline__ void bt_cols_store(const T (&w)[4], float* vp, int i, long long ptv) {
    *reinterpret_cast<T*>(vp + (4 * i + 0) * ptv) = sub(w[0], w[2]);
    *reinterpret_cast<T*>(vp + (4 * i + 1) * ptv) = add(w[1], w[2]);
    *reinterpret_cast<T*>(vp + (4 * i + 2) * ptv) = sub(w[2], w[1]);
    *reinterpret_cast<T*>(vp + (4 * i + 3) * ptv) = sub(w[1], w[3]);
}

template <typename T, typename I>
__device__ __forceinline__ void bt_d_b_store(const T (&d)[4][4], float* V, I row, int ld, int c, long long ptv) {
    T w[4][4];                                       // rows: B^T d
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w[0][j] = sub(d[0][j], d[2][j]);
        w[1][j] = add(d[1][j], d[2][j]);
        w[2][j] = sub(d[2][j], d[1][j]);
        w[3][j] = sub(d[1][j], d[3][j]);
    }
    float* vp = V + (long long)row * ld + c;
#pragma unroll
    for (int i = 0; i < 4; ++i) bt_cols_store(w[i], vp, i, ptv);      // columns: (B^T d) B
}

// dM[4i + j] = (A y A^T)[i][j] of one 2 x 2 output tile y, A = [1 0; 1 1; 1 -1; 0 -1]; point p at mp + p ptm
__device__ __forceinline__ void a_y_at_store(float4 y00, float4 y01, float4 y10, float4 y11, float* mp, long long ptm) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 s[4][2] = {{y00, y01}, {add(y00, y10), add(y01, y11)}, {sub(y00, y10), sub(y01, y11)}, {sub(zero, y10), sub(zero, y11)}};   // A y
#pragma unroll
    for (int i = 0; i < 4; ++i) {                    // (A y) A^T
        *reinterpret_cast<float4*>(mp + (4 * i + 0) * ptm) = s[i][0];
        *reinterpret_cast<float4*>(mp + (4 * i + 1) * ptm) = add(s[i][0], s[i][1]);
        *reinterpret_cast<float4*>(mp + (4 * i + 2) * ptm) = sub(s[i][0], s[i][1]);
        *reinterpret_cast<float4*>(mp + (4 * i + 3) * ptm) = sub(zero, s[i][1]);
    }
}

// Row k of the weight matrix G of a 1-D Winograd form on the three taps w0, w1, w2, in float64:
//   F(2, 3): G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1] (exact on fp32 taps)
//   F(4, 3): G = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1] (the sixths are not exact in float64: the result is the
//            evaluation below, correctly rounded to within one float64 rounding per operation)
__device__ __forceinline__ double depth_row_f23(int k, double w0, double w1, double w2) {
    return k == 0 ? w0 : k == 1 ? 0.5 * (w0 + w1 + w2) : k == 2 ? 0.5 * (w0 - w1 + w2) : w2;
}
__device__ __forceinline__ double depth_row_f43(int k, double w0, double w1, double w2) {
    return k == 0 ? 0.25 * w0 : k == 1 ? -((w0 + w2) + w1) / 6.0 : k == 2 ? -((w0 + w2) - w1) / 6.0
         : k == 3 ? ((0.25 * w0 + w2) + 0.5 * w1) / 6.0 : k == 4 ? ((0.25 * w0 + w2) - 0.5 * w1) / 6.0 : w2;
}

// U[4i + j] = (float)(G_H d G^T)[i][j] of one 3 x 3 kernel slice d in float64, rounded once; point p at up + p pt. G_H = the NH rows HROW of the form along H
// (F(2, 3): 4 rows, 16 points; F(4, 3): 6 rows, 24 points), G = F(2, 3) along W. NW = 6: F(4, 3) along W as well, point 6 i + j = depth_row_f43(j, .) of the three
// W taps of row i (36 points).
template <int NH = 4, double (*HROW)(int, double, double, double) = depth_row_f23, int NW = 4>
__device__ __forceinline__ void g_d_gt_store(const double (&d)[3][3], float* up, long long pt) {
    double g[NH][3];                                 // G_H d
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int i = 0; i < NH; ++i) g[i][b] = HROW(i, d[0][b], d[1][b], d[2][b]);
    if constexpr (NW == 6) {
#pragma unroll
        for (int i = 0; i < NH; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) up[(6 * i + j) * pt] = (float)depth_row_f43(j, g[i][0], g[i][1], g[i][2]);
        return;
    }
#pragma unroll
    for (int i = 0; i < NH; ++i) {                   // (G_H d) G^T
        up[(4 * i + 0) * pt] = (float)g[i][0];
        up[(4 * i + 1) * pt] = (float)(0.5 * (g[i][0] + g[i][1] + g[i][2]));
        up[(4 * i + 2) * pt] = (float)(0.5 * (g[i][0] - g[i][1] + g[i][2]));
        up[(4 * i + 3) * pt] = (float)g[i][2];
    }
}

struct WinoInArgs {
    const float* in; int ld; long long bs;        // rows [n][D][H][W] x ld floats, batch stride bs rows
    float* V; int ldv; long long ptv;             // V[p] = V + p ptv, rows [n][D][H/2][W/2] x ldv floats
    int n, D, H, W, C;
    int nsum; long long ss;                       // nsum > 1: the input is the MEAN of nsum tensors ss rows apart (the view mean of models/encoder.py:62
                                                  // feeding fusion_conv: sum in view order, then x (1 / nsum), as torch.mean) - no separate reduction launch
    float* dM; long long ptm;                     // DY instantiation: also dM[p] = (A y A^T)[p] of the tile's own 2 x 2 pixels y (rows [n][D][H/2][W/2] x C)
};

// one thread = one tile x 4 channels: 16 float4 loads (zero outside the grid), 32 float4 additions, 16 float4 stores.
// DY: the tensor is an upstream gradient that the backward pass needs in BOTH transformed forms - B^T d B for the data-gradient GEMMs and
// A y A^T (wino_dy_kernel) for the weight-gradient GEMMs; the 2 x 2 pixels of the latter are the centre of the patch already in registers,
// so one launch writes both (9 instead of 10 passes of the tensor's size, one launch less per gradient).
template <bool DY>
__global__ __launch_bounds__(256) void wino_input_kernel(const WinoInArgs a) {
    const int C4 = a.C >> 2, Ht = a.H >> 1, Wt = a.W >> 1;
    // each XCD transforms one CONTIGUOUS slab of tiles: neighbouring tiles share half of their 4 x 4 input patches, and with the dispatcher's
    // round-robin order every XCD's private L2 fetched most of the input again (r03 PMC: 102.5 MB moved for 83.9 MB). Placement only.
    const long long idx = (long long)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    const long long R = (long long)a.n * a.D * Ht * Wt;
    if (idx >= R * C4) return;
    unsigned r, t;
    int c, tw, th;
    tile_decode(idx, C4, 2, Ht, Wt, r, c, tw, th, t);
    const unsigned q = t; t = q / (unsigned)a.D;
    const int z = (int)(q - t * (unsigned)a.D);                      // t = batch element
    const float* base = a.in + ((long long)t * a.bs + (long long)z * a.H * a.W) * a.ld + c;
    float4 d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = 2 * th - 1 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = 2 * tw - 1 + j;
            const bool ok = (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                const float* p = base + ((long long)y * a.W + x) * a.ld;
                v = *reinterpret_cast<const float4*>(p);
                if (a.nsum > 1) {
                    for (int k = 1; k < a.nsum; ++k) v = add(v, *reinterpret_cast<const float4*>(p + (long long)k * a.ss * a.ld));
                    const float inv = 1.f / (float)a.nsum;           // ATen divides by a scalar as a multiplication by its fp32 reciprocal
                    v = make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
                }
            }
            d[i][j] = v;
        }
    }
    if constexpr (DY) a_y_at_store(d[1][1], d[1][2], d[2][1], d[2][2], a.dM + (long long)r * a.C + c, a.ptm);    // y = the centre of the patch
    bt_d_b_store(d, a.V, r, a.ldv, c, a.ptv);
}

// The input transform of the F(4, 3) depth nest (forge_wino_input_dn4): wino_input_kernel's B^T d B on the DEPTH-COMBINED patches of a group of four
// planes. Group g of a batch element covers the output planes 4g .. 4g + 3 and reads the planes p_e = plane 4g - 1 + e, e = 0..5 (zero outside the batch
// element's grid, never the neighbouring element's planes). Depth stage, per patch element: q0 .. q5 = f43_six_lines(p0 .. p5), the rows of B^T of F(4, 3);
// then the 2-D stage of wino_input_kernel on each q_k (rows first, then columns). Output V6 [16][n][D/4][6][Ht Wt][C]: position k of group g is plane
// 6 g + k of the element.
// One thread = one tile of one group x ONE channel (96 values live): a wave reads and writes 256 contiguous bytes per instruction, every loaded value is
// used for all six positions (96 loads, 96 stores).
// TH = 4 (forge_wino_input_dn4h): F(4, 3) along H as well - tiles of 4 x 2 output pixels, Ht = H / 4; the patch of tile (th, tw) is the six rows 4 th - 1 ..
// 4 th + 4 x the four columns 2 tw - 1 .. 2 tw + 2. Three stages, in this order:
//   depth   q_k[i][j] = f43_six_lines over the six planes of the group, per patch element                     (the same code as TH = 2)
//   rows    w_k[i'][j] = f43_six_lines over the six patch rows i of q_k, per depth position k and patch column j
//   cols    V[4 i' + j'] = w_k[i'] B of F(2, 3): w0 - w2, w1 + w2, w2 - w1, w1 - w3                             (bt_cols_store: wino_input_kernel's column stage)
// Output V [24][n][D/4][6][Ht Wt][C], point p = 4 i' + j': the same operand layout on the (Ht, Wt) grid with 24 points. 144 loads, 144 values live, 144
// stores per thread (a float4 of channels per thread would need 576 registers). Code object (hipcc -O3, gfx950): 170 VGPRs, no scratch = 2 waves per SIMD
// (TH = 2: 120 VGPRs, 4 waves); per launch 21.9 us against 24.1 us at one scene, 172 against 231 us at eight (profiles/r22_wino_dn4h_launch.txt).
template <int TH>
__global__ __launch_bounds__(256) void wino_input_dn4_kernel(const WinoInArgs a) {
    constexpr int NR = TH + 2;                                       // patch rows
    const int Ht = TH == 4 ? a.H >> 2 : a.H >> 1, Wt = a.W >> 1, Dg = a.D >> 2;
    const long long idx = (long long)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    const long long RG = (long long)a.n * Dg * Ht * Wt;             // group tiles
    if (idx >= RG * a.C) return;
    unsigned r, t;
    int c, tw, th;
    tile_decode(idx, a.C, 0, Ht, Wt, r, c, tw, th, t);
    const unsigned q = t; t = q / (unsigned)Dg;
    const int g = (int)(q - t * (unsigned)Dg);                      // t = batch element
    const long long HW = (long long)a.H * a.W;
    const float* base = a.in + (long long)t * a.bs * a.ld + c;
    const float inv = 1.f / (float)a.nsum;                           // ATen divides by a scalar as a multiplication by its fp32 reciprocal
    float d[6][NR][4];                                               // [depth position k][patch row i][patch column j]
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int y = TH * th - 1 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = 2 * tw - 1 + j;
            const bool ok = (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
            float p[6];
#pragma unroll
            for (int e = 0; e < 6; ++e) {
                const int z = 4 * g - 1 + e;
                float v = 0.f;
                if (ok && (unsigned)z < (unsigned)a.D) {
                    const float* s = base + ((long long)z * HW + (long long)y * a.W + x) * a.ld;
                    v = *s;
                    if (a.nsum > 1) {
                        for (int k = 1; k < a.nsum; ++k) v += s[(long long)k * a.ss * a.ld];
                        v *= inv;
                    }
                }
                p[e] = v;
            }
            f43_six_lines(p[0], p[1], p[2], p[3], p[4], p[5], d[0][i][j], d[1][i][j], d[2][i][j], d[3][i][j], d[4][i][j], d[5][i][j]);
        }
    }
    const long long HWt = (long long)Ht * Wt;
    float* vp = a.V + ((((long long)t * Dg + g) * 6) * HWt + (long long)th * Wt + tw) * a.ldv + c;
    if constexpr (TH == 4) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                f43_six_lines(d[k][0][j], d[k][1][j], d[k][2][j], d[k][3][j], d[k][4][j], d[k][5][j], d[k][0][j], d[k][1][j], d[k][2][j], d[k][3][j], d[k][4][j], d[k][5][j]);
#pragma unroll
            for (int i = 0; i < 6; ++i) bt_cols_store(d[k][i], vp + k * HWt * a.ldv, i, a.ptv);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) bt_d_b_store(d[k], vp, k * HWt, a.ldv, 0, a.ptv);
    }
}

// The input transform of the F(4, 3) nest on depth, H AND W (forge_wino_input_dn4hw): tiles of 4 x 4 output pixels, Ht = H / 4, Wt = W / 4; the patch of tile
// (th, tw) of group g is the planes 4 g - 1 .. 4 g + 4 x the rows 4 th - 1 .. 4 th + 4 x the columns 4 tw - 1 .. 4 tw + 4 (zero outside the batch element's grid).
// Three stages, in this order, all f43_six_lines:
//   depth   q_k[i][j]   over the six planes of the group, per patch element
//   rows    w_k[i'][j]  over the six patch rows i of q_k, per depth position k and patch column j
//   cols    V[6 i' + j'] over the six patch columns j of w_k[i'], per depth position and point row
// Output V [36][n][D/4][6][Ht Wt][C], point p = 6 i' + j'. A tile's 6 x 6 x 6 values per channel do not fit one thread: a tile and channel is split over the THREE
// waves of a 192-thread workgroup by depth-position pairs - (0, 5), (1, 2), (3, 4): the lines 0 and 5 read three planes each, the other four the same four
// planes, so the three waves load 14 planes per patch element (168 loads per wave; the sibling waves' repeats are L1 hits: the same addresses from the same
// workgroup). A wave keeps its two positions: 72 values live, 72 stores. It reads and writes 64 channels = 256 contiguous bytes per instruction. KP is the
// wave's index, uniform, so each wave runs one instantiation of the body.
// Every load is unconditional - the coordinates are clamped into the element's grid and the value is masked to zero outside it - so that the loads issue back
// to back instead of one branch and one wait each (with the loads under their conditions the launch took 34 us where this form takes 27, at one scene).
// MEAN: the view-mean path (nsum > 1), a kernel instantiation of its own.
// Code object (hipcc -O3, gfx950): MEAN = false 165 VGPRs, no scratch = 3 waves per SIMD; MEAN = true 252 VGPRs, no scratch = 2 waves per SIMD.
template <int KP, bool MEAN>
__device__ __forceinline__ void wino_input_dn4hw_body(const WinoInArgs& a, long long idx) {
    const int Ht = a.H >> 2, Wt = a.W >> 2, Dg = a.D >> 2;
    unsigned r, t;
    int c, tw, th;
    tile_decode(idx, a.C, 0, Ht, Wt, r, c, tw, th, t);
    const unsigned q = t; t = q / (unsigned)Dg;
    const int g = (int)(q - t * (unsigned)Dg);                      // t = batch element
    const float* base = a.in + (long long)t * a.bs * a.ld + c;
    const float inv = 1.f / (float)a.nsum;                           // ATen divides by a scalar as a multiplication by its fp32 reciprocal
    constexpr int K0 = KP == 0 ? 0 : 2 * KP - 1, K1 = KP == 0 ? 5 : 2 * KP;      // the pairs (0, 5), (1, 2), (3, 4): lines 0 and 5 read three planes each, the others
    const int kpos[2] = {K0, K1};                                    // the same four - 14 loads per patch element over the three waves instead of 18
    float d[2][6][6];                                                // [depth position kpos[k]][patch row i][patch column j]
    // offsets of the six planes, rows and columns inside the batch element, in floats (32 bits: the entry refuses elements of 2^31 floats), clamped into its grid
    unsigned oz[6], oy[6], ox[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        oz[e] = (unsigned)min(max(4 * g - 1 + e, 0), a.D - 1) * (unsigned)(a.H * a.W) * (unsigned)a.ld;
        oy[e] = (unsigned)min(max(4 * th - 1 + e, 0), a.H - 1) * (unsigned)a.W * (unsigned)a.ld;
        ox[e] = (unsigned)min(max(4 * tw - 1 + e, 0), a.W - 1) * (unsigned)a.ld;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {                                    // one patch column at a time: its loads, depth lines and row lines
        const int x = 4 * tw - 1 + j;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int y = 4 * th - 1 + i;
            const bool ok = (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
            float p[6], o[6];
#pragma unroll
            for (int e = 0; e < 6; ++e) {
                const int z = 4 * g - 1 + e;
                const float* s = base + (oz[e] + oy[i] + ox[j]);
                float v = *s;
                if constexpr (MEAN) {
                    for (int k = 1; k < a.nsum; ++k) v += s[(long long)k * a.ss * a.ld];
                    v *= inv;
                }
                p[e] = __int_as_float(__float_as_int(v) & (ok && (unsigned)z < (unsigned)a.D ? -1 : 0));    // (a mask, not a select: a select of a load becomes a branch again)
            }
            f43_six_lines(p[0], p[1], p[2], p[3], p[4], p[5], o[0], o[1], o[2], o[3], o[4], o[5]);
            d[0][i][j] = o[K0];
            d[1][i][j] = o[K1];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            f43_six_lines(d[k][0][j], d[k][1][j], d[k][2][j], d[k][3][j], d[k][4][j], d[k][5][j], d[k][0][j], d[k][1][j], d[k][2][j], d[k][3][j], d[k][4][j], d[k][5][j]);
    }
    const long long HWt = (long long)Ht * Wt;
    float* vp = a.V + ((((long long)t * Dg + g) * 6) * HWt + (long long)th * Wt + tw) * a.ldv + c;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            float v[6];
            f43_six_lines(d[k][i][0], d[k][i][1], d[k][i][2], d[k][i][3], d[k][i][4], d[k][i][5], v[0], v[1], v[2], v[3], v[4], v[5]);
#pragma unroll
            for (int j = 0; j < 6; ++j) vp[kpos[k] * HWt * a.ldv + (6 * i + j) * a.ptv] = v[j];
        }
    }
}

template <bool MEAN>
__global__ __launch_bounds__(192) void wino_input_dn4hw_kernel(const WinoInArgs a) {
    const long long idx = (long long)xcd_remap(blockIdx.x, gridDim.x) * 64 + (threadIdx.x & 63);
    if (idx >= (long long)a.n * (a.D >> 2) * (a.H >> 2) * (a.W >> 2) * a.C) return;
    const int kp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (kp == 0) wino_input_dn4hw_body<0, MEAN>(a, idx);
    else if (kp == 1) wino_input_dn4hw_body<1, MEAN>(a, idx);
    else wino_input_dn4hw_body<2, MEAN>(a, idx);
}

// U[4i+j][kd][o][c] = (G w[kd] G^T)[i][j] from packed weights wp[(kd 3 + a) 3 + b][co][ci]: one thread per (kd, o, c). Evaluated in float64
// (exact: at most 9 fp32 terms with coefficients 1, 1/2, 1/4) and rounded once. transpose: the weights of the DATA GRADIENT - the
// correlation of dy with the flipped kernel and swapped channel roles: w'[kd][a][b][o = ci][c = co] = wp[(2-kd, 2-a, 2-b)][co][ci].
__global__ __launch_bounds__(256) void wino_weight_kernel(const float* __restrict__ wp, float* __restrict__ U, int Cout, int Cin, int KD, int transpose) {
    const int No = transpose ? Cin : Cout, Nc = transpose ? Cout : Cin;      // U's [o][c] extents
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)No * Nc;
    if (idx >= KD * per) return;                      // KD = 3 depth taps (3x3x3 kernels) or 1 (3x3 kernels of a 2-D convolution)
    const int kd = (int)(idx / per);
    const long long oc = idx - kd * per;
    const int o = (int)(oc / Nc), c = (int)(oc - (long long)o * Nc);
    double w[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int tap = transpose ? ((KD - 1 - kd) * 3 + (2 - a)) * 3 + (2 - b) : (kd * 3 + a) * 3 + b;
            w[a][b] = (double)wp[((long long)tap * Cout + (transpose ? c : o)) * Cin + (transpose ? o : c)];
        }
    g_d_gt_store(w, U + ((long long)kd * No + o) * Nc + c, KD * per);
}

// Weights of the depth nests: U'[4i+j][k][o][c] = sum_kd Gd[k][kd] (G w[kd] G^T)[i][j] over K depth positions k, Gd[k] evaluated by ROW(k, w0, w1, w2) on
// every element of the three depth slices. One thread per (o, c); float64 throughout, rounded once.
//   F(2, 3) (forge_wino_gemm_dn): Gd = G, the rows w0, (w0 + w1 + w2) / 2, (w0 - w1 + w2) / 2, w2 (exact: at most 27 fp32 terms with coefficients 1, 1/2, 1/4, 1/8)
//   F(4, 3) (forge_wino_gemm_dn4): Gd = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1] (the sixths are not exact in float64: the
//           result is depth_row_f43's float64 evaluation, correctly rounded to within one float64 rounding per operation)
//   F(4, 3) on depth AND on H (forge_wino_gemm_dn4h, NH = 6, HROW = the F(4, 3) rows): U''' [24][6][Cout][Cin] = G4(depth) (x) G4(H) (x) G2(W), point p = 4 i + j with
//           i = 0..5 the H point: the depth rows on every element, then the H rows, then the W rows, all in float64, rounded once
//   F(4, 3) on depth, H AND W (forge_wino_weights_dn4hw, NW = 6): U [36][6][Cout][Cin] = G4(depth) (x) G4(H) (x) G4(W), point p = 6 i + j: the depth rows on every
//           element, then the H rows, then the same six rows over the W taps, all in float64, rounded once
// (the rows: depth_row_f23 / depth_row_f43 above g_d_gt_store)
template <int K, double (*ROW)(int, double, double, double), int NH = 4, double (*HROW)(int, double, double, double) = depth_row_f23, int NW = 4>
__global__ __launch_bounds__(256) void wino_weight_nest_kernel(const float* __restrict__ wp, float* __restrict__ U, int Cout, int Cin) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)Cout * Cin;
    if (idx >= per) return;
    double w[3][3][3];
#pragma unroll
    for (int t = 0; t < 27; ++t) w[t / 9][(t / 3) % 3][t % 3] = (double)wp[t * per + idx];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double d[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) d[a][b] = ROW(k, w[0][a][b], w[1][a][b], w[2][a][b]);
        g_d_gt_store<NH, HROW, NW>(d, U + k * per + idx, K * per);
    }
}

enum WinoEpilogue : int { W_BIAS = 0, W_AFFINE_ACT = 1, W_GRU_GATES = 2, W_GRU_OUT = 3 };   // = ConvEpilogue of conv_igemm.hip

struct WinoOutArgs {
    const float* Mm; long long ptm;               // Mm[p] = Mm + p ptm, rows [n][D][H/2][W/2] x Cout floats
    const float* Mm2; long long ptm2, bs2;        // nullable second addend (the input half of conv([x, h], W), shared across fusions):
                                                  // Mm2[p] = Mm2 + p ptm2, batch element n starts at row n bs2 (rows [D][H/2][W/2] x Cout)
    const float* bias; const float* scale; const float* shift; float slope;
    const float* residual;                        // nullable, [rows][Cout]: added to the pre-activation
    const float* aux_h; const float* aux_z;
    float* out; float* out2; float* out3; int ldo;
    int n, D, H, W, Cout, epi;
};

// m[i][j] = plane 4 i + j of Mm (+ of Mm2, when given: the second addend in the same form - the transform is linear) at tile row r, channels c .. c + 3;
// ROWS = 4: the 16 points, 2: the 8 planes of the half form. R1: tile rows per batch element (Mm2's batch elements lie bs2 rows apart)
template <int ROWS>
__device__ __forceinline__ void load_planes(float4 (&m)[ROWS][4], const float* Mm, long long ptm, const float* Mm2, long long ptm2, long long bs2, int Cout, unsigned R1, unsigned r, int c) {
    const float* mp = Mm + (long long)r * Cout + c;
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[i][j] = *reinterpret_cast<const float4*>(mp + (4 * i + j) * ptm);
    if (Mm2) {
        const unsigned nn = r / R1;
        const float* mp2 = Mm2 + ((long long)nn * bs2 + (r - nn * R1)) * Cout + c;
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) m[i][j] = add(m[i][j], *reinterpret_cast<const float4*>(mp2 + (4 * i + j) * ptm2));
    }
}

// one thread = one tile x 4 output channels: 16 float4 loads, 24 float4 additions, then the element-wise tail of 2x2 output voxels
// HALF: Mm (and Mm2) hold 8 planes [2][4] - the row stage s = A^T m was applied by the GEMM's epilogue (forge_wino_gemm_half) - and this kernel runs the
// column stage only (8 instead of 16 float4 loads per operand).
// TH = 4 (forge_wino_output_dn4h): tiles of 4 x 2 voxels, Ht = H / 4, from forge_wino_gemm_dn4h's 24 point products, point p = 4 i + j with i = 0..5 the H
// point: the row stage is A^T of F(4, 3) = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1] in the four lines of the depth-nest GEMM's output schedule
// (s = m1 + m2, d = m1 - m2, S = m3 + m4, D = m3 - m4: (s + S) + m0 | d + 2 D | s + 4 S | (d + 8 D) + m5, the scalings fused and exact); 24 float4 loads, no
// second addend.
template <int EPI, bool HALF = false, int TH = 2>
__global__ __launch_bounds__(256) void wino_output_kernel(const WinoOutArgs a) {
    static_assert(TH == 2 || (TH == 4 && !HALF), "tiles of 2 x 2 voxels, or of 4 x 2 from the 24 points");
    const int C4 = a.Cout >> 2, Ht = TH == 4 ? a.H >> 2 : a.H >> 1, Wt = a.W >> 1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long R = (long long)a.n * a.D * Ht * Wt;
    if (idx >= R * C4) return;
    unsigned r, t;                                   // t = (n, z) plane index
    int c, tw, th;
    tile_decode(idx, C4, 2, Ht, Wt, r, c, tw, th, t);
    float4 s[TH][4];                                 // A^T m
    if constexpr (TH == 4) {
        const float* mp = a.Mm + (long long)r * a.Cout + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float4 m[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) m[i] = *reinterpret_cast<const float4*>(mp + (4 * i + j) * a.ptm);
            const float4 sl = add(m[1], m[2]), dl = sub(m[1], m[2]), Sl = add(m[3], m[4]), Dl = sub(m[3], m[4]);
            s[0][j] = add(add(sl, Sl), m[0]);
            s[1][j] = fma4(2.f, Dl, dl);
            s[2][j] = fma4(4.f, Sl, sl);
            s[3][j] = add(fma4(8.f, Dl, dl), m[5]);
        }
    } else if constexpr (HALF) {
        load_planes<2>(s, a.Mm, a.ptm, a.Mm2, a.ptm2, a.bs2, a.Cout, (unsigned)(a.D * Ht * Wt), r, c);
    } else {
        float4 m[4][4];
        load_planes<4>(m, a.Mm, a.ptm, a.Mm2, a.ptm2, a.bs2, a.Cout, (unsigned)(a.D * Ht * Wt), r, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[0][j] = add(add(m[0][j], m[1][j]), m[2][j]);
            s[1][j] = sub(sub(m[1][j], m[2][j]), m[3][j]);
        }
    }
    float4 y[TH][2];
#pragma unroll
    for (int i = 0; i < TH; ++i) {
        y[i][0] = add(add(s[i][0], s[i][1]), s[i][2]);
        y[i][1] = sub(sub(s[i][1], s[i][2]), s[i][3]);
    }
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f), sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = bias;
    if (a.bias) bias = *reinterpret_cast<const float4*>(a.bias + c);
    if ((EPI == W_AFFINE_ACT || (EPI == W_GRU_OUT && a.out2)) && a.scale) {
        sc = *reinterpret_cast<const float4*>(a.scale + c);
        sh = *reinterpret_cast<const float4*>(a.shift + c);
    }
    const int Ch = a.Cout >> 1;
    const long long plane = (long long)t * a.H * a.W;               // first output row of plane (n, z)
#pragma unroll
    for (int i = 0; i < TH; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long orow = plane + (long long)(TH * th + i) * a.W + (2 * tw + j);
            float v[4] = {y[i][j].x + bias.x, y[i][j].y + bias.y, y[i][j].z + bias.z, y[i][j].w + bias.w};
            if (a.residual) {
                const float4 rr = *reinterpret_cast<const float4*>(a.residual + orow * a.Cout + c);
                v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
            }
            const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
            if constexpr (EPI == W_BIAS) {
                *reinterpret_cast<float4*>(a.out + orow * a.ldo + c) = make_float4(v[0], v[1], v[2], v[3]);
            } else if constexpr (EPI == W_AFFINE_ACT) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float u = fmaf(v[k], scv[k], shv[k]);
                    v[k] = u > 0.f ? u : u * a.slope;
                }
                *reinterpret_cast<float4*>(a.out + orow * a.ldo + c) = make_float4(v[0], v[1], v[2], v[3]);
            } else if constexpr (EPI == W_GRU_GATES) {
                float g[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) g[k] = 1.f / (1.f + expf(-v[k]));      // full-precision exponential, as torch.sigmoid
                if (c < Ch) {
                    *reinterpret_cast<float4*>(a.out + orow * Ch + c) = make_float4(g[0], g[1], g[2], g[3]);
                } else {
                    const float4 h = *reinterpret_cast<const float4*>(a.aux_h + orow * Ch + (c - Ch));
                    *reinterpret_cast<float4*>(a.out2 + orow * Ch + (c - Ch)) = make_float4(h.x * g[0], h.y * g[1], h.z * g[2], h.w * g[3]);
                    if (a.out3) *reinterpret_cast<float4*>(a.out3 + orow * Ch + (c - Ch)) = make_float4(g[0], g[1], g[2], g[3]);
                }
            } else {   // W_GRU_OUT
                const float4 z4 = *reinterpret_cast<const float4*>(a.aux_z + orow * a.Cout + c);
                const float4 h4 = *reinterpret_cast<const float4*>(a.aux_h + orow * a.Cout + c);
                const float zv[4] = {z4.x, z4.y, z4.z, z4.w}, hv[4] = {h4.x, h4.y, h4.z, h4.w};
                float cand[4], hn[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    cand[k] = tanhf(v[k]);
                    hn[k] = hv[k] * (1.f - zv[k]) + cand[k] * zv[k];
                }
                *reinterpret_cast<float4*>(a.out + orow * a.ldo + c) = make_float4(hn[0], hn[1], hn[2], hn[3]);
                if (a.out2)
                    *reinterpret_cast<float4*>(a.out2 + orow * a.ldo + c) =
                        make_float4(fmaf(hn[0], scv[0], shv[0]), fmaf(hn[1], scv[1], shv[1]), fmaf(hn[2], scv[2], shv[2]), fmaf(hn[3], scv[3], shv[3]));
                if (a.out3) *reinterpret_cast<float4*>(a.out3 + orow * a.ldo + c) = make_float4(cand[0], cand[1], cand[2], cand[3]);
            }
        }
}

// A deliberate second copy of wino_output_kernel's GRU tails: with that kernel calling this function its existing instantiations compile to other code (another
// instruction order and register allocation, e.g. <W_GRU_OUT, false, 4> 2559 -> 2581 lines, 168 -> 160 VGPRs), and the steps that do not take the 36-point form
// would no longer run the code they were measured with. A change to either tail is made in both.
// The GRU tails of wino_output_kernel (the same operations in the same order) on the NI x NJ voxels y of one tile and four channels c .. c + 3: voxel (i, j) is
// row y0 + i, column x0 + j of plane t = (n, z). EPI: W_GRU_GATES (z | h r | optional r) or W_GRU_OUT (lerp, optional tanh(c), fusion_norm-folded second output).
template <int EPI, int NI, int NJ>
__device__ __forceinline__ void wino_tail(const WinoOutArgs& a, const float4 (&y)[NI][NJ], unsigned t, int y0, int x0, int c) {
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f), sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = bias;
    if (a.bias) bias = *reinterpret_cast<const float4*>(a.bias + c);
    if (EPI == W_GRU_OUT && a.out2 && a.scale) {
        sc = *reinterpret_cast<const float4*>(a.scale + c);
        sh = *reinterpret_cast<const float4*>(a.shift + c);
    }
    const int Ch = a.Cout >> 1;
    const long long plane = (long long)t * a.H * a.W;               // first output row of plane (n, z)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const long long orow = plane + (long long)(y0 + i) * a.W + (x0 + j);
            float v[4] = {y[i][j].x + bias.x, y[i][j].y + bias.y, y[i][j].z + bias.z, y[i][j].w + bias.w};
            const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
            if constexpr (EPI == W_GRU_GATES) {
                float g[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) g[k] = 1.f / (1.f + expf(-v[k]));      // full-precision exponential, as torch.sigmoid
                if (c < Ch) {
                    *reinterpret_cast<float4*>(a.out + orow * Ch + c) = make_float4(g[0], g[1], g[2], g[3]);
                } else {
                    const float4 h = *reinterpret_cast<const float4*>(a.aux_h + orow * Ch + (c - Ch));
                    *reinterpret_cast<float4*>(a.out2 + orow * Ch + (c - Ch)) = make_float4(h.x * g[0], h.y * g[1], h.z * g[2], h.w * g[3]);
                    if (a.out3) *reinterpret_cast<float4*>(a.out3 + orow * Ch + (c - Ch)) = make_float4(g[0], g[1], g[2], g[3]);
                }
            } else {   // W_GRU_OUT
                const float4 z4 = *reinterpret_cast<const float4*>(a.aux_z + orow * a.Cout + c);
                const float4 h4 = *reinterpret_cast<const float4*>(a.aux_h + orow * a.Cout + c);
                const float zv[4] = {z4.x, z4.y, z4.z, z4.w}, hv[4] = {h4.x, h4.y, h4.z, h4.w};
                float cand[4], hn[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    cand[k] = tanhf(v[k]);
                    hn[k] = hv[k] * (1.f - zv[k]) + cand[k] * zv[k];
                }
                *reinterpret_cast<float4*>(a.out + orow * a.ldo + c) = make_float4(hn[0], hn[1], hn[2], hn[3]);
                if (a.out2)
                    *reinterpret_cast<float4*>(a.out2 + orow * a.ldo + c) =
                        make_float4(fmaf(hn[0], scv[0], shv[0]), fmaf(hn[1], scv[1], shv[1]), fmaf(hn[2], scv[2], shv[2]), fmaf(hn[3], scv[3], shv[3]));
                if (a.out3) *reinterpret_cast<float4*>(a.out3 + orow * a.ldo + c) = make_float4(cand[0], cand[1], cand[2], cand[3]);
            }
        }
}

// The inverse transform of forge_wino_gemm_dn4hw's 36 point products (forge_wino_output_dn4hw): tiles of 4 x 4 voxels, Ht = H / 4, Wt = W / 4, point p = 6 i + j
// (i the H point, j the W point). A^T of F(4, 3) over the H points, per W point j - the four lines of wino_output_kernel<., false, 4> - then THE SAME four lines
// over the six W points of each output row, then the GRU tails. A tile and four channels is split over two threads by output-row pairs: the waves 0, 1 of a
// workgroup run the rows 0, 1 and the waves 2, 3 the rows 2, 3 of the same 128 (tile, channel quad) items, so RH is uniform per wave. A thread loads 30 of the
// 36 planes (rows 0, 1 need no m5, rows 2, 3 no m0; the sibling waves' repeats are L1 hits), keeps 12 row sums and writes 2 x 4 voxels.
template <int EPI, int RH>
__device__ __forceinline__ void wino_output_dn4hw_body(const WinoOutArgs& a, long long idx) {
    const int C4 = a.Cout >> 2, Ht = a.H >> 2, Wt = a.W >> 2;
    unsigned r, t;                                   // t = (n, z) plane index
    int c, tw, th;
    tile_decode(idx, C4, 2, Ht, Wt, r, c, tw, th, t);
    const float* mp = a.Mm + (long long)r * a.Cout + c;
    float4 s[2][6];                                  // rows 2 RH, 2 RH + 1 of A^T m
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float4 m[6];
#pragma unroll
        for (int i = RH; i < 5 + RH; ++i) m[i] = *reinterpret_cast<const float4*>(mp + (6 * i + j) * a.ptm);
        const float4 sl = add(m[1], m[2]), dl = sub(m[1], m[2]), Sl = add(m[3], m[4]), Dl = sub(m[3], m[4]);
        if constexpr (RH == 0) {
            s[0][j] = add(add(sl, Sl), m[0]);
            s[1][j] = fma4(2.f, Dl, dl);
        } else {
            s[0][j] = fma4(4.f, Sl, sl);
            s[1][j] = add(fma4(8.f, Dl, dl), m[5]);
        }
    }
    float4 y[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float4 sl = add(s[i][1], s[i][2]), dl = sub(s[i][1], s[i][2]), Sl = add(s[i][3], s[i][4]), Dl = sub(s[i][3], s[i][4]);
        y[i][0] = add(add(sl, Sl), s[i][0]);
        y[i][1] = fma4(2.f, Dl, dl);
        y[i][2] = fma4(4.f, Sl, sl);
        y[i][3] = add(fma4(8.f, Dl, dl), s[i][5]);
    }
    wino_tail<EPI>(a, y, t, 4 * th + 2 * RH, 4 * tw, c);
}

// Code object (hipcc -O3, gfx950): gates 182 VGPRs, state 196 VGPRs, no scratch = 2 waves per SIMD (wino_output_kernel<., false, 4>: 153 / 168, 2 waves).
template <int EPI>
__global__ __launch_bounds__(256) void wino_output_dn4hw_kernel(const WinoOutArgs a) {
    const long long idx = (long long)blockIdx.x * 128 + (threadIdx.x & 127);
    if (idx >= (long long)a.n * a.D * (a.H >> 2) * (a.W >> 2) * (a.Cout >> 2)) return;
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7)) == 0) wino_output_dn4hw_body<EPI, 0>(a, idx);
    else wino_output_dn4hw_body<EPI, 1>(a, idx);
}

// ---- weight gradient in the Winograd domain: dL/dU[p][kd] = sum_r dMm[p][r] (x) V[p][r + kd plane] (forge_wino_wgrad: conv_wgrad_kernel
// on 16 batched problems), with dMm = A dy A^T the adjoint of the inverse transform, then dL/dw[kd] = G^T dU[kd] G.
struct WinoDyArgs {
    const float* dy; int ldy;                     // upstream gradient rows [n][D][H][W] x ldy floats, Cout channels used
    float* dM; long long ptm;                     // dM[p] = dM + p ptm, rows [n][D][H/2][W/2] x Cout floats
    int n, D, H, W, Cout;
};

// one thread = one 2x2 output tile x 4 channels: 4 float4 loads, A = [1 0; 1 1; 1 -1; 0 -1] on both sides, 16 float4 stores
__global__ __launch_bounds__(256) void wino_dy_kernel(const WinoDyArgs a) {
    const int C4 = a.Cout >> 2, Ht = a.H >> 1, Wt = a.W >> 1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long R = (long long)a.n * a.D * Ht * Wt;
    if (idx >= R * C4) return;
    unsigned r, t;                                   // t = (n, z) plane index
    int c, tw, th;
    tile_decode(idx, C4, 2, Ht, Wt, r, c, tw, th, t);
    const float* yp = a.dy + ((long long)t * a.H * a.W + (long long)(2 * th) * a.W + 2 * tw) * a.ldy + c;
    float4 y[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) y[i][j] = *reinterpret_cast<const float4*>(yp + ((long long)i * a.W + j) * a.ldy);
    a_y_at_store(y[0][0], y[0][1], y[1][0], y[1][1], a.dM + (long long)r * a.Cout + c, a.ptm);
}

// dw[(kd 3 + a) 3 + b][co][ci] += sum_ij G[i][a] G[j][b] dU[4i+j][kd][co][ci]   (G^T dU G): one thread per (kd, co, ci); accumulates into dw
// like forge_conv_wgrad (each element is touched by exactly one thread: deterministic)
__global__ __launch_bounds__(256) void wino_dw_kernel(const float* __restrict__ dU, float* __restrict__ dw, int Cout, int Cin, int KD) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)Cout * Cin;
    if (idx >= KD * per) return;
    const int kd = (int)(idx / per);
    const long long oc = idx - kd * per;
    const long long pt = KD * per;
    float u[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) u[i][j] = dU[(4 * i + j) * pt + kd * per + oc];
    float g[3][4];                                   // G^T u: rows a = 0..2
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g[0][j] = u[0][j] + 0.5f * (u[1][j] + u[2][j]);
        g[1][j] = 0.5f * (u[1][j] - u[2][j]);
        g[2][j] = 0.5f * (u[1][j] + u[2][j]) + u[3][j];
    }
#pragma unroll
    for (int a_ = 0; a_ < 3; ++a_) {                 // (G^T u) G
        float* o = dw + ((long long)((kd * 3 + a_) * 3) * per) + oc;
        o[0 * per] += g[a_][0] + 0.5f * (g[a_][1] + g[a_][2]);
        o[1 * per] += 0.5f * (g[a_][1] - g[a_][2]);
        o[2 * per] += 0.5f * (g[a_][1] + g[a_][2]) + g[a_][3];
    }
}

}  // namespace forge

using namespace forge;

extern "C" int forge_wino_dy(const float* dy, int ldy, float* dM, int n, int D, int H, int W, int Cout, forge_stream_t stream) {
    FORGE_REQUIRE(dy && dM, FORGE_EINVAL, "forge_wino_dy: null pointer argument");
    FORGE_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && Cout > 0 && Cout % 4 == 0 && ldy >= Cout && ldy % 4 == 0, FORGE_ESHAPE,
                  "forge_wino_dy: n=%d D=%d H=%d W=%d Cout=%d ldy=%d (H, W even; Cout, ldy multiples of 4)", n, D, H, W, Cout, ldy);
    WinoDyArgs a;
    const long long R = (long long)n * D * (H / 2) * (W / 2);
    a.dy = dy; a.ldy = ldy; a.dM = dM; a.ptm = R * Cout; a.n = n; a.D = D; a.H = H; a.W = W; a.Cout = Cout;
    FORGE_REQUIRE(R < (1ll << 31), FORGE_ESHAPE, "forge_wino_dy: more than 2^31 tiles; split the batch");
    const long long total = R * (Cout / 4), grid = (total + 255) / 256;
    FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "forge_wino_dy: grid too large");
    hipLaunchKernelGGL(wino_dy_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    FORGE_LAUNCH_CHECK("forge_wino_dy");
    return 0;
}

extern "C" int forge_wino_dw(const float* dU, float* dw, int Cout, int Cin, int kd, forge_stream_t stream) {
    FORGE_REQUIRE(dU && dw && Cout > 0 && Cin > 0 && (kd == 1 || kd == 3), FORGE_EINVAL, "forge_wino_dw: bad argument (kd = 1 or 3)");
    const long long total = (long long)kd * Cout * Cin;
    hipLaunchKernelGGL(wino_dw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dU, dw, Cout, Cin, kd);
    FORGE_LAUNCH_CHECK("forge_wino_dw");
    return 0;
}

// the one launch behind the three weight entries: one thread per element of `total`
template <typename K, typename... A>
static int wino_weights_launch(const char* name, K kernel, long long total, forge_stream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, args...);
    FORGE_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int forge_wino_weights(const float* wp, float* U, int Cout, int Cin, int kd, int transpose, forge_stream_t stream) {
    FORGE_REQUIRE(wp && U && Cout > 0 && Cin > 0 && (kd == 1 || kd == 3), FORGE_EINVAL, "forge_wino_weights: bad argument (kd = 1 or 3)");
    return wino_weights_launch("forge_wino_weights", wino_weight_kernel, (long long)kd * Cout * Cin, stream, wp, U, Cout, Cin, kd, transpose);
}

extern "C" int forge_wino_weights_dn(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream) {
    FORGE_REQUIRE(wp && Ud && Cout > 0 && Cin > 0, FORGE_EINVAL, "forge_wino_weights_dn: bad argument");
    return wino_weights_launch("forge_wino_weights_dn", wino_weight_nest_kernel<4, depth_row_f23>, (long long)Cout * Cin, stream, wp, Ud, Cout, Cin);
}

extern "C" int forge_wino_weights_dn4(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream) {
    FORGE_REQUIRE(wp && Ud && Cout > 0 && Cin > 0, FORGE_EINVAL, "forge_wino_weights_dn4: bad argument");
    return wino_weights_launch("forge_wino_weights_dn4", wino_weight_nest_kernel<6, depth_row_f43>, (long long)Cout * Cin, stream, wp, Ud, Cout, Cin);
}

extern "C" int forge_wino_weights_dn4h(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream) {
    FORGE_REQUIRE(wp && Ud && Cout > 0 && Cin > 0, FORGE_EINVAL, "forge_wino_weights_dn4h: bad argument");
    return wino_weights_launch("forge_wino_weights_dn4h", wino_weight_nest_kernel<6, depth_row_f43, 6, depth_row_f43>, (long long)Cout * Cin, stream, wp, Ud, Cout, Cin);
}

extern "C" int forge_wino_weights_dn4hw(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream) {
    FORGE_REQUIRE(wp && Ud && Cout > 0 && Cin > 0, FORGE_EINVAL, "forge_wino_weights_dn4hw: bad argument");
    return wino_weights_launch("forge_wino_weights_dn4hw", wino_weight_nest_kernel<6, depth_row_f43, 6, depth_row_f43, 6>, (long long)Cout * Cin, stream, wp, Ud, Cout, Cin);
}

// The five input entries. IN_DN4: the depth stage of the F(4, 3) nest in front (wino_input_dn4_kernel: one thread per tile of a GROUP of four planes and channel,
// six operand rows per group tile); IN_DN4H: that with F(4, 3) along H as well (wino_input_dn4_kernel<4>: tiles of 4 x 2 pixels, H % 4 == 0);
// IN_DN4HW: and along W (wino_input_dn4hw_kernel: tiles of 4 x 4 pixels, W % 4 == 0, three waves per 64 tile-channels);
// IN_DY: also dM = A y A^T (wino_input_kernel<true>; dense operands, no view mean).
enum WinoInKind { IN_PLAIN, IN_DN4, IN_DY, IN_DN4H, IN_DN4HW };

static int wino_input_impl(const char* name, WinoInKind kind, const float* in, int ld, long long bs, float* V, int ldv, long long ptv, float* dM, int n, int D, int H,
                           int W, int C, int nsum, long long sum_stride, forge_stream_t stream) {
    const bool h4 = kind == IN_DN4H || kind == IN_DN4HW, dn4 = kind == IN_DN4 || h4;       // six operand rows per tile of a group of four planes
    const int th = h4 ? 4 : 2, tw = kind == IN_DN4HW ? 4 : 2;          // output rows and columns per tile
    FORGE_REQUIRE(in && V && (kind != IN_DY || dM), FORGE_EINVAL, "%s: null pointer argument", name);
    FORGE_REQUIRE(nsum >= 1 && (nsum == 1 || sum_stride > 0), FORGE_EINVAL, "%s: nsum >= 1, and a positive sum_stride (rows) with nsum > 1", name);
    FORGE_REQUIRE(!dn4 || (D > 0 && D % 4 == 0), FORGE_EINVAL, "%s: D=%d must be a multiple of 4", name, D);
    FORGE_REQUIRE(!h4 || (D >= 8 && H > 0 && H % 4 == 0), FORGE_EINVAL, "%s: D=%d H=%d (D >= 8; H a multiple of 4)", name, D, H);
    FORGE_REQUIRE(kind != IN_DN4HW || (W > 0 && W % 4 == 0), FORGE_EINVAL, "%s: W=%d must be a multiple of 4", name, W);
    FORGE_REQUIRE(kind != IN_DN4HW || (long long)D * H * W * ld < (1ll << 31), FORGE_EINVAL, "%s: a batch element of 2^31 floats or more (32-bit offsets inside it)", name);
    const bool ok = n > 0 && D > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0 && ldv >= C && ldv % 4 == 0;
    if (kind == IN_DY)                                // (this entry takes no ldv: its operands are dense)
        FORGE_REQUIRE(ok, FORGE_ESHAPE, "%s: n=%d D=%d H=%d W=%d C=%d ld=%d (H, W even; C, ld multiples of 4)", name, n, D, H, W, C, ld);
    FORGE_REQUIRE(ok, FORGE_ESHAPE, "%s: n=%d D=%d H=%d W=%d C=%d ld=%d ldv=%d (H, W even; C, ld, ldv multiples of 4)", name, n, D, H, W, C, ld, ldv);
    WinoInArgs a;
    a.in = in; a.ld = ld; a.bs = bs > 0 ? bs : (long long)D * H * W; a.V = V; a.ldv = ldv; a.n = n; a.D = D; a.H = H; a.W = W; a.C = C;
    a.nsum = nsum; a.ss = sum_stride;
    const long long R = (long long)n * (dn4 ? D / 4 : D) * (H / th) * (W / tw), rows = dn4 ? 6 * R : R;    // thread tiles; operand rows per point
    a.ptv = ptv > 0 ? ptv : rows * ldv;
    a.dM = dM; a.ptm = dM ? R * C : 0;
    FORGE_REQUIRE(rows < (1ll << 31), FORGE_ESHAPE, dn4 ? "%s: more than 2^31 operand rows; split the batch" : "%s: more than 2^31 tiles; split the batch", name);
    const int per = kind == IN_DN4HW ? 64 : 256;                        // tile-channels per workgroup (IN_DN4HW: three waves each)
    const long long total = R * (dn4 ? C : C / 4), grid = (total + per - 1) / per;
    FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "%s: grid too large", name);
    const dim3 g((unsigned)grid), b(256);
    if (kind == IN_DN4HW && nsum > 1) hipLaunchKernelGGL(wino_input_dn4hw_kernel<true>, g, dim3(192), 0, (hipStream_t)stream, a);
    else if (kind == IN_DN4HW) hipLaunchKernelGGL(wino_input_dn4hw_kernel<false>, g, dim3(192), 0, (hipStream_t)stream, a);
    else if (kind == IN_DN4H) hipLaunchKernelGGL(wino_input_dn4_kernel<4>, g, b, 0, (hipStream_t)stream, a);
    else if (dn4) hipLaunchKernelGGL(wino_input_dn4_kernel<2>, g, b, 0, (hipStream_t)stream, a);
    else if (kind == IN_DY) hipLaunchKernelGGL(wino_input_kernel<true>, g, b, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(wino_input_kernel<false>, g, b, 0, (hipStream_t)stream, a);
    FORGE_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int forge_wino_input(const float* in, int ld, long long bs, float* V, int ldv, long long ptv, int n, int D, int H, int W, int C,
                                int nsum, long long sum_stride, forge_stream_t stream) {
    return wino_input_impl("forge_wino_input", IN_PLAIN, in, ld, bs, V, ldv, ptv, nullptr, n, D, H, W, C, nsum, sum_stride, stream);
}

// forge_wino_input with the depth stage of the F(4, 3) nest (wino_input_dn4_kernel): V6 [16][n][D/4][6][H/2 W/2][C], the operand of forge_wino_gemm_dn4.
// ptv: floats between points (0 = dense, n (D/4) 6 (H/2)(W/2) ldv).
extern "C" int forge_wino_input_dn4(const float* in, int ld, long long bs, float* V6, int ldv, long long ptv, int n, int D, int H, int W, int C,
                                    int nsum, long long sum_stride, forge_stream_t stream) {
    return wino_input_impl("forge_wino_input_dn4", IN_DN4, in, ld, bs, V6, ldv, ptv, nullptr, n, D, H, W, C, nsum, sum_stride, stream);
}

// forge_wino_input_dn4 with F(4, 3) along H as well (wino_input_dn4_kernel<4>): V [24][n][D/4][6][H/4 W/2][C], the operand of forge_wino_gemm_dn4h.
// ptv: floats between points (0 = dense, n (D/4) 6 (H/4)(W/2) ldv). FORGE_EINVAL unless D % 4 == 0, D >= 8 and H % 4 == 0.
extern "C" int forge_wino_input_dn4h(const float* in, int ld, long long bs, float* V, int ldv, long long ptv, int n, int D, int H, int W, int C,
                                     int nsum, long long sum_stride, forge_stream_t stream) {
    return wino_input_impl("forge_wino_input_dn4h", IN_DN4H, in, ld, bs, V, ldv, ptv, nullptr, n, D, H, W, C, nsum, sum_stride, stream);
}

// forge_wino_input_dn4h with F(4, 3) along W as well (wino_input_dn4hw_kernel): V [36][n][D/4][6][H/4 W/4][C], the operand of forge_wino_gemm_dn4hw.
// ptv: floats between points (0 = dense, n (D/4) 6 (H/4)(W/4) ldv). FORGE_EINVAL unless D % 4 == 0, D >= 8, H % 4 == 0 and W % 4 == 0.
extern "C" int forge_wino_input_dn4hw(const float* in, int ld, long long bs, float* V, int ldv, long long ptv, int n, int D, int H, int W, int C,
                                      int nsum, long long sum_stride, forge_stream_t stream) {
    return wino_input_impl("forge_wino_input_dn4hw", IN_DN4HW, in, ld, bs, V, ldv, ptv, nullptr, n, D, H, W, C, nsum, sum_stride, stream);
}

extern "C" int forge_wino_input_dy(const float* dy, int ld, float* V, float* dM, int n, int D, int H, int W, int C, forge_stream_t stream) {
    return wino_input_impl("forge_wino_input_dy", IN_DY, dy, ld, 0, V, C, 0, dM, n, D, H, W, C, 1, 0, stream);
}

static int wino_output_impl(const float* Mm, const float* Mm2, long long bs2, long long pt2, const float* bias, const float* scale, const float* shift, float slope, const float* residual,
                            const float* aux_h, const float* aux_z, float* out, float* out2, float* out3, int n, int D, int H, int W, int Cout,
                            int ldo, int epilogue, bool half, forge_stream_t stream) {
    FORGE_REQUIRE(Mm && out, FORGE_EINVAL, "forge_wino_output: null pointer argument");
    FORGE_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && Cout > 0 && Cout % 8 == 0 && ldo % 4 == 0, FORGE_ESHAPE,
                  "forge_wino_output: n=%d D=%d H=%d W=%d Cout=%d ldo=%d (H, W even; Cout multiple of 8; ldo of 4)", n, D, H, W, Cout, ldo);
    FORGE_REQUIRE(epilogue >= 0 && epilogue <= 3, FORGE_EINVAL, "forge_wino_output: unknown epilogue %d", epilogue);
    // ldo: the row stride of out (and of out2 / out3 of the GRU state epilogue). The gate epilogue writes dense rows of Cout / 2 floats and takes no other.
    FORGE_REQUIRE(epilogue == W_GRU_GATES ? ldo == Cout / 2 : ldo >= Cout, FORGE_ESHAPE,
                  "forge_wino_output: ldo=%d (epilogues 0, 1, 3: ldo >= Cout=%d; epilogue 2: ldo == Cout / 2)", ldo, Cout);
    FORGE_REQUIRE(epilogue != W_AFFINE_ACT || (scale && shift), FORGE_EINVAL, "forge_wino_output: affine epilogue needs scale/shift");
    FORGE_REQUIRE(epilogue != W_GRU_GATES || (aux_h && out2), FORGE_EINVAL, "forge_wino_output: GRU gate epilogue needs aux_h, out2");
    FORGE_REQUIRE(epilogue != W_GRU_OUT || (aux_h && aux_z && (!out2 || (scale && shift))), FORGE_EINVAL,
                  "forge_wino_output: GRU out epilogue needs aux_h, aux_z (and scale/shift with out2)");
    FORGE_REQUIRE(out3 == nullptr || epilogue == W_GRU_GATES || epilogue == W_GRU_OUT, FORGE_EINVAL, "forge_wino_output: out3 is a GRU-epilogue output");
    WinoOutArgs a;
    const long long R = (long long)n * D * (H / 2) * (W / 2);
    a.Mm = Mm; a.ptm = R * Cout; a.Mm2 = Mm2; a.bs2 = bs2 > 0 ? bs2 : (long long)D * (H / 2) * (W / 2); a.ptm2 = pt2 > 0 ? pt2 : R * Cout; a.bias = bias; a.scale = scale; a.shift = shift; a.slope = slope; a.residual = residual; a.aux_h = aux_h; a.aux_z = aux_z;
    a.out = out; a.out2 = out2; a.out3 = out3; a.ldo = ldo; a.n = n; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.epi = epilogue;
    FORGE_REQUIRE(R < (1ll << 31), FORGE_ESHAPE, "forge_wino_output: more than 2^31 tiles; split the batch");
    const long long total = R * (Cout / 4), grid = (total + 255) / 256;
    FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "forge_wino_output: grid too large");
    const dim3 g((unsigned)grid), b(256);
    hipStream_t st = (hipStream_t)stream;
    if (half) {
        switch (epilogue) {
            case W_BIAS: hipLaunchKernelGGL((wino_output_kernel<W_BIAS, true>), g, b, 0, st, a); break;
            case W_AFFINE_ACT: hipLaunchKernelGGL((wino_output_kernel<W_AFFINE_ACT, true>), g, b, 0, st, a); break;
            case W_GRU_GATES: hipLaunchKernelGGL((wino_output_kernel<W_GRU_GATES, true>), g, b, 0, st, a); break;
            default: hipLaunchKernelGGL((wino_output_kernel<W_GRU_OUT, true>), g, b, 0, st, a); break;
        }
    } else {
        switch (epilogue) {
            case W_BIAS: hipLaunchKernelGGL(wino_output_kernel<W_BIAS>, g, b, 0, st, a); break;
            case W_AFFINE_ACT: hipLaunchKernelGGL(wino_output_kernel<W_AFFINE_ACT>, g, b, 0, st, a); break;
            case W_GRU_GATES: hipLaunchKernelGGL(wino_output_kernel<W_GRU_GATES>, g, b, 0, st, a); break;
            default: hipLaunchKernelGGL(wino_output_kernel<W_GRU_OUT>, g, b, 0, st, a); break;
        }
    }
    FORGE_LAUNCH_CHECK("forge_wino_output");
    return 0;
}

extern "C" int forge_wino_output(const float* Mm, const float* Mm2, long long bs2, long long pt2, const float* bias, const float* scale, const float* shift, float slope, const float* residual,
                                 const float* aux_h, const float* aux_z, float* out, float* out2, float* out3, int n, int D, int H, int W, int Cout,
                                 int ldo, int epilogue, forge_stream_t stream) {
    return wino_output_impl(Mm, Mm2, bs2, pt2, bias, scale, shift, slope, residual, aux_h, aux_z, out, out2, out3, n, D, H, W, Cout, ldo, epilogue, false, stream);
}

// The column stage of the inverse transform + the fused tail on forge_wino_gemm_half's 8 planes Mm8 [2][4][R][Cout] (+ a second addend in the same form, as
// forge_wino_output's Mm2): without Mm2_8 bitwise forge_wino_output's result; with it the two operands are row-combined before they are added.
extern "C" int forge_wino_output_half(const float* Mm8, const float* Mm2_8, long long bs2, long long pt2, const float* bias, const float* scale, const float* shift, float slope,
                                      const float* residual, const float* aux_h, const float* aux_z, float* out, float* out2, float* out3, int n, int D, int H, int W,
                                      int Cout, int ldo, int epilogue, forge_stream_t stream) {
    return wino_output_impl(Mm8, Mm2_8, bs2, pt2, bias, scale, shift, slope, residual, aux_h, aux_z, out, out2, out3, n, D, H, W, Cout, ldo, epilogue, true, stream);
}

// The inverse transform of forge_wino_gemm_dn4h's point products Mm [24][n D H/4 W/2][Cout] with the GRU tails of forge_wino_output (epilogue 2: gates, ldo ==
// Cout / 2; 3: state): wino_output_kernel<., false, 4>. The steps of the eval fusion are its only callers: no second addend, no residual, no other epilogue.
extern "C" int forge_wino_output_dn4h(const float* Mm, const float* bias, const float* scale, const float* shift, const float* aux_h, const float* aux_z, float* out,
                                      float* out2, float* out3, int n, int D, int H, int W, int Cout, int ldo, int epilogue, forge_stream_t stream) {
    FORGE_REQUIRE(Mm && out && aux_h, FORGE_EINVAL, "forge_wino_output_dn4h: null pointer argument");
    FORGE_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 2 == 0 && Cout > 0 && Cout % 8 == 0 && ldo % 4 == 0, FORGE_ESHAPE,
                  "forge_wino_output_dn4h: n=%d D=%d H=%d W=%d Cout=%d ldo=%d (H multiple of 4, W even; Cout multiple of 8; ldo of 4)", n, D, H, W, Cout, ldo);
    FORGE_REQUIRE(epilogue == W_GRU_GATES || epilogue == W_GRU_OUT, FORGE_EINVAL, "forge_wino_output_dn4h: epilogue %d is not a GRU tail (2, 3)", epilogue);
    FORGE_REQUIRE(epilogue == W_GRU_GATES ? ldo == Cout / 2 : ldo >= Cout, FORGE_ESHAPE,
                  "forge_wino_output_dn4h: ldo=%d (epilogue 3: ldo >= Cout=%d; epilogue 2: ldo == Cout / 2)", ldo, Cout);
    FORGE_REQUIRE(epilogue != W_GRU_GATES || out2, FORGE_EINVAL, "forge_wino_output_dn4h: GRU gate epilogue needs out2");
    FORGE_REQUIRE(epilogue != W_GRU_OUT || (aux_z && (!out2 || (scale && shift))), FORGE_EINVAL,
                  "forge_wino_output_dn4h: GRU out epilogue needs aux_z (and scale/shift with out2)");
    WinoOutArgs a;
    const long long R = (long long)n * D * (H / 4) * (W / 2);
    a.Mm = Mm; a.ptm = R * Cout; a.Mm2 = nullptr; a.bs2 = 0; a.ptm2 = 0; a.bias = bias; a.scale = scale; a.shift = shift; a.slope = 1.f; a.residual = nullptr;
    a.aux_h = aux_h; a.aux_z = aux_z; a.out = out; a.out2 = out2; a.out3 = out3; a.ldo = ldo; a.n = n; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.epi = epilogue;
    FORGE_REQUIRE(R < (1ll << 31), FORGE_ESHAPE, "forge_wino_output_dn4h: more than 2^31 tiles; split the batch");
    const long long total = R * (Cout / 4), grid = (total + 255) / 256;
    FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "forge_wino_output_dn4h: grid too large");
    const dim3 g((unsigned)grid), b(256);
    if (epilogue == W_GRU_GATES) hipLaunchKernelGGL((wino_output_kernel<W_GRU_GATES, false, 4>), g, b, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((wino_output_kernel<W_GRU_OUT, false, 4>), g, b, 0, (hipStream_t)stream, a);
    FORGE_LAUNCH_CHECK("forge_wino_output_dn4h");
    return 0;
}

// The inverse transform of forge_wino_gemm_dn4hw's point products Mm [36][n D H/4 W/4][Cout] with the GRU tails of forge_wino_output_dn4h (epilogue 2: gates, ldo ==
// Cout / 2; 3: state; no second addend, no residual, as that entry): wino_output_dn4hw_kernel. FORGE_EINVAL unless H % 4 == 0 and W % 4 == 0.
extern "C" int forge_wino_output_dn4hw(const float* Mm, const float* bias, const float* scale, const float* shift, const float* aux_h, const float* aux_z, float* out,
                                       float* out2, float* out3, int n, int D, int H, int W, int Cout, int ldo, int epilogue, forge_stream_t stream) {
    FORGE_REQUIRE(Mm && out && aux_h, FORGE_EINVAL, "forge_wino_output_dn4hw: null pointer argument");
    FORGE_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, FORGE_EINVAL, "forge_wino_output_dn4hw: n=%d D=%d H=%d W=%d (H, W multiples of 4)", n, D, H, W);
    FORGE_REQUIRE(Cout > 0 && Cout % 8 == 0 && ldo % 4 == 0, FORGE_ESHAPE, "forge_wino_output_dn4hw: Cout=%d ldo=%d (Cout multiple of 8; ldo of 4)", Cout, ldo);
    FORGE_REQUIRE(epilogue == W_GRU_GATES || epilogue == W_GRU_OUT, FORGE_EINVAL, "forge_wino_output_dn4hw: epilogue %d is not a GRU tail (2, 3)", epilogue);
    FORGE_REQUIRE(epilogue == W_GRU_GATES ? ldo == Cout / 2 : ldo >= Cout, FORGE_ESHAPE,
                  "forge_wino_output_dn4hw: ldo=%d (epilogue 3: ldo >= Cout=%d; epilogue 2: ldo == Cout / 2)", ldo, Cout);
    FORGE_REQUIRE(epilogue != W_GRU_GATES || out2, FORGE_EINVAL, "forge_wino_output_dn4hw: GRU gate epilogue needs out2");
    FORGE_REQUIRE(epilogue != W_GRU_OUT || (aux_z && (!out2 || (scale && shift))), FORGE_EINVAL,
                  "forge_wino_output_dn4hw: GRU out epilogue needs aux_z (and scale/shift with out2)");
    WinoOutArgs a;
    const long long R = (long long)n * D * (H / 4) * (W / 4);
    a.Mm = Mm; a.ptm = R * Cout; a.Mm2 = nullptr; a.bs2 = 0; a.ptm2 = 0; a.bias = bias; a.scale = scale; a.shift = shift; a.slope = 1.f; a.residual = nullptr;
    a.aux_h = aux_h; a.aux_z = aux_z; a.out = out; a.out2 = out2; a.out3 = out3; a.ldo = ldo; a.n = n; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.epi = epilogue;
    FORGE_REQUIRE(R < (1ll << 31), FORGE_ESHAPE, "forge_wino_output_dn4hw: more than 2^31 tiles; split the batch");
    const long long total = R * (Cout / 4), grid = (total + 127) / 128;              // 128 (tile, channel quad) items per workgroup, two threads each
    FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "forge_wino_output_dn4hw: grid too large");
    const dim3 g((unsigned)grid), b(256);
    if (epilogue == W_GRU_GATES) hipLaunchKernelGGL(wino_output_dn4hw_kernel<W_GRU_GATES>, g, b, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(wino_output_dn4hw_kernel<W_GRU_OUT>, g, b, 0, (hipStream_t)stream, a);
    FORGE_LAUNCH_CHECK("forge_wino_output_dn4hw");
    return 0;
}
