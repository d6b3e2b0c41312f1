// conv_igemm.hip — implicit-GEMM convolution on the gfx950 fp32 matrix cores.
//
// Replaces the dense convolutions of the hot path that the reference runs through cuDNN:
// the ConvGRU fusion (models/fusion.py:29-35, 61-68: 71 % of the hot-path FLOPs), conv1
// (models/encoder.py:36-40) and the heads (models/encoder.py:16-34), with the element-wise tails
// (bias, eval-mode BN, LeakyReLU, GRU sigmoid/tanh/lerp, the cat([x, h])) fused into the GEMM.
//
//   GEMM view:  M = output voxels, N = C_out, K = taps * C_in
//   A[m][k]     = in[voxel(m) + tap offset][ci]      gathered on the fly (zero outside the grid)
//   B[k][n]     = Wp[tap][n][ci]                      weights pre-packed [tap][C_out][C_in]
//
// Arithmetic is exact fp32: v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate; bitwise an fmaf
// chain; 157 TFLOP/s chip peak = 1/16 of bf16) — the reference is fp32 and parity is stated in
// fp32. There is no xf32/TF32 on gfx950.
//
// Tiling: conv_igemm_kernel<BM, BN, NW, MT>: NW waves (8 or 4) arranged WM(M) x WN(N), workgroup
// tile BM x BN x 32(K) (128x128, 64x128, 128x64 with 8 waves; 64x64, 128x32 with 4), wave tile
// (32 MT) x (BN / WN) made of 32x32 MFMA tiles; the tile and a split-K factor are chosen per launch
// by plan_conv(). Both operands are staged as [row][32 k] images in LDS (128-byte rows, 16-byte
// chunks XOR-swizzled with (row>>1)&7 so that the 16-lane groups of ds_read_b128 hit 16 distinct
// slots), filled by LDS-DMA (buffer_load_dwordx4 ... lds: global memory straight into LDS, an
// out-of-range offset lands as zeros — the zero padding of out-of-grid taps / ragged tiles costs
// neither a branch nor a select; round 3, see the kernel's comment and common.h), double-buffered
// with one barrier per K-step and the next K-step's loads in flight under the current MFMAs. The K order inside a 32-chunk is permuted identically for A
// and B: a lane's 16-byte read supplies operand k = 4c+j (lanes 0-31) / 4c+4+j (lanes 32-63) of
// MFMA j.
//
// Round 2: the same kernel also runs the 16 point GEMMs of a Winograd F(2x2, 3x3) x depth-tap convolution in ONE launch (forge_wino_gemm,
// `nbat` problems: workgroup ranges select the point and add a per-point offset to the operand / weight / output pointers; transforms in
// winograd.hip) - the stride-1 3x3x3 convolutions of the fusion, conv1 and the ResNet layer3/4 3x3 convolutions take that route.
#include "common.h"
#include <cmath>
#include <type_traits>

namespace forge {

enum ConvEpilogue : int {
    EPI_BIAS = 0,        // y = acc + bias
    EPI_AFFINE_ACT = 1,  // y = lrelu((acc + bias) * scale + shift, slope)   (eval BN folded; slope 1 = none, 0 = ReLU)
    EPI_GRU_GATES = 2,   // cols [0,Ch): out[m][c] = sigmoid(v) (update z); cols [Ch,2Ch): out2[m][c-Ch] = h * sigmoid(v)
    EPI_GRU_OUT = 3,     // cand = tanh(v); hn = h (1 - z) + cand z; out = hn; out2 (nullable) = hn * scale + shift
};

constexpr int MAX_TAPS = 64;

struct ConvArgs {
    const float* in1; const float* in2;   // channel-concatenated inputs, channels-last; in2 nullable
    int C1, C2, ld1, ld2;                  // channels taken from each input and their row strides (floats)
    long long bs1r, bs2r;                  // batch strides of in1/in2 in rows (voxels)
    long long span1, span2;                // byte spans of in1/in2 (buffer-descriptor bounds, < 2 GiB)
    const float* wp;                       // [ntaps][Cout][C1 + C2]
    const float* bias;                     // [Cout] nullable
    const float* scale; const float* shift; float slope;
    const float* aux_h; const float* aux_z;
    float* out; float* out2; float* out3;   // out3 (nullable): GRU gates -> reset gate r; GRU out -> cand = tanh(v)  (saved for a hand-written backward)
    int n, D, H, W;                        // GEMM-row grid (M = n D H W rows)
    int is, Di, Hi, Wi;                    // input voxel = (z is + dz, y is + dy, x is + dx) in an (n,Di,Hi,Wi) grid
    const float* residual; int ldr;        // EPI_AFFINE_ACT: added before the activation (nullable), [rows][ldr]
    int Cout, ldo;                         // output channels, output row stride (floats)
    int ntaps;
    int os, pz, py, px, Do, Ho, Wo;        // output voxel = (z os + pz, y os + py, x os + px) in an (Do,Ho,Wo) grid
    int nphase, tpp;                       // > 1: all output phases of a stride-2 transposed conv in ONE launch: phase p = (pz,py,px) bits uses taps [p tpp, (p+1) tpp)
    int epi;
    int lift;                              // > 0: 2D->3D lift of the output (models/encoder.py:49), see forge_hip.h
    int nbat;                              // > 1: nbat independent GEMMs in one launch (the 16 Winograd points, forge_wino_gemm): problem p adds
    long long pt1, pt2, ptw, pto;          //      p * pt1 / pt2 / ptw / pto floats to in1 / in2 / wp / out (EPI_BIAS, no split-K, no phases)
    float* ws; int ksplit;                 // split-K: raw partial tiles go to ws[ks][M][Cout], a second kernel reduces + applies the epilogue
    double* stats;                         // EPI_BIAS, nullable: per 32-row block of M the column sums / sums of squares of the OUTPUT, [ceil(M/32)..][2][Cout] float64 -
                                           // the batch statistics of the BatchNorm behind this convolution as a by-product of its epilogue (csrc/bnorm.hip finalizes them)
    int flat_rows;                         // 1: one tap (0,0,0), is == 1, input grid == row grid, dense batch strides: GEMM row m IS input row m (set by launch_conv_tile only)
    int fast_epi;                          // 1: the direct-store epilogue of the convolution body (conv_fast_epilogue_applies, set by launch_conv_tile only)
    signed char tap[MAX_TAPS][4];          // (dz, dy, dx, 0)
};

constexpr int BK = 32, NTHREADS = 512;
constexpr int RS_STAGES = 2;               // LDS stages of the point-GEMM forms (RS): the four-point form's dynamic LDS is RS_STAGES x 24 KB, and three such
                                           // workgroups are resident per CU (at most 80 VGPRs = 6 waves per SIMD; tests/test_conv_igemm_resources.py holds both)

#ifdef FORGE_CONV_TIMING   // debug build (tools/debug/conv_timing.py): per-workgroup clock stamps at entry / first barrier / loop end / exit
__device__ long long g_conv_stamp[8192 * 4];
#define FORGE_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_conv_stamp[blockIdx.x * 4 + (k)] = wall_clock64(); } while (0)
extern "C" int forge_debug_conv_stamps(long long* host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_conv_stamp), (size_t)n * 4 * sizeof(long long));
}
#else
#define FORGE_STAMP(k) do { } while (0)
#endif

__device__ __forceinline__ int lds_off(int row, int chunk) {   // float offset of a 16-byte chunk
    return row * BK + ((chunk ^ ((row >> 1) & 7)) << 2);
}

struct LanePos { int wm, wn, half, l31; };   // wave (wm, wn) of the WM x WN arrangement; half = lane >> 5, l31 = lane & 31

struct ReadA {                                 // the A fragment as staged: one ds_read_b128
    __device__ __forceinline__ float4 operator()(const float* p) const { return *reinterpret_cast<const float4*>(p); }
};

// One K-step = 4 MFMA groups of 8 k-values; read_a(address in the stage's first A image) gives the lane's A fragment. (A/B in round 1: issuing the
// next tile's global loads after group 0 and its LDS writes after group 2, pinned with sched_barrier, changed nothing: 127.3 vs 126.3 TF on the
// ConvGRU gates shape.)
template <int BN, int WN, int MT, int NT, class Read>
__device__ __forceinline__ void mfma_group(const LanePos& lp, f32x16 (&acc)[MT][NT], const float* sa, const float* sb, int g, Read&& read_a) {
    float4 fa[MT], fb[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) fa[i] = read_a(sa + lds_off(lp.wm * (32 * MT) + i * 32 + lp.l31, 2 * g + lp.half));
#pragma unroll
    for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const float4*>(sb + lds_off(lp.wn * (BN / WN) + j * 32 + lp.l31, 2 * g + lp.half));
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
}

// The K loop of the point-GEMM forms (RS): nsteps K-steps into the accumulator set acc over the ring of RS_STAGES LDS stages of STAGE floats (B image
// at B_AT), from stage buf on. issue() moves the form's issue cursor: the NEXT step's loads fly under this step's MFMAs, into the stage read in step
// s - 1 (every wave is past that barrier). The step closes when that stage is in LDS, this wave's part and everybody else's; the forms' plane stores
// are in flight too, hence lds_dma_wait_barrier (common.h).
template <int STAGE, int B_AT, int BN, int WN, class Issue, class Read>
__device__ __forceinline__ void k_loop(const LanePos& lp, f32x16 (&acc)[1][1], const float* smem, int& buf, int nsteps, Issue&& issue, Read&& read_a) {
    for (int s = 0; s < nsteps; ++s) {
        const float* sa = smem + buf * STAGE;
        const float* sb = sa + B_AT;
        issue();
#pragma unroll
        for (int g = 0; g < 4; ++g) mfma_group<BN, WN, 1, 1>(lp, acc, sa, sb, g, read_a);
        lds_dma_wait_barrier();
        buf = buf + 1 == RS_STAGES ? 0 : buf + 1;
    }
}

// Plane store of the point-GEMM forms: the 16 values val(r) of this lane (C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) +
// 4 (lane >> 5)) to the tile's rows of `plane`, row_off bytes further down (identity rows, no bias). Stores go through a buffer descriptor of the
// plane: rows beyond M lie beyond its num_records and columns beyond Cout are sent to OOB - dropped by the hardware, no branch (plane < 2 GiB:
// checked on the host).
struct PlaneStore {
    unsigned ldo4, ovb; int bytes;              // bytes per output row; byte offset of this lane's first element; bytes of a plane
    __device__ __forceinline__ PlaneStore(const ConvArgs& a, long long M, long long m0, int col0, const LanePos& lp) {
        const int ocol = col0 + lp.l31;
        ldo4 = (unsigned)a.ldo * 4u;
        ovb = ocol < a.Cout ? (unsigned)(((int)m0 + lp.wm * 32 + 4 * lp.half) * a.ldo + ocol) * 4u : OOB;
        bytes = (int)(M * a.ldo * 4);
    }
    template <class Val>
    __device__ __forceinline__ void operator()(float* plane, unsigned row_off, Val&& val) const {
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(plane, bytes);
        unsigned vb = ovb + row_off;
        asm volatile("" : "+v"(vb));                             // keeps the 16 row offsets from being computed ahead of the K loops and held in registers
#pragma unroll
        for (int r = 0; r < 16; ++r)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val(r)), rs, (int)(vb + (unsigned)((r & 3) + 8 * (r >> 2)) * ldo4), 0, 0);
    }
};

// Output side of an F(2, 3) over four K loops, A^T = [1 1 1 0; 0 1 -1 -1]: s0 = (m0 + m1) + m2, s1 = (m1 - m2) - m3, wino_output_kernel's own operations
// in its own order (RS = 1: the row stage over the four points; RS = 2: the two planes of the depth nest). Called after K loop q = 0..3, which ran into
// set q (loop 3: set 0); store(i, val) stores output i. s0 is complete after loop 2: its stores fly under loop 3 (they count in vmcnt like the loads:
// the first wait of that loop covers them, a whole K-step later) and loop 3 accumulates into the freed set - three sets live instead of four.
template <class Store>
__device__ __forceinline__ void f23_step(int q, f32x16 (&acc)[3][1][1], Store&& store) {
    if (q == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][0][r] = acc[0][0][0][r] + acc[1][0][0][r];              // t = m0 + m1
    } else if (q == 2) {
        store(0, [&](int r) { return acc[0][0][0][r] + acc[2][0][0][r]; });                            // s0 = t + m2
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[1][0][0][r] = acc[1][0][0][r] - acc[2][0][0][r]; acc[0][0][0][r] = 0.f; }   // u = m1 - m2
    } else if (q == 3) {
        FORGE_STAMP(2);
        store(1, [&](int r) { return acc[1][0][0][r] - acc[0][0][0][r]; });                            // s1 = u - m3
        FORGE_STAMP(3);
    }
}

// Operand staging is LDS-DMA: `buffer_load_dwordx4 ... offen lds` (M0 = the wave's LDS byte address; lane L lands at + 16 L, out-of-range
// lanes write zeros) puts a K-step's A / B rows straight into the other LDS stage - no staging VGPRs, no ds_write. The loads are inline
// assembly because the compiler's own waitcnt insertion would drain them (vmcnt(0)) BEFORE the step's MFMAs (round 2's builtin-based variant
// lost 2-6 % to that); here the loads of step s+1 are issued at the top of step s, fly under its 16 MFMAs per accumulator, and the hand-placed
// `s_waitcnt vmcnt(0)` sits directly in front of the step's closing barrier. Against the register-staged loop this kernel replaced (same K
// order, bitwise the same results): +5..21 % per launch (profiles/TUNING_LOG.md, round 3: 64x128 tile 106 -> 129 TF on the Winograd gates
// GEMM, 128x128 tile 112 -> 135 TF on the K = 6912 direct launch). A third LDS stage (loads two steps ahead) was slower than two: on the
// single-point tiles the extra LDS costs a resident workgroup per CU; on the four-point form (below), where it does not, a three-stage ring with a
// counted vmcnt was still 1-3 % slower than two stages (profiles/TUNING_LOG.md, round 7).
//
// RS = 0: the convolution. RS = 1 / 2 / 3: the three Winograd point-GEMM forms on the 64x128 tile, each described at its branch below; they share the
// tile origin, the staging geometry, prep_tap and issue_step with the convolution, and k_loop, PlaneStore and f23_step (above) among themselves.
template <int BM, int BN, int NW, int MT = 1, int RS = 0>
__global__ __launch_bounds__(NW * 64) void conv_igemm_kernel(const ConvArgs a) {
    constexpr int NP = RS ? 4 : 1;                   // points (RS = 2: depth positions) per workgroup
    constexpr int WM = BM / (32 * MT), WN = NW / WM; // NW waves as WM(M) x WN(N); wave tile (32 MT) x (BN / WN)
    constexpr int NT = BN / (32 * WN);              // 32-col MFMA tiles per wave
    static_assert(NT >= 1 && WM * WN == NW && NT * 32 * WN == BN && WM * 32 * MT == BM, "unsupported tile");
    constexpr int A_FLOATS = BM * BK, B_FLOATS = BN * BK;
    constexpr int RPP = NW * 8;                     // tile rows staged per pass (8 threads per 128-byte row)
    constexpr int ACH = BM / RPP, BCH = BN / RPP;   // 16-byte chunks per thread per K-step
    static_assert(ACH >= 1 && BCH >= 1, "tile too small for the workgroup");
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [2][A_FLOATS + B_FLOATS] (RS: RS_STAGES of them)

    FORGE_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const long long M = (long long)a.n * a.D * a.H * a.W;
    const int ntile_n = (a.Cout + BN - 1) / BN;
    const unsigned bid_all = xcd_remap(blockIdx.x, gridDim.x);
    int ks = 0;                                                   // K-slice of this workgroup (split-K for small M x N problems)
    unsigned bid = bid_all;
    if (!RS && a.ksplit > 1) { ks = (int)(bid_all % (unsigned)a.ksplit); bid = bid_all / (unsigned)a.ksplit; }
    int phase = 0;
    if (a.nphase > 1) {
        // merged transposed-conv phases, phase fastest: the 2^nd output phases of one row tile read the same 3^nd neighbourhood of input rows -
        // dispatched back to back on one XCD (xcd_remap) they share them through its L2 (phase-major, every phase streamed the whole input
        // again: 8 GB of L2->fabric traffic per heads launch of the 4-scene training step, profiles/r04_train_pmc_traffic_b4.txt; 883 -> 867 us)
        phase = (int)(bid % (unsigned)a.nphase);
        bid /= (unsigned)a.nphase;
    }
    const int pz = a.nphase > 1 ? (a.nphase == 8 ? (phase >> 2) & 1 : 0) : a.pz;
    const int py = a.nphase > 1 ? (phase >> 1) & 1 : a.py, px = a.nphase > 1 ? phase & 1 : a.px;
    const int t_lo = phase * a.tpp;
    constexpr int PLANES = RS == 2 ? 2 : RS == 3 ? 4 : 1;          // depth nests: the tiles of every PLANES-th plane only (plane pairs / groups of four)
    long long pb = 0;                                               // batched problems: workgroups [p tiles, (p+1) tiles) do problem p, so that (with
    if (a.nbat > 1) {                                               // xcd_remap's contiguous chunks) an XCD's L2 holds the weights of its own problems only
        const unsigned tiles = (PLANES > 1 ? (unsigned)(M / (PLANES * BM)) : (unsigned)((M + BM - 1) / BM)) * (unsigned)ntile_n;
        pb = bid / tiles;
        bid -= (unsigned)pb * tiles;
    }
    float* const outp = a.out + pb * a.pto;
    const long long m0 = [&]() -> long long {
        if constexpr (PLANES > 1) {                                 // tile ti of every PLANES-th plane: group ti / (HW / BM) = planes PLANES grp .. of the flat
            const unsigned tpl = (unsigned)(a.H * a.W) / BM;       // (n, z) axis (D % PLANES == 0: a group never straddles batch elements)
            const unsigned ti = bid / ntile_n, grp = ti / tpl;
            return (long long)((unsigned)PLANES * grp * tpl + (ti - grp * tpl)) * BM;
        } else {
            return (long long)(bid / ntile_n) * BM;
        }
    }();
    const int n0 = (bid % ntile_n) * BN;
    const int Cin = a.C1 + a.C2;
    const int kchunks = Cin / BK;
    const int nsteps_all = a.tpp * kchunks;
    // K-steps [s_begin, s_end) of slice ks. Without split-K (every launch of the trunk) no division at all, with it 32-bit ones (ksplit <= 8: the products
    // stay far below 2^32): this arithmetic sits in front of the first load of every workgroup, and two 64-bit divisions were some 300 instructions of it
    int s_begin = 0, s_end = nsteps_all;
    if (!RS && a.ksplit > 1) {
        s_begin = (int)((unsigned)ks * (unsigned)nsteps_all / (unsigned)a.ksplit);
        s_end = (int)((unsigned)(ks + 1) * (unsigned)nsteps_all / (unsigned)a.ksplit);
    }
    const int nsteps = s_end - s_begin;

    // RS: pb = the point column j; the workgroup's points are pb, pb + 4, pb + 8, pb + 12 (descriptors re-made at every point switch)
    forge_v4i32 w1 = make_rsrc_words(a.in1 + pb * a.pt1, a.span1), w2 = make_rsrc_words(a.in2 ? a.in2 + pb * a.pt2 : a.in1, a.in2 ? a.span2 : 0),
                ww = make_rsrc_words(a.wp + pb * a.ptw, (long long)a.ntaps * a.Cout * Cin * 4);
    // LDS byte address of this WAVE's first 1 KB block of a stage (lane L lands at + 16 L: the row-major [row][32 k] image, 8 lanes per row)
    const unsigned lds_wave = lds_addr(smem) + (unsigned)__builtin_amdgcn_readfirstlane(wave) * 1024u;
    // ---- per-thread staging geometry: ACH A rows, BCH B rows, one 16-byte chunk each
    const int cp = tid & 7;                                      // physical chunk in the 128-byte LDS row
    int br[BCH]; unsigned boff[BCH];
#pragma unroll
    for (int j = 0; j < BCH; ++j) {
        br[j] = (tid >> 3) + RPP * j;
        const int bsrc = (cp ^ ((br[j] >> 1) & 7)) << 2;
        boff[j] = (n0 + br[j]) < a.Cout ? (unsigned)(((n0 + br[j]) * Cin + bsrc) * 4) : OOB;
    }
    constexpr bool KC_OUTER = (BM == 128 && BN == 128);
    int kc, t;                                                   // K cursor: channel chunk and tap of the next step (orders: see the K loop below)
    if constexpr (KC_OUTER) { kc = s_begin / a.tpp; t = s_begin - kc * a.tpp; }
    else { t = s_begin / kchunks; kc = s_begin - t * kchunks; }
    t += t_lo;
    // LDS-DMA: chunk j of this thread is row (tid >> 3) + RPP j = LDS bytes 16 tid + j NW 1024 -> per wave a lane-linear 1 KB block
    auto issue_b = [&](int t, int kc, int buf) {
        const unsigned stage = lds_wave + (unsigned)buf * (unsigned)((A_FLOATS + B_FLOATS) * 4);
        const unsigned wbase = (unsigned)((t * a.Cout * Cin + kc * BK) * 4);
#pragma unroll
        for (int j = 0; j < BCH; ++j) lds_dma16(ww, boff[j] + wbase, stage + (unsigned)(A_FLOATS * 4 + j * NW * 1024));
    };
    // The convolution's first weight stage needs n0 and tid only: it is issued here, ahead of the A-row decode (three divisions per row), and flies under it
    if constexpr (!RS) issue_b(t, kc, 0);
    const bool flat = !RS && a.flat_rows;                        // workgroup-uniform: GEMM row m is input row m (the point forms never are: their rows are tiles)
    const int Wi_ = flat ? (int)M : a.Wi;                        // input width the taps are tested against
    int ar[ACH], az[ACH], ay[ACH], ax[ACH], an[ACH], asrc[ACH];
    bool aval[ACH];
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
        ar[j] = (tid >> 3) + RPP * j;
        const long long vl = m0 + ar[j];
        aval[j] = vl < M;
        unsigned v = aval[j] ? (unsigned)vl : 0u;                // M < 2^31 (checked on the host): 32-bit divisions (64-bit ones are ~100 instructions each)
        if (flat) {                                              // workgroup-uniform (the 1x1 convolutions of the trunk): row m of the GEMM is row m of the input -
            ax[j] = (int)v; ay[j] = az[j] = an[j] = 0;            // decoded as x = m on a 1 x 1 x M grid (Wi_ below), the same offsets without a division
        } else {
            unsigned q = v / (unsigned)a.W;
            ax[j] = (int)(v - q * (unsigned)a.W) * a.is; v = q;
            q = v / (unsigned)a.H;
            ay[j] = (int)(v - q * (unsigned)a.H) * a.is; v = q;
            q = v / (unsigned)a.D;
            az[j] = (int)(v - q * (unsigned)a.D) * a.is;
            an[j] = (int)q;
        }
        asrc[j] = (cp ^ ((ar[j] >> 1) & 7)) << 2;                // logical channel offset inside the 32-chunk
    }

    // 128x128 tile (tap-inner K order, below): switching taps every K-step must be cheap. Per A row: bit t of vmask = tap t lands
    // inside the input grid; the input row of tap t is base + delta(t) with the uniform delta(t) = (dz Hi + dy) Wi + dx (LDS table),
    // so a tap switch costs a shift, a test and an add per row. The other tiles switch taps once per Cin / 32 K-steps and compute it directly.
    static_assert(!RS || (!KC_OUTER && MT == 1), "the row-stage form exists on the tap-outer tiles");
    __shared__ int sdelta[KC_OUTER ? 2 * MAX_TAPS : 1];             // byte deltas of the taps for in1 / in2
    unsigned long long vmask[KC_OUTER ? ACH : 1];
    unsigned base1[KC_OUTER ? ACH : 1], base2[KC_OUTER ? ACH : 1];  // byte offset of (row of tap (0,0,0), this thread's 16-byte chunk) in in1 / in2
    if constexpr (KC_OUTER) {
#pragma unroll
        for (int j = 0; j < ACH; ++j) {
            const int sp = (az[j] * a.Hi + ay[j]) * a.Wi + ax[j];
            base1[j] = (unsigned)(((an[j] * (int)a.bs1r + sp) * a.ld1 + asrc[j]) * 4);
            base2[j] = (unsigned)(((an[j] * (int)a.bs2r + sp) * a.ld2 + asrc[j]) * 4);
            vmask[j] = 0ull;
        }
        for (int tt = 0; tt < a.ntaps; ++tt) {
            const int dz = a.tap[tt][0], dy = a.tap[tt][1], dx = a.tap[tt][2];
#pragma unroll
            for (int j = 0; j < ACH; ++j) {
                const int zi = az[j] + dz, yi = ay[j] + dy, xi = ax[j] + dx;
                const bool ok = aval[j] && (unsigned)zi < (unsigned)a.Di && (unsigned)yi < (unsigned)a.Hi && (unsigned)xi < (unsigned)Wi_;
                vmask[j] |= (unsigned long long)ok << tt;
            }
        }
        if (tid < a.ntaps) {
            const int d = (a.tap[tid][0] * a.Hi + a.tap[tid][1]) * a.Wi + a.tap[tid][2];
            sdelta[tid] = d * a.ld1 * 4;
            sdelta[MAX_TAPS + tid] = d * a.ld2 * 4;
        }
        __syncthreads();
    }
    // Byte offset of each A row's chunk for the current tap, OOB (>= 2^31) when the tap falls outside the grid: a K-step's load address is then
    // ONE add (offset + 4 c0) per chunk - no multiply, no select (OOB + anything < 2^31 stays out of the buffer's range and reads 0).
    unsigned eoff[ACH], eoff2[ACH];
    auto prep_tap = [&](int t) {
        if constexpr (KC_OUTER) {
            const unsigned d1 = (unsigned)sdelta[t], d2 = (unsigned)sdelta[MAX_TAPS + t];
#pragma unroll
            for (int j = 0; j < ACH; ++j) {
                const bool ok = (vmask[j] >> t) & 1ull;
                eoff[j] = ok ? base1[j] + d1 : OOB;
                eoff2[j] = ok ? base2[j] + d2 : OOB;
            }
        } else {
            const int dz = a.tap[t][0], dy = a.tap[t][1], dx = a.tap[t][2];
#pragma unroll
            for (int j = 0; j < ACH; ++j) {
                const int zi = az[j] + dz, yi = ay[j] + dy, xi = ax[j] + dx;
                const bool ok = aval[j] && (unsigned)zi < (unsigned)a.Di && (unsigned)yi < (unsigned)a.Hi && (unsigned)xi < (unsigned)Wi_;
                const int sp = (zi * a.Hi + yi) * a.Wi + xi;
                eoff[j] = ok ? (unsigned)(((an[j] * (int)a.bs1r + sp) * a.ld1 + asrc[j]) * 4) : OOB;
                eoff2[j] = ok ? (unsigned)(((an[j] * (int)a.bs2r + sp) * a.ld2 + asrc[j]) * 4) : OOB;
            }
        }
    };
    auto issue_a = [&](int t, int kc, int buf) {
        const int c0 = kc * BK;
        const unsigned stage = lds_wave + (unsigned)buf * (unsigned)((A_FLOATS + B_FLOATS) * 4);
        if (c0 < a.C1) {
#pragma unroll
            for (int j = 0; j < ACH; ++j) lds_dma16(w1, eoff[j] + (unsigned)(c0 * 4), stage + (unsigned)(j * NW * 1024));
        } else {
#pragma unroll
            for (int j = 0; j < ACH; ++j) lds_dma16(w2, eoff2[j] + (unsigned)((c0 - a.C1) * 4), stage + (unsigned)(j * NW * 1024));
        }
    };
    auto issue_step = [&](int t, int kc, int buf) { issue_a(t, kc, buf); issue_b(t, kc, buf); };
    constexpr int NACC = RS == 3 ? 4 : RS ? 3 : 1;                 // accumulator sets (RS = 1, 2: the row stage frees one after point 2; RS = 3: s, d, m3, m4)
    f32x16 accs[NACC][MT][NT];
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) accs[q][i][j][r] = 0.f;
    f32x16 (&acc)[MT][NT] = accs[0];                                // the single-point form's accumulators (epilogues below)

    const int half = lane >> 5, l31 = lane & 31;
    // K order of the 128x128 tile: channel chunk OUTER, tap INNER. All workgroups of an XCD walk the taps of one 32-channel slice of
    // their rows before moving to the next slice, so the slice (128 B per row, ~0.7 MB per XCD with its halo) stays in the 4 MiB L2
    // across the 27 taps; with the tap outer the per-tap working set is the full 1 KB rows = the whole L2 and every tap re-fetches them
    // from the fabric (ConvGRU gates launch: 502 -> 132 MB of L2 fills per launch, FETCH_SIZE). The 64-row tiles keep the tap outer:
    // they measured 3-4 % slower with the chunk outer (tools/conv_ab.py).
    auto advance = [&]() {
        if constexpr (KC_OUTER) {
            if (++t == t_lo + a.tpp) { t = t_lo; ++kc; }
            prep_tap(t);
        } else {
            if (++kc == kchunks) { kc = 0; ++t; prep_tap(t); }
        }
    };
    if constexpr (!RS) {
        prep_tap(t);
        issue_a(t, kc, 0);                                          // (the weight half of stage 0 is already in flight)
        lds_dma_wait();
        __syncthreads();
        FORGE_STAMP(1);
    }
    const LanePos lp{wm, wn, half, l31};
    [[maybe_unused]] const unsigned HW = (unsigned)(a.H * a.W);   // the forms: rows of a plane; first output column of this wave
    [[maybe_unused]] const int col0 = n0 + wn * (BN / WN);
    if constexpr (!RS) {
    int buf = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        for (int s = 0; s < nsteps; ++s) {
            const float* sa = smem + buf * (A_FLOATS + B_FLOATS);
            const float* sb = sa + A_FLOATS;
            if (s + 1 < nsteps) {                                 // the other stage was last read in step s - 1: every wave is past that barrier
                advance();
                issue_step(t, kc, buf ^ 1);                       // in flight under this step's MFMAs
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) mfma_group<BN, WN, MT, NT>(lp, accs[q], sa, sb, g, ReadA{});
            lds_dma_wait();                                       // this wave's part of the next step is in LDS ...
            __syncthreads();                                      // ... and so is everybody else's
            buf ^= 1;
        }
    }
    } else if constexpr (RS == 1) {
        // RS = 1 (forge_wino_gemm_half, 64x128 tile): one workgroup runs the FOUR Winograd points i = 0..3 of a point column j on its tile, one K loop after
        // the other (the first stage of the next point is loaded under the last step of the current one), and applies the ROW stage of the inverse
        // transform A^T M A in registers - the same lane holds element (row, col) of all four points: s0 = (m0 + m1) + m2, s1 = (m1 - m2) - m3,
        // wino_output_kernel's own operations in its own order - and stores 2 planes instead of 4: Mm8 [2][4][R][Cout]. The point products then cross HBM
        // as 2x instead of 4x the output tensor, written here and read by the inverse transform. s0 is stored as soon as point 2 is done, under point 3's
        // K loop, so three accumulator sets are live, not four: at most 80 VGPRs = 6 waves per SIMD = THREE resident workgroups per CU (3 x 48 KB of LDS;
        // with four sets and 96 VGPRs it was two - 512 slots chip-wide, not the 640 an earlier note assumed).
        // Four points, one K loop after the other. An issue cursor (point iq, tap it, chunk ikc) runs one step ahead of the MFMAs and walks straight
        // over the point switches (descriptors re-made there): the next point's first stage flies under the current point's last step.
        // Depth taps that are zero for the WHOLE tile are not walked: when all valid rows of the tile lie in one depth plane z and z + dz is
        // outside the grid, that tap's Cin / 32 K-steps multiply DMA'd zeros. Workgroup-uniform. Bitwise neutral for finite weights: an
        // accumulator that starts at +0 never becomes -0, and x + (+-0) = x. Only leading / trailing taps are trimmed (the K order stays).
        static_assert(NT == 1, "the row stage is written for one 32-column MFMA tile per wave");
        int t_first = 0, t_end = a.tpp;
        const long long mlast = (m0 + BM < M ? m0 + BM : M) - 1;
        const unsigned p0 = (unsigned)m0 / HW, p1 = (unsigned)mlast / HW;
        if (p0 == p1) {
            const int z = (int)(p0 % (unsigned)a.D) * a.is;
            while (t_first < t_end - 1 && (unsigned)(z + a.tap[t_first][0]) >= (unsigned)a.Di) ++t_first;
            while (t_end - 1 > t_first && (unsigned)(z + a.tap[t_end - 1][0]) >= (unsigned)a.Di) --t_end;
        }
        const int nst = (t_end - t_first) * kchunks;               // K-steps per point
        int iq = 0, it = t_first, ikc = 0, ibuf = 0;
        auto issue_next = [&]() {
            if (iq >= NP) return;
            issue_step(it, ikc, ibuf);
            ibuf = ibuf + 1 == RS_STAGES ? 0 : ibuf + 1;
            if (++ikc == kchunks) {
                ikc = 0;
                if (++it == t_end) {
                    it = t_first;
                    if (++iq < NP) {                                // pb = the point column j; the workgroup's points are pb, pb + 4, pb + 8, pb + 12
                        const long long pn = pb + 4 * iq;
                        w1 = make_rsrc_words(a.in1 + pn * a.pt1, a.span1);
                        w2 = make_rsrc_words(a.in2 ? a.in2 + pn * a.pt2 : a.in1, a.in2 ? a.span2 : 0);
                        ww = make_rsrc_words(a.wp + pn * a.ptw, (long long)a.ntaps * a.Cout * Cin * 4);
                    }
                }
                if (iq < NP) prep_tap(it);
            }
        };
        prep_tap(t_first);
        issue_next();
        lds_dma_wait_barrier();
        FORGE_STAMP(1);
        const PlaneStore store_plane(a, M, m0, col0, lp);
        int buf = 0;
        auto store = [&](int i, auto&& val) { store_plane(a.out + (pb + 4 * i) * a.pto, 0u, val); };       // plane i of point column pb
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            k_loop<A_FLOATS + B_FLOATS, A_FLOATS, BN, WN>(lp, accs[q == 3 ? 0 : q], smem, buf, nst, issue_next, ReadA{});
            f23_step(q, accs, store);
        }
    } else if constexpr (RS == 2) {
        // RS = 2 (forge_wino_gemm_dn, 64x128 tile): the depth nest. A Winograd F(2, 3) over the three DEPTH taps on top of the 2-D points: a workgroup owns 64
        // tile rows of an EVEN plane z for one point p and runs four K loops k = 0..3 of K = Cin each (instead of 2 planes x 3 taps = six) on the operands
        //   k = 0: V[z-1] - V[z+1]   k = 1: V[z] + V[z+1]   k = 2: V[z+1] - V[z]   k = 3: V[z] - V[z+2]      (the rows of B^T; planes outside the grid are zero)
        // against U'[p][k] (forge_wino_weights_dn). Both planes of a position are staged as two A images by LDS-DMA (an out-of-grid plane at the out-of-range
        // offset) and combined with one fp32 operation per element on the ds_read_b128 results, in front of the MFMAs. The output side is A^T = [1 1 1 0; 0 1 -1 -1]
        // over the four positions - the four-point form's own skeleton: y_z = (m0 + m1) + m2 stored under k = 3's loop, y_{z+1} = (m1 - m2) - m3 - and the result
        // is the ordinary 16-plane Mm [16][R][Cout] of forge_wino_gemm. 2 x 32 KB of LDS: two workgroups per CU (resources: the remark above forge_wino_gemm_dn).
        // All 64 rows of the tile lie in plane (n, z), z even; the host has checked H W % 64 == 0, D even, M H W ldo 4 < 2^31.
        constexpr int STAGE = 2 * A_FLOATS + B_FLOATS;             // [A image of plane a_k][A image of plane b_k][B]
        static_assert(ACH == 1 && NT == 1, "the depth nest is written for the 64 x 128 tile of 8 waves");
        const int z = (int)(((unsigned)m0 / HW) % (unsigned)a.D);  // workgroup-uniform
        const int sp0 = (az[0] * a.Hi + ay[0]) * a.Wi + ax[0];
        const unsigned base1 = (unsigned)(((an[0] * (int)a.bs1r + sp0) * a.ld1 + asrc[0]) * 4), base2 = (unsigned)(((an[0] * (int)a.bs2r + sp0) * a.ld2 + asrc[0]) * 4);
        const int ps1 = (int)HW * a.ld1 * 4, ps2 = (int)HW * a.ld2 * 4;   // bytes from a plane to the next in V1 / V2
        unsigned ea1, eb1, ea2, eb2;                               // this thread's chunk in planes z + dza / z + dzb of V1 / V2, OOB outside the grid
        auto prep_pos = [&](int k) {
            const int dza = k == 0 ? -1 : k == 2 ? 1 : 0, dzb = k == 2 ? 0 : k == 3 ? 2 : 1;
            const bool oka = (unsigned)(z + dza) < (unsigned)a.D, okb = (unsigned)(z + dzb) < (unsigned)a.D;
            ea1 = oka ? base1 + (unsigned)(dza * ps1) : OOB; ea2 = oka ? base2 + (unsigned)(dza * ps2) : OOB;
            eb1 = okb ? base1 + (unsigned)(dzb * ps1) : OOB; eb2 = okb ? base2 + (unsigned)(dzb * ps2) : OOB;
        };
        int ik = 0, ikc = 0, ibuf = 0;
        auto issue_next = [&]() {                                  // the issue cursor runs one step ahead of the MFMAs, straight over the position switches
            if (ik >= NP) return;
            const int c0 = ikc * BK;
            const unsigned stage = lds_wave + (unsigned)ibuf * (unsigned)(STAGE * 4);
            if (c0 < a.C1) {
                lds_dma16(w1, ea1 + (unsigned)(c0 * 4), stage);
                lds_dma16(w1, eb1 + (unsigned)(c0 * 4), stage + (unsigned)(A_FLOATS * 4));
            } else {
                lds_dma16(w2, ea2 + (unsigned)((c0 - a.C1) * 4), stage);
                lds_dma16(w2, eb2 + (unsigned)((c0 - a.C1) * 4), stage + (unsigned)(A_FLOATS * 4));
            }
            const unsigned wbase = (unsigned)((ik * a.Cout * Cin + c0) * 4);
#pragma unroll
            for (int j = 0; j < BCH; ++j) lds_dma16(ww, boff[j] + wbase, stage + (unsigned)(2 * A_FLOATS * 4 + j * NW * 1024));
            ibuf = ibuf + 1 == RS_STAGES ? 0 : ibuf + 1;
            if (++ikc == kchunks) {
                ikc = 0;
                if (++ik < NP) prep_pos(ik);
            }
        };
        prep_pos(0);
        issue_next();
        lds_dma_wait_barrier();
        FORGE_STAMP(1);
        const PlaneStore store_plane(a, M, m0, col0, lp);
        int buf = 0;
        auto store = [&](int i, auto&& val) { store_plane(outp, (unsigned)i * HW * store_plane.ldo4, val); };   // the tile's rows of plane z + i: the first plane's plus H W
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const float sgn = q == 1 ? 1.f : -1.f;                 // a_k + b_k at k = 1, a_k - b_k elsewhere: fmaf(+-1, b, a) is that one rounded add / sub
            k_loop<STAGE, 2 * A_FLOATS, BN, WN>(lp, accs[q == 3 ? 0 : q], smem, buf, kchunks, issue_next, [sgn](const float* p) {
                const float4 pa = *reinterpret_cast<const float4*>(p), pq = *reinterpret_cast<const float4*>(p + A_FLOATS);
                return make_float4(fmaf(sgn, pq.x, pa.x), fmaf(sgn, pq.y, pa.y), fmaf(sgn, pq.z, pa.z), fmaf(sgn, pq.w, pa.w));
            });
            f23_step(q, accs, store);
        }
    } else {
        // RS = 3 (forge_wino_gemm_dn4, 64x128 tile): the depth nest with F(4, 3). A workgroup owns 64 tile rows of a GROUP of four planes 4g .. 4g + 3 for one point and
        // runs six K loops of K = Cin (1.5 per plane) on the depth-combined operand planes V6[.][g][k] that forge_wino_input_dn4 wrote - ONE A image per K-step, the
        // inner loop of RS = 1, no VALU in front of the MFMAs - against U''[p][k] (forge_wino_weights_dn4). The output side is A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0;
        // 0 1 1 4 4 0; 0 1 -1 8 -8 1] over the six positions, all scalings powers of two: loops 1, 2 -> s = m1 + m2, d = m1 - m2; loops 3, 4 -> S = m3 + m4,
        // D = m3 - m4; y1 = d + 2 D and y2 = s + 4 S are stored under the next loop; loop 0 accumulates onto s + S (y0, stored under loop 5), loop 5 onto d + 8 D (y3).
        // Four accumulator sets live; 2 x 24 KB of LDS (resources: the remark above forge_wino_gemm_dn4).
        // The tile's 64 rows lie in plane (n, 4 g) of the output; the host has checked H W % 64 == 0, D % 4 == 0 and that operands and an output plane
        // stay below 2 GiB. The operand of position k is plane 6 g + k of the element's V6 block: one A image per K-step.
        constexpr int NPOS = 6;
        static_assert(ACH == 1 && NT == 1, "the depth nest is written for the 64 x 128 tile of 8 waves");
        const unsigned plane0 = (unsigned)m0 / HW;                 // n D + 4 g, workgroup-uniform
        const unsigned nb = plane0 / (unsigned)a.D, g4 = plane0 - nb * (unsigned)a.D;      // g4 = 4 g
        const unsigned rin = (unsigned)m0 - plane0 * HW + (unsigned)ar[0];                 // this thread's row inside the plane
        const unsigned row6 = (g4 + (g4 >> 1)) * HW + rin;         // row of position 0 in the element's [D/4][6][H W] block
        const unsigned base1 = (unsigned)((((int)nb * (int)a.bs1r + (int)row6) * a.ld1 + asrc[0]) * 4);
        const unsigned base2 = (unsigned)((((int)nb * (int)a.bs2r + (int)row6) * a.ld2 + asrc[0]) * 4);
        const unsigned ps1 = HW * (unsigned)a.ld1 * 4u, ps2 = HW * (unsigned)a.ld2 * 4u;   // bytes from a position to the next in V1 / V2
        // K loops in the order of the output schedule: positions 1, 2 | 3, 4 | 0 | 5
        auto pos_of = [](int iq) { return iq < 4 ? iq + 1 : iq == 4 ? 0 : 5; };
        int iq = 0, ikc = 0, ibuf = 0, ipos = 1;
        eoff[0] = base1 + ps1; eoff2[0] = base2 + ps2;
        auto issue_next = [&]() {                                  // the issue cursor runs one step ahead of the MFMAs, straight over the position switches
            if (iq >= NPOS) return;
            issue_step(ipos, ikc, ibuf);
            ibuf = ibuf + 1 == RS_STAGES ? 0 : ibuf + 1;
            if (++ikc == kchunks) {
                ikc = 0;
                if (++iq < NPOS) {
                    ipos = pos_of(iq);
                    eoff[0] = base1 + (unsigned)ipos * ps1; eoff2[0] = base2 + (unsigned)ipos * ps2;
                }
            }
        };
        issue_next();
        lds_dma_wait_barrier();
        FORGE_STAMP(1);
        const PlaneStore store_plane(a, M, m0, col0, lp);
        auto store = [&](int i, const f32x16& y) { store_plane(outp, (unsigned)i * HW * store_plane.ldo4, [&](int r) { return y[r]; }); };   // the tile's rows of plane 4 g + i
        int buf = 0;
#pragma unroll
        for (int q = 0; q < NPOS; ++q) {                           // m1, m2, m3, m4 into sets 0..3; position 0 onto set 0 (s + S), position 5 onto set 1 (d + 8 D)
            k_loop<A_FLOATS + B_FLOATS, A_FLOATS, BN, WN>(lp, accs[q < 4 ? q : q - 4], smem, buf, kchunks, issue_next, ReadA{});
            if (q == 1) {                                          // s = m1 + m2, d = m1 - m2
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float m1 = accs[0][0][0][r], m2 = accs[1][0][0][r];
                    accs[0][0][0][r] = m1 + m2; accs[1][0][0][r] = m1 - m2;
                }
            } else if (q == 3) {                                   // S = m3 + m4, D = m3 - m4: y1 = d + 2 D, y2 = s + 4 S stored under position 0's loop
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float S = accs[2][0][0][r] + accs[3][0][0][r], Dl = accs[2][0][0][r] - accs[3][0][0][r];
                    accs[2][0][0][r] = fmaf(4.f, S, accs[0][0][0][r]);     // y2
                    accs[3][0][0][r] = fmaf(2.f, Dl, accs[1][0][0][r]);    // y1
                    accs[0][0][0][r] = accs[0][0][0][r] + S;               // s + S: position 0 accumulates onto it
                    accs[1][0][0][r] = fmaf(8.f, Dl, accs[1][0][0][r]);    // d + 8 D: position 5 accumulates onto it
                }
                store(1, accs[3][0][0]);
                store(2, accs[2][0][0]);
            } else if (q == 4) {
                store(0, accs[0][0][0]);                           // y0 = (s + S) + m0, in flight under position 5's loop
            }
        }
        FORGE_STAMP(2);
        store(3, accs[1][0][0]);                                   // y3 = (d + 8 D) + m5
        FORGE_STAMP(3);
    }
    if constexpr (RS != 0) return;

    FORGE_STAMP(2);
    // ---- epilogue: C/D layout of 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    // Direct-store epilogue (a.fast_epi, workgroup-uniform, chosen on the host by conv_fast_epilogue_applies: identity output rows, EPI_BIAS / EPI_AFFINE_ACT,
    // no split-K, lift or statistics): what PlaneStore does for the point forms. Stores go through a buffer descriptor of exactly the bytes
    // ((M - 1) ldo + Cout) 4 that the launch may write, with one 32-bit byte offset per lane: rows beyond M lie beyond num_records (ldo >= Cout), columns
    // beyond Cout start at OOB and stay in [2^31, 2^32) (ldo < 2^22: a tile's last row is at most 127 rows below) - dropped by the hardware. No row table in
    // LDS, no barrier after the K loop, no 64-bit address and no branch per element. The residual is read through a descriptor of its own, all 16 MT NT
    // loads of the wave ahead of its first store: each lane reads exactly the elements it writes, so an in-place residual (residual == out, ldr == ldo:
    // the one legal overlap) sees its own values. Every launch that reaches this epilogue today has ldr == ldo (forge_conv_igemm reads the residual at the
    // output's stride unless there is a lift or a GRU epilogue, which keep the row table); ldr stays a stride of its own here as in the row-table epilogue.
    // Batched problems (nbat > 1, the point GEMMs) come here with EPI_BIAS only (launch_conv_tile): the residual carries no per-problem offset.
    // The arithmetic per element is the general epilogue's, operation for operation: the stored bits are the same.
    if (a.fast_epi) {
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(outp, ((M - 1) * a.ldo + a.Cout) * 4);
        const unsigned row0 = (unsigned)m0 + (unsigned)(wm * (32 * MT) + 4 * half);        // this lane's first row; element (i, r) is (i 32 + (r & 3) + 8 (r >> 2)) rows below
        const unsigned ldo4 = (unsigned)a.ldo * 4u;
        auto direct = [&](auto EPI_TAG, auto RES_TAG) {
            constexpr int EPI = decltype(EPI_TAG)::value;
            constexpr bool RES = decltype(RES_TAG)::value;
            float res[RES ? NT : 1][MT][16];
            if constexpr (RES) {
                const __amdgpu_buffer_rsrc_t rr = make_rsrc(a.residual, ((M - 1) * a.ldr + a.Cout) * 4);
                const unsigned ldr4 = (unsigned)a.ldr * 4u;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int col = col0 + j * 32 + l31;
                    const unsigned rb = col < a.Cout ? (row0 * (unsigned)a.ldr + (unsigned)col) * 4u : OOB;
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            res[j][i][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, (int)(rb + (unsigned)(i * 32 + (r & 3) + 8 * (r >> 2)) * ldr4), 0, 0));
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = col0 + j * 32 + l31;
                const bool cok = col < a.Cout;
                const int colc = cok ? col : 0;
                const float bias = a.bias ? a.bias[colc] : 0.f;
                float sc = 1.f, sh = 0.f;
                if (EPI == EPI_AFFINE_ACT && a.scale) { sc = a.scale[colc]; sh = a.shift[colc]; }
                const unsigned vb = cok ? (row0 * (unsigned)a.ldo + (unsigned)col) * 4u : OOB;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[i][j][r] + bias;
                        if constexpr (EPI == EPI_AFFINE_ACT) {
                            v = fmaf(v, sc, sh);
                            if constexpr (RES) v += res[j][i][r];
                            v = v > 0.f ? v : v * a.slope;
                        }
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, (int)(vb + (unsigned)(i * 32 + (r & 3) + 8 * (r >> 2)) * ldo4), 0, 0);
                    }
            }
        };
        if (a.epi == EPI_BIAS) direct(std::integral_constant<int, EPI_BIAS>{}, std::false_type{});
        else if (a.residual) direct(std::integral_constant<int, EPI_AFFINE_ACT>{}, std::true_type{});
        else direct(std::integral_constant<int, EPI_AFFINE_ACT>{}, std::false_type{});
        FORGE_STAMP(3);
        return;
    }
    // The output-row mapping (identity, strided / phase remap of a transposed convolution, or the 2D->3D lift) is computed ONCE per
    // tile row by one thread (32-bit divisions) into an LDS table; the fully unrolled per-accumulator code below (the accumulators
    // must stay in registers) then holds no division and no remap branch. (Round 1 inlined three 64-bit divisions per accumulator
    // element: 45-90 k instructions per instantiation, far beyond the instruction cache, which cost every workgroup a chain of
    // instruction-fetch misses - the reason 2 us of MFMA work took 20 us per launch in the ResNet trunk.)
    const int Ch = a.Cout / 2;
    const bool remap = (a.os != 1) || (a.Do != a.D) || (a.Ho != a.H) || (a.Wo != a.W);
    long long* s_row = reinterpret_cast<long long*>(smem);          // [BM] output row (or lifted base offset) of each tile row, -1 = beyond M
    if (a.ksplit == 1 && tid < BM) {
        const long long m = m0 + tid;
        long long o = -1;
        if (m < M) {
            if (a.lift > 0) {                                        // row (n, hw) -> base of out[n][0][hw][0] in the [n][lift][HW][Cl] volume
                const unsigned HW = (unsigned)(a.H * a.W), nn = (unsigned)m / HW, hw = (unsigned)m - nn * HW;
                o = ((long long)nn * a.lift * HW + hw) * (a.Cout / a.lift);
            } else if (remap) {
                unsigned q = (unsigned)m, t2 = q / (unsigned)a.W;
                const int x = (int)(q - t2 * (unsigned)a.W); q = t2; t2 = q / (unsigned)a.H;
                const int y = (int)(q - t2 * (unsigned)a.H); q = t2; t2 = q / (unsigned)a.D;
                const int z = (int)(q - t2 * (unsigned)a.D);
                o = (((long long)t2 * a.Do + (z * a.os + pz)) * a.Ho + (y * a.os + py)) * a.Wo + (x * a.os + px);
            } else {
                o = m;
            }
        }
        s_row[tid] = o;
    }
    __syncthreads();
    auto epilogue = [&](auto EPI_TAG) {
        constexpr int EPI = decltype(EPI_TAG)::value;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = n0 + wn * (BN / WN) + j * 32 + l31;
            const bool cok = col < a.Cout;
            const int colc = cok ? col : 0;
            const float bias = a.bias ? a.bias[colc] : 0.f;
            float sc = 1.f, sh = 0.f;
            if ((EPI == EPI_AFFINE_ACT || (EPI == EPI_GRU_OUT && a.out2)) && a.scale) { sc = a.scale[colc]; sh = a.shift[colc]; }
            long long liftoff = 0;
            if (EPI == EPI_AFFINE_ACT && a.lift > 0) {               // column (z, c), c fastest -> + z HW Cl + c
                const int Cl = a.Cout / a.lift, zc = colc / Cl;
                liftoff = (long long)zc * a.H * a.W * Cl + (colc - zc * Cl);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = wm * (32 * MT) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const long long orow = s_row[rl];
                    float v = acc[i][j][r] + bias;
                    if (cok && orow >= 0) {
                        if constexpr (EPI == EPI_BIAS) {
                            outp[orow * a.ldo + col] = v;
                        } else if constexpr (EPI == EPI_AFFINE_ACT) {
                            v = fmaf(v, sc, sh);
                            if (a.lift > 0) {
                                if (a.residual) v += a.residual[(m0 + rl) * a.ldr + col];      // residual rows are the un-lifted GEMM rows
                                v = v > 0.f ? v : v * a.slope;
                                a.out[orow + liftoff] = v;
                            } else {
                                if (a.residual) v += a.residual[orow * a.ldr + col];
                                v = v > 0.f ? v : v * a.slope;
                                a.out[orow * a.ldo + col] = v;
                            }
                        } else if constexpr (EPI == EPI_GRU_GATES) {
                            if (a.residual) v += a.residual[orow * a.ldr + col];       // precomputed input half conv(x, W_x) (shared across fusions)
                            const float g = 1.f / (1.f + expf(-v));          // torch.sigmoid's formula with the full-precision exponential (models/fusion.py:31-32)
                            if (col < Ch) a.out[orow * Ch + col] = g;
                            else {
                                a.out2[orow * Ch + (col - Ch)] = a.aux_h[orow * Ch + (col - Ch)] * g;
                                if (a.out3) a.out3[orow * Ch + (col - Ch)] = g;
                            }
                        } else {   // EPI_GRU_OUT
                            if (a.residual) v += a.residual[orow * a.ldr + col];
                            const float cand = tanhf(v);
                            const float z = a.aux_z[orow * a.Cout + col], h = a.aux_h[orow * a.Cout + col];
                            const float hn = h * (1.f - z) + cand * z;
                            a.out[orow * a.ldo + col] = hn;
                            if (a.out2) a.out2[orow * a.ldo + col] = fmaf(hn, sc, sh);
                            if (a.out3) a.out3[orow * a.ldo + col] = cand;
                        }
                    }
                }
            }
            if constexpr (EPI == EPI_BIAS) {
                if (a.stats) {                                       // workgroup-uniform, off the plain path: a second walk over this column's accumulators
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        double t1 = 0.0, t2 = 0.0;                   // this lane's share of column `col` in the 32-row block (rows beyond M excluded)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int rl = wm * (32 * MT) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                            if (s_row[rl] >= 0) {
                                const double v = (double)(acc[i][j][r] + bias);
                                t1 += v; t2 += v * v;
                            }
                        }
                        // the two half-waves hold the rows 4 (lane >> 5) + ... of the block: add them; lanes 0..31 then own one column each
                        t1 += __shfl_xor(t1, 32, 64); t2 += __shfl_xor(t2, 32, 64);
                        const long long blk = (m0 + wm * (32 * MT) + i * 32) >> 5;
                        if (half == 0 && cok) {
                            a.stats[(blk * 2) * a.Cout + col] = t1;
                            a.stats[(blk * 2 + 1) * a.Cout + col] = t2;
                        }
                    }
                }
            }
        }
    };
    if (a.ksplit > 1) {                                             // raw partial sums; conv_splitk_epilogue_kernel finishes the job
        float* wsl = a.ws + (long long)ks * M * a.Cout;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = n0 + wn * (BN / WN) + j * 32 + l31;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long m = m0 + wm * (32 * MT) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (col < a.Cout && m < M) wsl[m * a.Cout + col] = acc[i][j][r];
                }
        }
        return;
    }
    switch (a.epi) {
        case EPI_BIAS: epilogue(std::integral_constant<int, EPI_BIAS>{}); break;
        case EPI_AFFINE_ACT: epilogue(std::integral_constant<int, EPI_AFFINE_ACT>{}); break;
        case EPI_GRU_GATES: epilogue(std::integral_constant<int, EPI_GRU_GATES>{}); break;
        default: epilogue(std::integral_constant<int, EPI_GRU_OUT>{}); break;
    }
    FORGE_STAMP(3);
}



// Second half of a split-K launch: out = epilogue(sum_ks ws[ks][m][col]). One thread per 4 output channels; deterministic
// (fixed summation order), memory-bound (ksplit x M x Cout floats read once).
__global__ __launch_bounds__(256) void conv_splitk_epilogue_kernel(const ConvArgs a) {
    const long long M = (long long)a.n * a.D * a.H * a.W;
    const int C4 = a.Cout >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * C4) return;
    const long long m = idx / C4;
    const int col = (int)(idx - m * C4) << 2;
    float4 v = *reinterpret_cast<const float4*>(a.ws + m * a.Cout + col);
    for (int k = 1; k < a.ksplit; ++k) {
        const float4 p = *reinterpret_cast<const float4*>(a.ws + ((long long)k * M + m) * a.Cout + col);
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    long long orow = m;
    if ((a.os != 1) || (a.Do != a.D) || (a.Ho != a.H) || (a.Wo != a.W)) {
        long long q = m;
        const int x = (int)(q % a.W); q /= a.W;
        const int y = (int)(q % a.H); q /= a.H;
        const int z = (int)(q % a.D); q /= a.D;
        orow = ((q * a.Do + (z * a.os + a.pz)) * a.Ho + (y * a.os + a.py)) * a.Wo + (x * a.os + a.px);
    }
    float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int cc = col + c;
        float t = r[c] + (a.bias ? a.bias[cc] : 0.f);
        if (a.epi == EPI_AFFINE_ACT) {
            t = fmaf(t, a.scale[cc], a.shift[cc]);
            if (a.residual) t += a.residual[orow * a.ldr + cc];
            t = t > 0.f ? t : t * a.slope;
        }
        if (a.lift > 0) {
            const int Cl = a.Cout / a.lift, zc = cc / Cl, c2 = cc - zc * Cl;
            const long long HW = (long long)a.H * a.W, nn = m / HW, hw = m - nn * HW;
            a.out[((nn * a.lift + zc) * HW + hw) * Cl + c2] = t;
        } else {
            a.out[orow * a.ldo + cc] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Narrow-N variant for Cout <= 16 (render-feature / density convs of the heads, conv_rgb): a 128-wide
// N tile would waste >= 75 % of the matrix-core work, so this one uses v_mfma_f32_16x16x4_f32
// (16 output channels per MFMA, same 64 FLOP/clk/SIMD), tile 256(M) x 16(N) x 16(K), 8 waves x 32 rows.
// LDS images are [row][16 k] (64-byte rows); chunk c of row r is stored at c ^ g[(r>>2)&3], g = {0,3,2,1},
// which makes the 16-lane groups of ds_read_b128 (rows r..r+15, chunk = lane>>4) conflict-free.
typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr int BM16 = 256, BK16 = 16;

__device__ __forceinline__ int lds_off16(int row, int chunk) {
    return row * BK16 + ((chunk ^ ((4 - ((row >> 2) & 3)) & 3)) << 2);
}

__global__ __launch_bounds__(NTHREADS) void conv_igemm_n16_kernel(const ConvArgs a) {
    constexpr int A_FLOATS = BM16 * BK16, B_FLOATS = 16 * BK16;
    __shared__ __attribute__((aligned(16))) float smem[2 * (A_FLOATS + B_FLOATS)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long M = (long long)a.n * a.D * a.H * a.W;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    int phase = 0;
    if (a.nphase > 1) {                                             // merged transposed-conv phases (see conv_igemm_kernel)
        const unsigned tiles = (unsigned)((M + BM16 - 1) / BM16);
        phase = (int)(bid / tiles);
        bid -= (unsigned)phase * tiles;
    }
    const int pz = a.nphase > 1 ? (a.nphase == 8 ? (phase >> 2) & 1 : 0) : a.pz;
    const int py = a.nphase > 1 ? (phase >> 1) & 1 : a.py, px = a.nphase > 1 ? phase & 1 : a.px;
    const int t_lo = phase * a.tpp;
    const long long m0 = (long long)bid * BM16;
    const int Cin = a.C1 + a.C2;
    const int kchunks = Cin / BK16;
    const int nsteps = a.tpp * kchunks;

    const forge_v4i32 w1 = make_rsrc_words(a.in1, a.span1), w2 = make_rsrc_words(a.in2 ? a.in2 : a.in1, a.in2 ? a.span2 : 0),
                      ww = make_rsrc_words(a.wp, (long long)a.ntaps * a.Cout * Cin * 4);
    // LDS-DMA staging (common.h): A chunk j of this thread is LDS bytes 16 tid + 8192 j of the stage, the weight chunk (wave 0) bytes 16 tid of the B image
    const unsigned lds_wave = lds_addr(smem) + (unsigned)__builtin_amdgcn_readfirstlane(wave) * 1024u;

    const int cp = tid & 3;                                      // physical chunk in the 64-byte LDS row
    int ar[2], az[2], ay[2], ax[2], an[2], asrc[2];
    bool aval[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ar[j] = (tid >> 2) + 128 * j;
        const long long vl = m0 + ar[j];
        aval[j] = vl < M;
        unsigned v = aval[j] ? (unsigned)vl : 0u;
        unsigned q = v / (unsigned)a.W;
        ax[j] = (int)(v - q * (unsigned)a.W) * a.is; v = q;
        q = v / (unsigned)a.H;
        ay[j] = (int)(v - q * (unsigned)a.H) * a.is; v = q;
        q = v / (unsigned)a.D;
        az[j] = (int)(v - q * (unsigned)a.D) * a.is;
        an[j] = (int)q;
        asrc[j] = (cp ^ ((4 - ((ar[j] >> 2) & 3)) & 3)) << 2;
    }
    const int brow = tid >> 2;                                   // threads 0..63 stage the 16 x 16 weight tile
    const unsigned boff = (tid < 64 && brow < a.Cout) ? (unsigned)((brow * Cin + ((cp ^ ((4 - ((brow >> 2) & 3)) & 3)) << 2)) * 4) : OOB;

    int erow[2], erow2[2];
    auto prep_tap = [&](int t) {
        const int dz = a.tap[t][0], dy = a.tap[t][1], dx = a.tap[t][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int zi = az[j] + dz, yi = ay[j] + dy, xi = ax[j] + dx;
            const bool ok = aval[j] && (unsigned)zi < (unsigned)a.Di && (unsigned)yi < (unsigned)a.Hi && (unsigned)xi < (unsigned)a.Wi;
            const int sp = (zi * a.Hi + yi) * a.Wi + xi;
            erow[j] = ok ? an[j] * (int)a.bs1r + sp : -1;
            erow2[j] = ok ? an[j] * (int)a.bs2r + sp : -1;
        }
    };
    auto issue_step = [&](int t, int kc, int buf) {
        const int c0 = kc * BK16;
        const unsigned stage = lds_wave + (unsigned)buf * (unsigned)((A_FLOATS + B_FLOATS) * 4);
        if (c0 < a.C1) {
#pragma unroll
            for (int j = 0; j < 2; ++j) lds_dma16(w1, erow[j] < 0 ? OOB : (unsigned)((erow[j] * a.ld1 + c0 + asrc[j]) * 4), stage + (unsigned)(j * 8192));
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) lds_dma16(w2, erow2[j] < 0 ? OOB : (unsigned)((erow2[j] * a.ld2 + (c0 - a.C1) + asrc[j]) * 4), stage + (unsigned)(j * 8192));
        }
        if (wave == 0) lds_dma16(ww, boff == OOB ? OOB : boff + (unsigned)((t * a.Cout * Cin + c0) * 4), stage + (unsigned)(A_FLOATS * 4));
    };

    f32x4 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;

    const int kq = lane >> 4, l15 = lane & 15;
    int t = t_lo, kc = 0;
    prep_tap(t);
    issue_step(t, 0, 0);
    lds_dma_wait();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) {
            if (++kc == kchunks) { kc = 0; ++t; prep_tap(t); }
            issue_step(t, kc, buf ^ 1);                            // in flight under this step's MFMAs
        }
        const float* sa = smem + buf * (A_FLOATS + B_FLOATS);
        const float* sb = sa + A_FLOATS;
        const float4 fb = *reinterpret_cast<const float4*>(sb + lds_off16(l15, kq));
        float4 fa[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const float4*>(sa + lds_off16(wave * 32 + i * 16 + l15, kq));
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].x, fb.x, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].y, fb.y, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].z, fb.z, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].w, fb.w, acc[i], 0, 0, 0);
        lds_dma_wait();
        __syncthreads();
    }

    // ---- epilogue (bias / folded-BN + LeakyReLU + residual only). 16x16 C layout: col = lane & 15, row = (lane >> 4) * 4 + r
    // output rows through an LDS table (one 32-bit decomposition per tile row), as in conv_igemm_kernel
    long long* s_row = reinterpret_cast<long long*>(smem);          // [BM16]
    {
        const bool remap = (a.os != 1) || (a.Do != a.D) || (a.Ho != a.H) || (a.Wo != a.W);
        if (tid < BM16) {
            const long long m = m0 + tid;
            long long o = -1;
            if (m < M) {
                o = m;
                if (remap) {
                    unsigned q = (unsigned)m, t2 = q / (unsigned)a.W;
                    const int x = (int)(q - t2 * (unsigned)a.W); q = t2; t2 = q / (unsigned)a.H;
                    const int y = (int)(q - t2 * (unsigned)a.H); q = t2; t2 = q / (unsigned)a.D;
                    const int z = (int)(q - t2 * (unsigned)a.D);
                    o = (((long long)t2 * a.Do + (z * a.os + pz)) * a.Ho + (y * a.os + py)) * a.Wo + (x * a.os + px);
                }
            }
            s_row[tid] = o;
        }
        __syncthreads();
    }
    const int col = l15;
    if (col < a.Cout) {
        const float bias = a.bias ? a.bias[col] : 0.f;
        float sc = 1.f, sh = 0.f;
        if (a.epi == EPI_AFFINE_ACT) { sc = a.scale[col]; sh = a.shift[col]; }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long orow = s_row[wave * 32 + i * 16 + kq * 4 + r];
                if (orow >= 0) {
                    float v = acc[i][r] + bias;
                    if (a.epi == EPI_AFFINE_ACT) {
                        v = fmaf(v, sc, sh);
                        if (a.residual) v += a.residual[orow * a.ldr + col];
                        v = v > 0.f ? v : v * a.slope;
                    }
                    a.out[orow * a.ldo + col] = v;
                }
            }
    }
}


// Narrow-N kernel for stride-1 convolutions whose taps form complete x-LINES: taps [(dz, dy)] x [dx = -R .. R] (the 3x3x3 second convolutions of the
// heads, R = 1; conv_rgb's 5x5, R = 2). conv_igemm_n16_kernel stages the 256 tile rows once per TAP: at 16 output columns a K-step is 8 MFMAs per wave
// against a 16 KB global -> LDS round trip, so every one of its 54 (heads) / 50 (conv_rgb) K-steps is load-latency bound. The dx taps of one
// (dz, dy) line read the SAME rows shifted by dx voxels = dx rows of the channels-last tensor, so here a K-step stages the slab of 256 + 2R rows ONCE
// (LDS-DMA, common.h) and runs all 2R + 1 taps on shifted views of it: (2R + 1) x fewer global loads, barriers and K-steps, (2R + 1) x the MFMA
// work per barrier. A shifted row that crosses the end of its x-line is another line's voxel: masked per (row, dx) at use. Rows whose (z + dz, y + dy)
// leave the grid are staged as zeros. Same sums as conv_igemm_n16_kernel in a different order (taps of a line innermost).
template <int R>
__global__ __launch_bounds__(NTHREADS) void conv_igemm_n16_lines_kernel(const ConvArgs a) {
    constexpr int NT = 2 * R + 1, SR = BM16 + 2 * R;               // taps per line, slab rows
    constexpr int A_FLOATS = ((SR * BK16 + 255) / 256) * 256, B_FLOATS = NT * 16 * BK16;     // A padded to whole 1 KB wave blocks
    constexpr int APASS = (SR * 4 + NTHREADS - 1) / NTHREADS;      // 16-byte chunks of the slab per thread (3)
    __shared__ __attribute__((aligned(16))) float smem[2 * (A_FLOATS + B_FLOATS)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long M = (long long)a.n * a.D * a.H * a.W;
    const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const long long m0 = (long long)bid * BM16;
    const int Cin = a.C1 + a.C2;
    const int kchunks = Cin / BK16;
    const int nlines = a.ntaps / NT;
    const int nsteps = nlines * kchunks;
    const forge_v4i32 w1 = make_rsrc_words(a.in1, a.span1), w2 = make_rsrc_words(a.in2 ? a.in2 : a.in1, a.in2 ? a.span2 : 0),
                      ww = make_rsrc_words(a.wp, (long long)a.ntaps * a.Cout * Cin * 4);
    const unsigned lds_wave = lds_addr(smem) + (unsigned)__builtin_amdgcn_readfirstlane(wave) * 1024u;

    // slab chunk q = tid + 512 j: slab row q >> 2 = the voxel m0 - R + (q >> 2), physical 16-byte chunk q & 3 (LDS byte 16 q: lane-linear)
    const int cp = tid & 3;
    int sz[APASS], sy[APASS], sn[APASS], sx[APASS], asrc[APASS];
    bool sval[APASS];
#pragma unroll
    for (int j = 0; j < APASS; ++j) {
        const int srow = (tid + NTHREADS * j) >> 2;
        const long long vl = m0 - R + srow;
        sval[j] = srow < SR && vl >= 0 && vl < M;
        unsigned v = sval[j] ? (unsigned)vl : 0u;
        unsigned q = v / (unsigned)a.W;
        sx[j] = (int)(v - q * (unsigned)a.W); v = q;
        q = v / (unsigned)a.H;
        sy[j] = (int)(v - q * (unsigned)a.H); v = q;
        q = v / (unsigned)a.D;
        sz[j] = (int)(v - q * (unsigned)a.D);
        sn[j] = (int)q;
        asrc[j] = (cp ^ ((4 - ((srow >> 2) & 3)) & 3)) << 2;
    }
    // weights of a line: NT x 16 rows (tap-in-line, cout) x 4 chunks, staged by the first NT waves; LDS byte 16 tid of the B image
    const int brow = tid >> 2;
    const unsigned boff = (wave < NT && (brow & 15) < a.Cout)
                              ? (unsigned)((((brow >> 4) * a.Cout + (brow & 15)) * Cin + ((cp ^ ((4 - ((brow >> 2) & 3)) & 3)) << 2)) * 4) : OOB;
    int line = 0, kc = 0;
    auto issue_step = [&](int buf) {
        const int dz = a.tap[line * NT][0], dy = a.tap[line * NT][1];
        const int c0 = kc * BK16;
        const unsigned stage = lds_wave + (unsigned)buf * (unsigned)((A_FLOATS + B_FLOATS) * 4);
#pragma unroll
        for (int j = 0; j < APASS; ++j) {
            if ((tid + NTHREADS * j) < A_FLOATS / 4) {                 // whole waves in or out except in the last pass (exec-masked lanes do not write)
                const int zi = sz[j] + dz, yi = sy[j] + dy;
                const bool ok = sval[j] && (unsigned)zi < (unsigned)a.D && (unsigned)yi < (unsigned)a.H;
                const int sp = (zi * a.H + yi) * a.W + sx[j];
                unsigned off = OOB;
                if (c0 < a.C1) { if (ok) off = (unsigned)(((sn[j] * (int)a.bs1r + sp) * a.ld1 + c0 + asrc[j]) * 4); lds_dma16(w1, off, stage + (unsigned)(j * 8 * 1024)); }
                else { if (ok) off = (unsigned)(((sn[j] * (int)a.bs2r + sp) * a.ld2 + (c0 - a.C1) + asrc[j]) * 4); lds_dma16(w2, off, stage + (unsigned)(j * 8 * 1024)); }
            }
        }
        if (wave < NT) lds_dma16(ww, boff == OOB ? OOB : boff + (unsigned)((line * NT * a.Cout * Cin + c0) * 4), stage + (unsigned)(A_FLOATS * 4));
    };
    auto advance = [&]() { if (++kc == kchunks) { kc = 0; ++line; } };

    f32x4 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;
    const int kq = lane >> 4, l15 = lane & 15;
    int xr[2];                                                     // x coordinate of this lane's two MFMA rows: shifted reads beyond the line end are masked
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long m = m0 + wave * 32 + i * 16 + l15;
        xr[i] = (int)((unsigned)(m < M ? m : 0) % (unsigned)a.W);
    }
    issue_step(0);
    lds_dma_wait();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) { advance(); issue_step(buf ^ 1); }
        const float* sa = smem + buf * (A_FLOATS + B_FLOATS);
        const float* sb = sa + A_FLOATS;
#pragma unroll
        for (int d = 0; d < NT; ++d) {
            const float4 fb = *reinterpret_cast<const float4*>(sb + lds_off16(d * 16 + l15, kq));
            float4 fa[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const float4*>(sa + lds_off16(wave * 32 + i * 16 + l15 + d, kq));     // slab row = tile row + R + dx, d = dx + R
                if ((unsigned)(xr[i] + d - R) >= (unsigned)a.W) fa[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].x, fb.x, acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].y, fb.y, acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].z, fb.z, acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].w, fb.w, acc[i], 0, 0, 0);
        }
        lds_dma_wait();
        __syncthreads();
    }
    // ---- epilogue (bias / folded-BN + LeakyReLU + residual): identity row mapping (stride 1, same grid). 16x16 C layout: col = lane & 15, row = (lane >> 4) * 4 + r
    const int col = l15;
    if (col < a.Cout) {
        const float bias = a.bias ? a.bias[col] : 0.f;
        float sc = 1.f, sh = 0.f;
        if (a.epi == EPI_AFFINE_ACT) { sc = a.scale[col]; sh = a.shift[col]; }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long orow = m0 + wave * 32 + i * 16 + kq * 4 + r;
                if (orow < M) {
                    float v = acc[i][r] + bias;
                    if (a.epi == EPI_AFFINE_ACT) {
                        v = fmaf(v, sc, sh);
                        if (a.residual) v += a.residual[orow * a.ldr + col];
                        v = v > 0.f ? v : v * a.slope;
                    }
                    a.out[orow * a.ldo + col] = v;
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Launch plan: tile shape and split-K factor from a makespan model of the 256-CU chip (times in us).
//   tiles      A 128x128 / 8 waves   B 64x128 / 8   C 128x64 / 8   D 64x64 / 4   E 128x32 / 4 (Cout <= 32)
//   tile_us    = BM x BN x K-steps / (8000 x eff): CU-time of one tile with the CU's resident workgroups saturating the MFMA
//                pipes; eff = measured rate of each tile on M = 131072 problems relative to tile A (130 TF)
//   makespan   = full waves of 256 x occupancy workgroups, then the remainder with r = ceil(rem / 256) workgroups per CU running at
//                g(r)/g(occ) of the saturated rate (a lone workgroup cannot overlap its own barriers: g(1) = 0.8); floored by the
//                operand/result traffic at 4 TB/s (short-K 1x1 convs are traffic-bound; narrow N tiles re-read A); plus a
//                prologue/epilogue term per round, larger for tile A whose 2 resident workgroups overlap it worst
//   split-K    slices K across workgroups when the chip is under-filled (M = 5120: ResNet, one scene); costs the reduction kernel
// Constants fitted (tools/fit_plan_model.py) on tools/conv_plan_sweep.py (54 shapes x 30 plans, 1 and 4 scenes; re-fitted in round 3 for the
// LDS-DMA loop, which moved the 64x128 tile from 0.98 to 1.06 of tile A): chosen plans are within 0.5 % / 0.1 % of the per-shape best in total. Callers may pass an explicit (tile, ksplit) to forge_conv_igemm instead (tools/conv_plan_sweep.py, tests).
struct ConvPlan { char tile; int ksplit; };

static ConvPlan plan_conv(long long M, int Cout, int Cin, int ntaps, bool can_split, long long ws_bytes) {
    struct Tile { char id; int bm, bn, occ; double eff, ov; };
    static const Tile tiles[5] = {{'A', 128, 128, 2, 1.00, 1.0}, {'B', 64, 128, 3, 1.06, 0.5}, {'C', 128, 64, 3, 0.93, 0.5},
                                  {'D', 64, 64, 5, 0.90, 1.0}, {'E', 128, 32, 4, 0.90, 0.5}};
    static const int splits[6] = {1, 2, 3, 4, 6, 8};
    auto g = [](long long o) { return o <= 1 ? 0.8 : o == 2 ? 0.85 : o == 3 ? 0.96 : 1.0; };
    const int nsteps = ntaps * (Cin / BK);
    const double K = (double)ntaps * Cin;
    ConvPlan best{'D', 1};
    double best_us = 1e300;
    for (const Tile& t : tiles) {
        if (t.id == 'E' && Cout > 32) continue;
        const long long ntn = (Cout + t.bn - 1) / t.bn;
        const long long nb = ((M + t.bm - 1) / t.bm) * ntn;
        for (int k : splits) {
            if (k > 1 && (!can_split || nsteps / k < 8 || (long long)k * M * Cout * 4 > ws_bytes)) continue;
            const long long wgs = nb * k, slots = 256LL * t.occ;
            const long long full = wgs / slots, rem = wgs - full * slots;
            const double tile_us = (double)t.bm * t.bn * ((nsteps + k - 1) / k) / (8000.0 * t.eff);
            double us = (double)full * t.occ * tile_us;
            long long rounds = full;
            if (rem > 0) {
                const long long r = (rem + 255) / 256;
                us += (double)r * tile_us * g(t.occ) / g(r);
                ++rounds;
            }
            const double traffic_us = ((double)M * K * 4.0 * ntn + (double)Cout * K * 4.0 + (double)M * Cout * 4.0) / 4.0e6;
            if (us < traffic_us) us = traffic_us;
            us += (double)(rounds + 1) * t.ov * sqrt((double)t.bm * t.bn / 16384.0);
            if (k > 1) us += 3.0 + (double)(k + 1) * M * Cout * 4.0 / 2.0e6;
            if (us < best_us) { best_us = us; best = ConvPlan{t.id, k}; }
        }
    }
    return best;
}

// Launch one of the point-GEMM forms (64 x 128 tile, 8 waves): the tiles of every `planes`-th plane x ceil(Cout / 128) workgroups per batched problem.
template <int RS>
static int launch_point_form(const ConvArgs& a, int planes, size_t lds, const char* entry, hipStream_t st) {
    const long long M = (long long)a.n * a.D * a.H * a.W;
    const long long grid = ((M + 64 * planes - 1) / (64 * planes)) * ((a.Cout + 127) / 128) * a.nbat;
    FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "%s: grid too large", entry);
    FORGE_REQUIRE(RS != 1 || M * a.ldo * 4 < (1ll << 31), FORGE_ESHAPE, "%s: an output plane spans >= 2 GiB (32-bit buffer offsets); split the batch", entry);
    FORGE_SET_MAX_LDS_ONCE((conv_igemm_kernel<64, 128, 8, 1, RS>), lds);
    hipLaunchKernelGGL((conv_igemm_kernel<64, 128, 8, 1, RS>), dim3((unsigned)grid), dim3(8 * 64), lds, st, a);
    return 0;
}

// Which epilogue a launch of the convolution body (RS = 0) takes: true = the direct-store epilogue (see the kernel). It needs identity output rows
// (no stride / phase remap, no lift), a plain bias or affine epilogue without split-K partials or the statistics by-product, and an output (and
// residual) whose written byte range ((M - 1) ld + Cout) 4 fits 32-bit buffer offsets; ld >= Cout puts the rows beyond M beyond that range, and
// ld < 2^22 keeps the offsets of a ragged tile's dropped rows (at most 127 rows further down) from wrapping round 2^32 into it.
static bool g_conv_fast_epilogue = true;        // forge_conv_fast_epilogue(): process-wide, for A/B measurements and tests

static bool conv_fast_epilogue_applies(long long M, int Cout, int ldo, int ldr, bool residual, int os, bool same_grid, int nphase, int lift, int ksplit,
                                       bool stats, int epi) {
    if (ksplit != 1 || os != 1 || !same_grid || nphase != 1 || lift != 0 || stats) return false;
    if (epi != EPI_BIAS && epi != EPI_AFFINE_ACT) return false;
    if (M < 1 || Cout < 1 || ldo < Cout || ldo >= (1 << 22) || ((M - 1) * ldo + Cout) * 4 >= (1ll << 31)) return false;
    if (residual && epi == EPI_AFFINE_ACT && (ldr < Cout || ldr >= (1 << 22) || ((M - 1) * ldr + Cout) * 4 >= (1ll << 31))) return false;
    return true;
}

// Launch conv_igemm_kernel with the planned tile: ceil(M / BM) x ceil(Cout / BN) workgroups per (K slice, phase, batched problem).
static int launch_conv_tile(const ConvArgs& args, char tile, hipStream_t st, int row_stage = 0) {
    ConvArgs a = args;
    const long long M = (long long)a.n * a.D * a.H * a.W;
    a.flat_rows = row_stage == 0 && a.ntaps == 1 && a.nphase == 1 && a.tap[0][0] == 0 && a.tap[0][1] == 0 && a.tap[0][2] == 0 && a.is == 1 && a.Di == a.D &&
                  a.Hi == a.H && a.Wi == a.W && a.bs1r == (long long)a.D * a.H * a.W && (a.in2 == nullptr || a.bs2r == a.bs1r);
    a.fast_epi = row_stage == 0 && g_conv_fast_epilogue && (a.nbat == 1 || a.epi == EPI_BIAS) &&
                 conv_fast_epilogue_applies(M, a.Cout, a.ldo, a.ldr, a.residual != nullptr, a.os, a.Do == a.D && a.Ho == a.H && a.Wo == a.W, a.nphase, a.lift,
                                            a.ksplit, a.stats != nullptr, a.epi);
    auto nblk = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((a.Cout + bn - 1) / bn); };
    // the forms: a.nbat = 4 point columns with four points per workgroup (RS = 1) / 16 points on the even planes (2) / on every fourth plane (3)
    if (row_stage == 1) { const size_t lds = RS_STAGES * (64 * BK + 128 * BK) * sizeof(float); return launch_point_form<1>(a, 1, lds, "forge_wino_gemm_half", st); }
    if (row_stage == 2) { const size_t lds = RS_STAGES * (2 * 64 * BK + 128 * BK) * sizeof(float); return launch_point_form<2>(a, 2, lds, "forge_wino_gemm_dn", st); }
    if (row_stage == 3) { const size_t lds = RS_STAGES * (64 * BK + 128 * BK) * sizeof(float); return launch_point_form<3>(a, 4, lds, "forge_wino_gemm_dn4", st); }
#define FORGE_LAUNCH_CONV(BMv, BNv, NWv)                                                                                   \
    do {                                                                                                                   \
        const long long grid = nblk(BMv, BNv) * a.ksplit * a.nphase * a.nbat;                                              \
        FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "forge_conv_igemm: grid too large");                                \
        const size_t lds = 2 * (BMv * BK + BNv * BK) * sizeof(float);                                                      \
        FORGE_SET_MAX_LDS_ONCE((conv_igemm_kernel<BMv, BNv, NWv>), lds);                                                   \
        hipLaunchKernelGGL((conv_igemm_kernel<BMv, BNv, NWv>), dim3((unsigned)grid), dim3(NWv * 64), lds, st, a);          \
    } while (0)
    switch (tile) {
        case 'A': FORGE_LAUNCH_CONV(128, 128, 8); break;
        case 'B': FORGE_LAUNCH_CONV(64, 128, 8); break;
        case 'C': FORGE_LAUNCH_CONV(128, 64, 8); break;
        case 'E': FORGE_LAUNCH_CONV(128, 32, 4); break;
        default: FORGE_LAUNCH_CONV(64, 64, 4); break;
    }
#undef FORGE_LAUNCH_CONV
    return 0;
}

}  // namespace forge

using namespace forge;

extern "C" int forge_conv_igemm_plan(long long M, int Cout, int Cin, int ntaps, int nphase, int epilogue, int ldo, long long splitk_ws_bytes,
                                     int* tile, int* ksplit) {
    FORGE_REQUIRE(tile && ksplit && M > 0 && Cout > 0 && Cin > 0 && ntaps > 0 && (nphase == 1 || nphase == 4 || nphase == 8) && ntaps % nphase == 0,
                  FORGE_EINVAL, "forge_conv_igemm_plan: bad argument");
    if (Cout <= 16) { *tile = 'N'; *ksplit = 1; return 0; }                         // conv_igemm_n16_kernel
    const ConvPlan pl = plan_conv(M * nphase, Cout, Cin, ntaps / nphase,
                                  nphase == 1 && splitk_ws_bytes > 0 && (epilogue == EPI_BIAS || epilogue == EPI_AFFINE_ACT) && Cout % 4 == 0 && ldo % 4 == 0,
                                  splitk_ws_bytes);
    *tile = pl.tile; *ksplit = pl.ksplit;
    return 0;
}

// The process-wide switch of the direct-store epilogue (default on) and the rule that selects it; see include/forge_hip.h. Host arithmetic only.
extern "C" int forge_conv_fast_epilogue(int on) {
    const int prev = g_conv_fast_epilogue;
    if (on >= 0) g_conv_fast_epilogue = on != 0;
    return prev;
}

extern "C" int forge_conv_igemm_epilogue(long long M, int Cout, int ldo, int ldr, int has_residual, int os, int same_grid, int nphase, int lift, int ksplit,
                                         int has_stats, int epilogue, int* fast) {
    FORGE_REQUIRE(fast && M > 0 && Cout > 0 && ldo > 0 && os >= 1 && nphase >= 1 && lift >= 0 && ksplit >= 1 && epilogue >= 0 && epilogue <= 3, FORGE_EINVAL,
                  "forge_conv_igemm_epilogue: bad argument");
    *fast = Cout > 16 && g_conv_fast_epilogue &&
            conv_fast_epilogue_applies(M, Cout, ldo, ldr, has_residual != 0, os, same_grid != 0, nphase, lift, ksplit, has_stats != 0, epilogue);
    return 0;
}

// Generic entry; see include/forge_hip.h for the contract.
extern "C" int forge_conv_igemm(const float* in1, int C1, int ld1, long long bs1, const float* in2, int C2, int ld2, long long bs2,
                                const float* wp,
                                const float* bias, const float* scale, const float* shift, float slope, const float* residual,
                                const float* aux_h, const float* aux_z, float* out, float* out2, float* out3,
                                int n, int D, int H, int W, int is, int Di, int Hi, int Wi, int Cout, int ldo,
                                const int* taps, int ntaps, int os, int pz, int py, int px, int Do, int Ho, int Wo,
                                int epilogue, int lift, int tile, int ksplit, float* splitk_ws, long long splitk_ws_bytes, double* stats,
                                forge_stream_t stream) {
    FORGE_REQUIRE(in1 && wp && out && taps, FORGE_EINVAL, "forge_conv_igemm: null pointer argument");
    FORGE_REQUIRE(stats == nullptr || (epilogue == EPI_BIAS && ksplit <= 1 && Cout > 16 && !(pz < 0) && lift == 0), FORGE_EINVAL,
                  "forge_conv_igemm: output statistics need the plain bias epilogue of the wide kernel without split-K, phases or lift");
    FORGE_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0 && Cout > 0 && ntaps > 0 && ntaps <= MAX_TAPS, FORGE_EINVAL,
                  "forge_conv_igemm: bad dims n=%d D=%d H=%d W=%d Cout=%d ntaps=%d", n, D, H, W, Cout, ntaps);
    const int kstep = Cout <= 16 ? 16 : 32;
    FORGE_REQUIRE(C1 > 0 && C1 % kstep == 0 && C2 >= 0 && C2 % kstep == 0, FORGE_ESHAPE,
                  "forge_conv_igemm: C1=%d / C2=%d must be multiples of the K-step %d (16 for Cout <= 16, else 32)", C1, C2, kstep);
    FORGE_REQUIRE((C2 == 0) == (in2 == nullptr), FORGE_EINVAL, "forge_conv_igemm: in2/C2 mismatch");
    FORGE_REQUIRE(epilogue >= 0 && epilogue <= 3, FORGE_EINVAL, "forge_conv_igemm: unknown epilogue %d", epilogue);
    FORGE_REQUIRE(epilogue != EPI_AFFINE_ACT || (scale && shift), FORGE_EINVAL, "forge_conv_igemm: affine epilogue needs scale/shift");
    FORGE_REQUIRE(epilogue != EPI_GRU_GATES || (aux_h && out2 && Cout % 2 == 0), FORGE_EINVAL, "forge_conv_igemm: GRU gate epilogue needs aux_h, out2");
    FORGE_REQUIRE(epilogue != EPI_GRU_OUT || (aux_h && aux_z), FORGE_EINVAL, "forge_conv_igemm: GRU out epilogue needs aux_h, aux_z");
    FORGE_REQUIRE(os >= 1 && Do > 0 && Ho > 0 && Wo > 0, FORGE_EINVAL, "forge_conv_igemm: bad output mapping");
    FORGE_REQUIRE(is >= 1 && Di > 0 && Hi > 0 && Wi > 0, FORGE_EINVAL, "forge_conv_igemm: bad input mapping");
    FORGE_REQUIRE(lift == 0 || (lift > 0 && epilogue == EPI_AFFINE_ACT && Cout % lift == 0 && D == 1 && os == 1 && Cout > 64), FORGE_EINVAL,
                  "forge_conv_igemm: lift needs the affine epilogue on a 2-D (D=1) conv with Cout %% lift == 0 and Cout > 64");
    FORGE_REQUIRE(ld1 >= C1 && ld1 % 4 == 0 && (C2 == 0 || (ld2 >= C2 && ld2 % 4 == 0)) && ldo >= 1, FORGE_EINVAL,
                  "forge_conv_igemm: row strides must cover the channels and keep 16-byte alignment");
    ConvArgs a;
    a.in1 = in1; a.in2 = in2; a.C1 = C1; a.C2 = C2; a.ld1 = ld1; a.ld2 = ld2;
    a.bs1r = bs1 > 0 ? bs1 : (long long)Di * Hi * Wi; a.bs2r = bs2 > 0 ? bs2 : (long long)Di * Hi * Wi;
    a.span1 = ((long long)(n - 1) * a.bs1r + (long long)Di * Hi * Wi) * ld1 * 4;
    a.span2 = in2 ? ((long long)(n - 1) * a.bs2r + (long long)Di * Hi * Wi) * ld2 * 4 : 0;
    FORGE_REQUIRE(a.span1 < (1ll << 31) && a.span2 < (1ll << 31) && (long long)ntaps * Cout * (C1 + C2) * 4 < (1ll << 31), FORGE_ESHAPE,
                  "forge_conv_igemm: an operand spans >= 2 GiB (32-bit buffer offsets); split the batch");
    a.is = is; a.Di = Di; a.Hi = Hi; a.Wi = Wi; a.residual = residual;
    a.ldr = (lift > 0 || epilogue == EPI_GRU_GATES || epilogue == EPI_GRU_OUT) ? Cout : ldo;
    a.lift = lift; a.ws = nullptr; a.ksplit = 1; a.stats = stats; a.flat_rows = a.fast_epi = 0;
    a.wp = wp; a.bias = bias; a.scale = scale; a.shift = shift; a.slope = slope;
    a.aux_h = aux_h; a.aux_z = aux_z; a.out = out; a.out2 = out2; a.out3 = out3; a.n = n; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.ldo = ldo;
    a.ntaps = ntaps; a.os = os; a.pz = pz; a.py = py; a.px = px; a.Do = Do; a.Ho = Ho; a.Wo = Wo; a.epi = epilogue;
    a.nphase = 1; a.tpp = ntaps; a.nbat = 1; a.pt1 = a.pt2 = a.ptw = a.pto = 0;
    if (pz < 0) {   // all output phases of a stride-2 transposed convolution in one launch
        FORGE_REQUIRE(os == 2 && py < 0 && px < 0 && Ho == 2 * H && Wo == 2 * W && (Do == 2 * D || Do == D), FORGE_EINVAL,
                      "forge_conv_igemm: merged phases (pz = py = px = -1) need os = 2 and a doubled output grid");
        a.nphase = Do == 2 * D ? 8 : 4;
        FORGE_REQUIRE(ntaps % a.nphase == 0, FORGE_EINVAL, "forge_conv_igemm: merged phases need ntaps %% %d == 0", a.nphase);
        a.tpp = ntaps / a.nphase;
        a.pz = a.py = a.px = 0;
    }
    for (int k = 0; k < 3 * ntaps; ++k)       // the kernels carry the taps as signed bytes
        FORGE_REQUIRE(taps[k] >= -128 && taps[k] <= 127, FORGE_EINVAL, "forge_conv_igemm: tap %d component %d = %d outside [-128, 127]", k / 3, k % 3, taps[k]);
    for (int t = 0; t < MAX_TAPS; ++t) {
        for (int k = 0; k < 3; ++k) a.tap[t][k] = (signed char)(t < ntaps ? taps[t * 3 + k] : 0);
        a.tap[t][3] = 0;
    }
    const long long M = (long long)n * D * H * W;
    FORGE_REQUIRE(M < (1ll << 31), FORGE_ESHAPE, "forge_conv_igemm: more than 2^31 GEMM rows; split the batch");
    FORGE_REQUIRE(out3 == nullptr || epilogue == EPI_GRU_GATES || epilogue == EPI_GRU_OUT, FORGE_EINVAL, "forge_conv_igemm: out3 is a GRU-epilogue output");
    hipStream_t st = (hipStream_t)stream;
    if (Cout <= 16) {
        FORGE_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_AFFINE_ACT, FORGE_EINVAL, "forge_conv_igemm: GRU epilogues need Cout > 16");
        const long long grid = (M + BM16 - 1) / BM16 * a.nphase;
        FORGE_REQUIRE(grid < (1ll << 31), FORGE_ESHAPE, "forge_conv_igemm: grid too large");
        // stride-1 convolution on its own grid whose taps are complete x-lines [(dz, dy)] x [dx = -R .. R], dx fastest (R = 1, 2): the lines kernel
        int lines_r = 0;
        if (a.nphase == 1 && is == 1 && os == 1 && lift == 0 && Do == D && Ho == H && Wo == W && Di == D && Hi == H && Wi == W && pz == 0 && py == 0 && px == 0) {
            for (int r = 1; r <= 2 && !lines_r; ++r) {
                const int nt = 2 * r + 1;
                bool ok = ntaps % nt == 0 && W > r;
                for (int t = 0; ok && t < ntaps; ++t)
                    ok = taps[t * 3 + 2] == (t % nt) - r && taps[t * 3] == taps[(t - t % nt) * 3] && taps[t * 3 + 1] == taps[(t - t % nt) * 3 + 1];
                if (ok) lines_r = r;
            }
        }
        if (lines_r == 1) hipLaunchKernelGGL(conv_igemm_n16_lines_kernel<1>, dim3((unsigned)grid), dim3(NTHREADS), 0, st, a);
        else if (lines_r == 2) hipLaunchKernelGGL(conv_igemm_n16_lines_kernel<2>, dim3((unsigned)grid), dim3(NTHREADS), 0, st, a);
        else hipLaunchKernelGGL(conv_igemm_n16_kernel, dim3((unsigned)grid), dim3(NTHREADS), 0, st, a);
    } else {
        const bool can_split = a.nphase == 1 && splitk_ws && (epilogue == EPI_BIAS || epilogue == EPI_AFFINE_ACT) && Cout % 4 == 0 && ldo % 4 == 0;
        ConvPlan pl;
        if (tile == 0) {
            pl = plan_conv(M * a.nphase, Cout, C1 + C2, a.tpp, can_split, splitk_ws_bytes);
        } else {                                                       // the caller's plan (forge_conv_igemm_plan's answer, or a sweep / test override)
            pl = ConvPlan{(char)tile, ksplit > 1 ? ksplit : 1};
            FORGE_REQUIRE(tile >= 'A' && tile <= 'E', FORGE_EINVAL, "forge_conv_igemm: tile '%c' is not one of A..E (0 = planned here)", (char)tile);
            FORGE_REQUIRE(pl.ksplit == 1 || (can_split && pl.ksplit <= 8 && (long long)pl.ksplit * M * Cout * 4 <= splitk_ws_bytes &&
                                             pl.ksplit <= a.tpp * ((C1 + C2) / BK)), FORGE_EINVAL,
                          "forge_conv_igemm: ksplit=%d needs epilogue 0/1 without phases, Cout, ldo %% 4 == 0 and a workspace of ksplit M Cout floats", pl.ksplit);
        }
        // the statistics by-product is written by the GEMM epilogue in 32-row blocks of the PLANNED tile: a caller that asks for it must know the
        // tile (to size `stats` and to tell forge_bn_train_fwd how many blocks to read) and must not land on a split-K plan, whose launches skip
        // the epilogue - so it has to hand the plan over (forge_conv_igemm_plan) instead of leaving it to this call
        FORGE_REQUIRE(stats == nullptr || (tile != 0 && pl.ksplit == 1), FORGE_EINVAL,
                      "forge_conv_igemm: output statistics need an explicit tile ('A'..'E' from forge_conv_igemm_plan) and a plan without split-K");
        if (pl.ksplit > 1) { a.ksplit = pl.ksplit; a.ws = splitk_ws; }
        if (int rc = launch_conv_tile(a, pl.tile, st)) return rc;
        if (a.ksplit > 1) {
            const long long total = M * (Cout / 4);
            hipLaunchKernelGGL(conv_splitk_epilogue_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
        }
    }
    FORGE_LAUNCH_CHECK("forge_conv_igemm");
    return 0;
}

// Workgroup tile of forge_wino_gemm for R tile rows per point and K = kd Cin. The makespan model (plan_conv) was fitted on single-problem
// launches; for the 16 short-K problems of one launch the measured optimum (tools/wino_gemm_sweep.py at 1 and 4 scenes, round 3, LDS-DMA loop)
// is the 64x128 tile on every shape of the step (gates 129 TF against 127 / 122 for 128x128 / 64x64; state 128 / 125 / 121; conv1 102 / 98 / 93);
// the 2-D trunk's tiny launches want many small workgroups. forge_wino_gemm's `tile` argument overrides it (that tool).
extern "C" int forge_wino_gemm_tile(long long R, int Cout, int Cin) {
    (void)Cin;
    if (Cout <= 64) return R < 2048 ? 'D' : 'C';               // a 64-wide output (conv1's data gradient, 128 -> 64) would leave half of a 64x128 tile's columns empty
    return R < 2048 ? 'D' : 'B';                                // R < 2048: the 2-D trunk's layer3/4 (R = 320 / 80)
}

// The 16 point-GEMMs of a Winograd F(2x2, 3x3) x 3-depth-tap convolution (winograd.hip) in ONE launch: problem p = (i, j) multiplies
// the transformed inputs V[p] (rows = (n, z, tile row, tile col), channels-last, the channel concatenation of V1 and V2) with the
// transformed weights U[p] [kd depth taps][Cout][C1 + C2] into Mm[p] [rows][Cout] - a kd-tap implicit GEMM over the tile grid, K = kd (C1 + C2);
// kd = 3 for the 3x3x3 convolutions, kd = 1 for the 3x3 convolutions of a 2-D network (D = 1 or D = images: planes do not mix).
static int wino_gemm_impl(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                          long long pt2, const float* U, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, int tile, int form, forge_stream_t stream) {
    // form: 0 = 16 points, 1 = the four-point row stage, 2 = the depth nest, 3 = its F(4, 3) form, 4 = that form on the 24 points of F(4, 3) along H (the same launch
    // with 24 batched problems on the grid of 4 x 2 tiles), 5 = on the 36 points of F(4, 3) along H and W (36 problems on the grid of 4 x 4 tiles)
    const bool half = form == 1, dn = form == 2, dn4hw = form == 5, dn4h = form == 4 || dn4hw, dn4 = form == 3 || dn4h;
    const char* const name4 = dn4hw ? "forge_wino_gemm_dn4hw" : dn4h ? "forge_wino_gemm_dn4h" : "forge_wino_gemm_dn4";
    FORGE_REQUIRE(tile == 0 || (tile >= 'A' && tile <= 'E'), FORGE_EINVAL, "forge_wino_gemm: tile must be 0 (default rule) or 'A'..'E'");
    FORGE_REQUIRE(V1 && U && Mm && (kd == 1 || kd == 3), FORGE_EINVAL, "forge_wino_gemm: null pointer argument / kd not 1 or 3");
    FORGE_REQUIRE(n > 0 && D > 0 && Ht > 0 && Wt > 0 && Cout > 16, FORGE_EINVAL, "forge_wino_gemm: bad dims n=%d D=%d Ht=%d Wt=%d Cout=%d (Cout > 16)", n,
                  D, Ht, Wt, Cout);
    FORGE_REQUIRE(C1 > 0 && C1 % BK == 0 && C2 >= 0 && C2 % BK == 0 && (C2 == 0) == (V2 == nullptr), FORGE_ESHAPE,
                  "forge_wino_gemm: C1=%d / C2=%d must be multiples of %d, V2 given iff C2 > 0", C1, C2, BK);
    FORGE_REQUIRE(ld1 >= C1 && ld1 % 4 == 0 && (C2 == 0 || (ld2 >= C2 && ld2 % 4 == 0)), FORGE_EINVAL, "forge_wino_gemm: bad row strides");
    FORGE_REQUIRE(!dn || (kd == 3 && D % 2 == 0 && ((long long)Ht * Wt) % 64 == 0), FORGE_EINVAL,
                  "forge_wino_gemm_dn: needs three depth taps, an even D and Ht Wt %% 64 == 0 (kd=%d D=%d Ht=%d Wt=%d)", kd, D, Ht, Wt);
    FORGE_REQUIRE(!dn4 || (kd == 3 && D % 4 == 0 && ((long long)Ht * Wt) % 64 == 0), FORGE_EINVAL,
                  "%s: needs three depth taps, D %% 4 == 0 and Ht Wt %% 64 == 0 (kd=%d D=%d Ht=%d Wt=%d)", name4, kd, D, Ht, Wt);
    FORGE_REQUIRE(!dn4h || D >= 8, FORGE_EINVAL, "%s: D=%d must be at least 8", name4, D);
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    // operand rows per batch element and K loops per tile: vol rows and the kd depth taps; depth nest: U' [16][4][Cout][Cin], the four depth positions
    // take the place of the taps; its F(4, 3) form: V6 [n][D/4][6][Ht Wt] = 1.5 vol rows, U'' [16][6][Cout][Cin]
    const long long vol = (long long)D * Ht * Wt, R = (long long)n * vol, rows = dn4 ? vol / 4 * 6 : vol, Cin = C1 + C2;
    const int npos = dn4 ? 6 : dn ? 4 : kd;
    a.in1 = V1; a.in2 = V2; a.C1 = C1; a.C2 = C2; a.ld1 = ld1; a.ld2 = ld2; a.bs1r = bs1 > 0 ? bs1 : rows; a.bs2r = bs2 > 0 ? bs2 : rows;
    a.span1 = ((long long)(n - 1) * a.bs1r + rows) * ld1 * 4;
    a.span2 = V2 ? ((long long)(n - 1) * a.bs2r + rows) * ld2 * 4 : 0;
    if (dn4) {
        FORGE_REQUIRE(a.span1 < (1ll << 31) && a.span2 < (1ll << 31) && R * Cout * 4 < (1ll << 31) && 6ll * Cout * Cin * 4 < (1ll << 31), FORGE_EINVAL,
                      "%s: an operand or an output plane spans >= 2 GiB (32-bit buffer offsets); split the batch", name4);
    } else {
        FORGE_REQUIRE(a.span1 < (1ll << 31) && a.span2 < (1ll << 31) && R < (1ll << 31), FORGE_ESHAPE,
                      "forge_wino_gemm: an operand spans >= 2 GiB per Winograd point (32-bit buffer offsets); split the batch");
        FORGE_REQUIRE(!dn || (R * Cout * 4 < (1ll << 31) && 4ll * Cout * Cin * 4 < (1ll << 31)), FORGE_ESHAPE,
                      "forge_wino_gemm_dn: an output plane spans >= 2 GiB (32-bit buffer offsets); split the batch");
    }
    a.wp = U; a.slope = 1.f; a.out = Mm; a.n = n; a.D = D; a.H = Ht; a.W = Wt; a.is = 1; a.Di = D; a.Hi = Ht; a.Wi = Wt;
    a.Cout = Cout; a.ldo = Cout; a.ldr = Cout; a.ntaps = a.tpp = npos; a.os = 1; a.Do = D; a.Ho = Ht; a.Wo = Wt; a.nphase = 1; a.epi = EPI_BIAS;
    a.ksplit = 1; a.nbat = half ? 4 : dn4hw ? 36 : dn4h ? 24 : 16;
    a.pt1 = pt1 > 0 ? pt1 : (long long)n * rows * ld1; a.pt2 = V2 ? (pt2 > 0 ? pt2 : (long long)n * rows * ld2) : 0;   // 0 = dense planes, as forge_wino_wgrad reads it
    a.ptw = (long long)npos * Cout * Cin; a.pto = R * Cout;
    if (form == 0 || half) {
        if (kd == 3) { a.tap[0][0] = -1; a.tap[2][0] = 1; }             // depth taps (-1,0,0), (0,0,0), (1,0,0); kd = 1: the 2-D convolution's single tap
        if (!tile) tile = forge_wino_gemm_tile(R, Cout, C1 + C2);
    }
    if (int rc = launch_conv_tile(a, (char)tile, (hipStream_t)stream, dn4h ? 3 : form)) return rc;
    FORGE_LAUNCH_CHECK(dn4 ? name4 : dn ? "forge_wino_gemm_dn" : "forge_wino_gemm");
    return 0;
}

extern "C" int forge_wino_gemm(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                               long long pt2, const float* U, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, int tile, forge_stream_t stream) {
    return wino_gemm_impl(V1, C1, ld1, bs1, pt1, V2, C2, ld2, bs2, pt2, U, Mm, n, D, Ht, Wt, Cout, kd, tile, 0, stream);
}

// forge_wino_gemm with the ROW stage of the inverse transform applied in the GEMM's epilogue (conv_igemm_kernel<..., RS = 1>): Mm8 [2][4][R][Cout],
// Mm8[i'][j] = sum over the four points (i, j) of A^T[i'][i] Mm[i][j] = (m0 + m1) + m2 | (m1 - m2) - m3 - bitwise what forge_wino_output computes
// first. forge_wino_output_half finishes the transform. 64 x 128 tile only (the launches forge_wino_gemm_tile gives 'B').
extern "C" int forge_wino_gemm_half(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                                    long long pt2, const float* U, float* Mm8, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream) {
    return wino_gemm_impl(V1, C1, ld1, bs1, pt1, V2, C2, ld2, bs2, pt2, U, Mm8, n, D, Ht, Wt, Cout, kd, 'B', 1, stream);
}

// forge_wino_gemm through the depth nest (conv_igemm_kernel<64, 128, 8, 1, 2>): the same 16 point products Mm [16][R][Cout] of a three-depth-tap problem,
// made with four K loops of C1 + C2 per plane pair instead of six, against Ud = U' [16][4][Cout][C1 + C2] (forge_wino_weights_dn). Rounded in another
// order than forge_wino_gemm: not bitwise its result. FORGE_EINVAL unless kd == 3, D is even, Ht Wt % 64 == 0 and C1, C2 are multiples of 32.
// Code object (hipcc -O3, gfx950): 74 VGPRs, 0 AGPRs, no scratch = 6 waves per SIMD by registers; 2 x 32 KB = 64 KB of dynamic LDS -> TWO workgroups per CU
// (the LDS binds; the four-point form: 76 VGPRs, 48 KB, three). tests/test_conv_igemm_resources.py holds the budget.
extern "C" int forge_wino_gemm_dn(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                                  long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream) {
    FORGE_REQUIRE(C1 > 0 && C1 % BK == 0 && C2 >= 0 && C2 % BK == 0, FORGE_EINVAL, "forge_wino_gemm_dn: C1=%d / C2=%d must be multiples of %d", C1, C2, BK);
    return wino_gemm_impl(V1, C1, ld1, bs1, pt1, V2, C2, ld2, bs2, pt2, Ud, Mm, n, D, Ht, Wt, Cout, kd, 'B', 2, stream);
}

// forge_wino_gemm through the F(4, 3) depth nest (conv_igemm_kernel<64, 128, 8, 1, 3>): the same 16 point products Mm [16][R][Cout] of a three-depth-tap problem,
// made with six K loops of C1 + C2 per group of FOUR planes instead of twelve, from the depth-combined operands V6 [16][n][D/4][6][Ht Wt][C]
// (forge_wino_input_dn4; bs1 / bs2 in rows of that layout, 0 = dense) against Ud = U'' [16][6][Cout][C1 + C2] (forge_wino_weights_dn4). Not bitwise
// forge_wino_gemm's result. FORGE_EINVAL, before any launch, unless kd == 3, D % 4 == 0, Ht Wt % 64 == 0, C1 and C2 are multiples of 32 and every
// operand and output plane stays within 32-bit buffer offsets.
// Code object (hipcc -O3, gfx950): 97 VGPRs, 0 AGPRs, no scratch = 4 waves per SIMD by registers (four accumulator sets) -> TWO workgroups per CU (tests/test_conv_igemm_resources.py);
// 2 x 24 KB = 48 KB of dynamic LDS would allow three, which needs <= 80 VGPRs (the four-point form: 76 VGPRs with three sets).
extern "C" int forge_wino_gemm_dn4(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                                   long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream) {
    FORGE_REQUIRE(C1 > 0 && C1 % BK == 0 && C2 >= 0 && C2 % BK == 0, FORGE_EINVAL, "forge_wino_gemm_dn4: C1=%d / C2=%d must be multiples of %d", C1, C2, BK);
    return wino_gemm_impl(V1, C1, ld1, bs1, pt1, V2, C2, ld2, bs2, pt2, Ud, Mm, n, D, Ht, Wt, Cout, kd, 'B', 3, stream);
}

// forge_wino_gemm_dn4 on the 24 points of F(4, 3) along H x F(2, 3) along W (the same kernel, 24 batched problems): the point products Mm [24][R][Cout],
// R = n D Ht Wt tile rows of the grid of 4 x 2 tiles (Ht = H / 4), from the operands V [24][n][D/4][6][Ht Wt][C] (forge_wino_input_dn4h) against
// Ud [24][6][Cout][C1 + C2] (forge_wino_weights_dn4h); forge_wino_output_dn4h inverts them. forge_wino_gemm_dn4's preconditions on this grid, and D >= 8.
extern "C" int forge_wino_gemm_dn4h(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                                    long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream) {
    FORGE_REQUIRE(C1 > 0 && C1 % BK == 0 && C2 >= 0 && C2 % BK == 0, FORGE_EINVAL, "forge_wino_gemm_dn4h: C1=%d / C2=%d must be multiples of %d", C1, C2, BK);
    return wino_gemm_impl(V1, C1, ld1, bs1, pt1, V2, C2, ld2, bs2, pt2, Ud, Mm, n, D, Ht, Wt, Cout, kd, 'B', 4, stream);
}

// forge_wino_gemm_dn4h on the 36 points of F(4, 3) along H AND W (the same kernel, 36 batched problems): the point products Mm [36][R][Cout], R = n D Ht Wt tile
// rows of the grid of 4 x 4 tiles (Ht = H / 4, Wt = W / 4), from the operands V [36][n][D/4][6][Ht Wt][C] (forge_wino_input_dn4hw) against Ud [36][6][Cout][C1 + C2]
// (forge_wino_weights_dn4hw); forge_wino_output_dn4hw inverts them. forge_wino_gemm_dn4h's preconditions on this grid.
extern "C" int forge_wino_gemm_dn4hw(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                                     long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream) {
    FORGE_REQUIRE(C1 > 0 && C1 % BK == 0 && C2 >= 0 && C2 % BK == 0, FORGE_EINVAL, "forge_wino_gemm_dn4hw: C1=%d / C2=%d must be multiples of %d", C1, C2, BK);
    return wino_gemm_impl(V1, C1, ld1, bs1, pt1, V2, C2, ld2, bs2, pt2, Ud, Mm, n, D, Ht, Wt, Cout, kd, 'B', 5, stream);
}
