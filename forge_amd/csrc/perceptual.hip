// perceptual.hip — the glue of the VGG-16 perceptual loss (models/perceptual_loss.py:23-44) around the convolution kernels: image
// preparation (channel repeat, normalisation, bilinear resize to 224^2, conv1_1's patch rows) and its adjoint, the per-tap L1 partial sums,
// and the fused block-boundary backward (max-pool backward + L1 gradient + ReLU mask). The ten 3x3 convolutions, the max-pool forward and
// the ReLU masks inside a block run on the existing entries (conv_igemm / winograd / stem / bnorm).
// Deterministic: no atomics anywhere; reductions are fixed-tree per-workgroup partial sums the caller adds in a fixed order.
#include "common.h"

namespace forge {

constexpr int PREP_K = 27, PREP_KPAD = 32;     // conv1_1: 3x3 taps x 3 channels, padded to the GEMM's 32-wide K-step
constexpr int L1_BLOCKS = 1024;

struct PrepSrc {
    const float* p;
    long long sn, sc, sh, sw;                  // element strides of the [N][C][H][W] view
};

// normalised, resized value of channel c (0..2) at output pixel (Y, X) of image n: ((v - mean[c]) / std[c]) of the source channel
// (c, or 0 when C = 1: the repeat), then ATen's bilinear interpolation (align_corners = False) when `resize`
__device__ __forceinline__ float prep_value(const PrepSrc& s, int n, int c, int C, int Y, int X, int Hi, int Wi, float sh, float sw, int resize,
                                            float mu, float sd) {
    const float* base = s.p + n * s.sn + (C == 1 ? 0 : c) * s.sc;
    if (!resize) return (base[Y * s.sh + X * s.sw] - mu) / sd;
    int h1, hp, w1, wp;
    float h0l, h1l, w0l, w1l;
    bilinear_src(Y, sh, Hi, h1, hp, h0l, h1l);
    bilinear_src(X, sw, Wi, w1, wp, w0l, w1l);
    const float v00 = (base[h1 * s.sh + w1 * s.sw] - mu) / sd, v01 = (base[h1 * s.sh + (w1 + wp) * s.sw] - mu) / sd;
    const float v10 = (base[(h1 + hp) * s.sh + w1 * s.sw] - mu) / sd, v11 = (base[(h1 + hp) * s.sh + (w1 + wp) * s.sw] - mu) / sd;
    return h0l * (w0l * v00 + w1l * v01) + h1l * (w0l * v10 + w1l * v11);
}

// rows [(N or 2N) Ho Wo][32]: row = (image, oy, ox), k = (ky * 3 + kx) * 3 + c (forge_im2col_nchw's order), zero outside the image and for k >= 27.
// Images 0..N-1 come from a, N..2N-1 from b.
__global__ __launch_bounds__(256) void vgg_prep_fwd_kernel(const PrepSrc a, const PrepSrc b, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           float* __restrict__ rows, int N, int nimg, int C, int Hi, int Wi, int Ho, int Wo, int resize,
                                                           float sh, float sw) {
    const long long total = (long long)nimg * Ho * Wo * PREP_KPAD;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int k = (int)(i & (PREP_KPAD - 1));
        long long r = i / PREP_KPAD;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int img = (int)(r / Ho);
        float v = 0.f;
        if (k < PREP_K) {
            const int c = k % 3, t = k / 3, kx = t % 3, ky = t / 3;
            const int y = oy - 1 + ky, x = ox - 1 + kx;
            if ((unsigned)y < (unsigned)Ho && (unsigned)x < (unsigned)Wo)
                v = img < N ? prep_value(a, img, c, C, y, x, Hi, Wi, sh, sw, resize, mean[c], stdv[c])
                            : prep_value(b, img - N, c, C, y, x, Hi, Wi, sh, sw, resize, mean[c], stdv[c]);
        }
        rows[i] = v;
    }
}

// adjoint of the preparation, one thread per INPUT element (n, c, y, x): gather of the resize adjoint over the output pixels that reference
// source pixel (y, x) (render.hip's resize_bilinear_bwd_kernel bounds), divided by std, summed over the three repeated channels when C = 1.
// g: the data gradient of the prepared image, channels-last [N][Ho][Wo][ldg] (channel c at column c).
__global__ __launch_bounds__(256) void vgg_prep_bwd_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ stdv, float* __restrict__ din,
                                                           long long sn, long long sc, long long sh_, long long sw_, int N, int C, int Hi, int Wi, int Ho,
                                                           int Wo, int resize, float sh, float sw) {
    const long long total = (long long)N * C * Hi * Wi;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % Wi);
        long long r = i / Wi;
        const int y = (int)(r % Hi); r /= Hi;
        const int cin = (int)(r % C);
        const int n = (int)(r / C);
        const float* gp = g + (long long)n * Ho * Wo * ldg;
        float res = 0.f;
        for (int c = (C == 1 ? 0 : cin); c < (C == 1 ? 3 : cin + 1); ++c) {
            float acc = 0.f;
            if (!resize) {
                acc = gp[((long long)y * Wo + x) * ldg + c];
            } else {
                const int Y0 = max(0, (int)ceilf(((float)y - 0.5f) / sh - 0.5f) - 1), Y1 = min(Ho - 1, (int)floorf(((float)y + 1.5f) / sh - 0.5f) + 1);
                const int X0 = max(0, (int)ceilf(((float)x - 0.5f) / sw - 0.5f) - 1), X1 = min(Wo - 1, (int)floorf(((float)x + 1.5f) / sw - 0.5f) + 1);
                for (int Y = Y0; Y <= Y1; ++Y) {
                    int h1, hp; float h0l, h1l;
                    bilinear_src(Y, sh, Hi, h1, hp, h0l, h1l);
                    const float wy = (h1 == y ? h0l : 0.f) + (h1 + hp == y ? h1l : 0.f);
                    if (wy == 0.f) continue;
                    for (int X = X0; X <= X1; ++X) {
                        int w1, wp; float w0l, w1l;
                        bilinear_src(X, sw, Wi, w1, wp, w0l, w1l);
                        const float wx = (w1 == x ? w0l : 0.f) + (w1 + wp == x ? w1l : 0.f);
                        if (wx != 0.f) acc = fmaf(wy * wx, gp[((long long)Y * Wo + X) * ldg + c], acc);
                    }
                }
            }
            res += acc / stdv[c];
        }
        din[n * sn + cin * sc + y * sh_ + x * sw_] = res;
    }
}

// partial[b] = sum |x - y| over the elements workgroup b visits (grid-stride, float4), fixed LDS tree
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, long long n, float* __restrict__ partial) {
    float acc = 0.f;
    const long long n4 = n / 4;
    const float4* x4 = (const float4*)x;
    const float4* y4 = (const float4*)y;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 a = x4[i], b = y4[i];
        acc += fabsf(a.x - b.x) + fabsf(a.y - b.y) + fabsf(a.z - b.z) + fabsf(a.w - b.w);
    }
    for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) acc += fabsf(x[i] - y[i]);
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// d_pre[m][c] = (maxpool2x2_bwd(g_next) + coef sign(x - y)) * (x > 0) on channels-last rows [N][H][W][C]; x post-ReLU. The pool backward
// recomputes each 2x2 window's winner from x with ATen's rule (scan in row-major order, `v > max || isnan(v)` takes over, first element
// initially). g_next [N][H/2][W/2][C] and coef (a device scalar) are nullable.
__global__ __launch_bounds__(256) void vgg_tap_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g_next,
                                                          const float* __restrict__ coef, float* __restrict__ dpre, int N, int H, int W, int C) {
    const long long total = (long long)N * H * W * C;
    const int Hp = H / 2, Wp = W / 2;
    const float cf = coef ? coef[0] : 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long long r = i / C;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H);
        const int n = (int)(r / H);
        const float xv = x[i];
        float v = 0.f;
        if (g_next && (h >> 1) < Hp && (w >> 1) < Wp) {
            const int h0 = h & ~1, w0 = w & ~1;
            const float* xb = x + (((long long)n * H + h0) * W + w0) * C + c;
            float m = xb[0];
            int win = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const float u = xb[((long long)(k >> 1) * W + (k & 1)) * C];
                if (u > m || isnan(u)) { m = u; win = k; }
            }
            if (win == ((h - h0) << 1) + (w - w0)) v = g_next[(((long long)n * Hp + (h >> 1)) * Wp + (w >> 1)) * C + c];
        }
        if (coef) {
            const float d = xv - y[i];
            v += cf * (float)((d > 0.f) - (d < 0.f));
        }
        dpre[i] = xv > 0.f ? v : 0.f;
    }
}

static unsigned stream_grid(long long total) {
    const long long g = (total + 255) / 256;
    return (unsigned)(g < 256 * 64 ? (g > 0 ? g : 1) : 256 * 64);
}

}  // namespace forge

using namespace forge;

extern "C" int forge_vgg_prep_fwd(const float* a, long long a_sn, long long a_sc, long long a_sh, long long a_sw, const float* b, long long b_sn,
                                  long long b_sc, long long b_sh, long long b_sw, const float* mean, const float* stdv, float* rows, int N, int C, int Hi,
                                  int Wi, int Ho, int Wo, int resize, forge_stream_t stream) {
    FORGE_REQUIRE(a && mean && stdv && rows, FORGE_EINVAL, "forge_vgg_prep_fwd: null pointer argument");
    FORGE_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && (resize == 0 || resize == 1), FORGE_EINVAL, "forge_vgg_prep_fwd: bad dims");
    FORGE_REQUIRE(C == 1 || C == 3, FORGE_ESHAPE, "forge_vgg_prep_fwd: C=%d (1 or 3 channels)", C);
    FORGE_REQUIRE(resize || (Ho == Hi && Wo == Wi), FORGE_ESHAPE, "forge_vgg_prep_fwd: without resize the output is the input's size");
    const PrepSrc sa{a, a_sn, a_sc, a_sh, a_sw}, sb{b ? b : a, b_sn, b_sc, b_sh, b_sw};
    const int nimg = b ? 2 * N : N;
    hipLaunchKernelGGL(vgg_prep_fwd_kernel, dim3(stream_grid((long long)nimg * Ho * Wo * PREP_KPAD)), dim3(256), 0, (hipStream_t)stream, sa, sb, mean, stdv,
                       rows, N, nimg, C, Hi, Wi, Ho, Wo, resize, (float)Hi / (float)Ho, (float)Wi / (float)Wo);
    FORGE_LAUNCH_CHECK("forge_vgg_prep_fwd");
    return 0;
}

extern "C" int forge_vgg_prep_bwd(const float* g, int ldg, const float* stdv, float* din, long long sn, long long sc, long long sh, long long sw, int N,
                                  int C, int Hi, int Wi, int Ho, int Wo, int resize, forge_stream_t stream) {
    FORGE_REQUIRE(g && stdv && din, FORGE_EINVAL, "forge_vgg_prep_bwd: null pointer argument");
    FORGE_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && ldg >= 3 && (resize == 0 || resize == 1), FORGE_EINVAL, "forge_vgg_prep_bwd: bad dims");
    FORGE_REQUIRE(C == 1 || C == 3, FORGE_ESHAPE, "forge_vgg_prep_bwd: C=%d (1 or 3 channels)", C);
    FORGE_REQUIRE(resize || (Ho == Hi && Wo == Wi), FORGE_ESHAPE, "forge_vgg_prep_bwd: without resize the output is the input's size");
    hipLaunchKernelGGL(vgg_prep_bwd_kernel, dim3(stream_grid((long long)N * C * Hi * Wi)), dim3(256), 0, (hipStream_t)stream, g, ldg, stdv, din, sn, sc, sh,
                       sw, N, C, Hi, Wi, Ho, Wo, resize, (float)Hi / (float)Ho, (float)Wi / (float)Wo);
    FORGE_LAUNCH_CHECK("forge_vgg_prep_bwd");
    return 0;
}

extern "C" int forge_l1_partial_blocks(void) { return L1_BLOCKS; }

extern "C" int forge_l1_partial(const float* x, const float* y, long long n, float* partial, forge_stream_t stream) {
    FORGE_REQUIRE(x && y && partial, FORGE_EINVAL, "forge_l1_partial: null pointer argument");
    FORGE_REQUIRE(n > 0, FORGE_EINVAL, "forge_l1_partial: n=%lld", n);
    FORGE_REQUIRE(((unsigned long long)x % 16) == 0 && ((unsigned long long)y % 16) == 0, FORGE_ESHAPE, "forge_l1_partial: x and y must be 16-byte aligned");
    hipLaunchKernelGGL(l1_partial_kernel, dim3(L1_BLOCKS), dim3(256), 0, (hipStream_t)stream, x, y, n, partial);
    FORGE_LAUNCH_CHECK("forge_l1_partial");
    return 0;
}

extern "C" int forge_vgg_tap_bwd(const float* x, const float* y, const float* g_next, const float* coef, float* d_pre, int N, int H, int W, int C,
                                 forge_stream_t stream) {
    FORGE_REQUIRE(x && d_pre && (coef == nullptr || y), FORGE_EINVAL, "forge_vgg_tap_bwd: null pointer argument (y is needed with coef)");
    FORGE_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, FORGE_EINVAL, "forge_vgg_tap_bwd: bad dims");
    FORGE_REQUIRE(g_next == nullptr || (H >= 2 && W >= 2), FORGE_ESHAPE, "forge_vgg_tap_bwd: a 2x2 pool needs H, W >= 2");
    hipLaunchKernelGGL(vgg_tap_bwd_kernel, dim3(stream_grid((long long)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, x, y, g_next, coef, d_pre, N, H, W,
                       C);
    FORGE_LAUNCH_CHECK("forge_vgg_tap_bwd");
    return 0;
}
