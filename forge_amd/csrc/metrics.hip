// metrics.hip — the image metrics of the evaluation protocol (utils/eval_utils.py:compute_img_metric, kubric_eval.py:297-311): PSNR and SSIM
// (skimage's peak_signal_noise_ratio / structural_similarity as the reference calls them) and the per-tap distance of LPIPS-VGG (lpips 0.1).
// LPIPS's VGG-16 trunk runs on the convolution entries (forge_amd/perceptual.py); these kernels are the rest.
// Deterministic: no atomics; every reduction is a fixed LDS tree per workgroup into a slab, summed in a fixed order by a finalize launch.
#include "geom_common.h"

namespace forge {

constexpr int METRIC_BLOCKS = 128;       // per-image partials of forge_psnr and forge_lpips_tap
constexpr int SSIM_T = 32;               // output tile edge of forge_ssim
constexpr int SSIM_WIN = 7;
constexpr int SSIM_IN = SSIM_T + SSIM_WIN - 1;

struct ImgSrc {
    const float* p;
    long long sn, sc, sh, sw;            // element strides of the [N][C][H][W] view
};

// partial[n][blockIdx.x] = sum of (a - b)^2 over the elements of image n that workgroup (blockIdx.x, n) visits; the difference and its square in
// float64 (exact for float32 inputs up to the square's rounding), as skimage forms them
__global__ __launch_bounds__(256) void psnr_partial_kernel(const ImgSrc a, const ImgSrc b, int C, int H, int W, double* __restrict__ partial) {
    const int n = blockIdx.y;
    const long long total = (long long)C * H * W;
    const float* pa = a.p + n * a.sn;
    const float* pb = b.p + n * b.sn;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)METRIC_BLOCKS * 256) {
        const int x = (int)(i % W);
        const long long r = i / W;
        const int y = (int)(r % H);
        const int c = (int)(r / H);
        const double d = (double)pa[c * a.sc + y * a.sh + x * a.sw] - (double)pb[c * b.sc + y * b.sh + x * b.sw];
        acc = fma(d, d, acc);
    }
    __shared__ double red[256];
    const double s = block_sum256(acc, red);
    if (threadIdx.x == 0) partial[(long long)n * METRIC_BLOCKS + blockIdx.x] = s;
}

// out[n] = 10 log10(R^2 / mse), mse = (sum of image n's partials in block order) / count; mse = 0 gives +inf
__global__ void psnr_finalize_kernel(const double* __restrict__ partial, int N, double count, double range, double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int k = 0; k < METRIC_BLOCKS; ++k) s += partial[(long long)n * METRIC_BLOCKS + k];
    const double mse = s / count;
    out[n] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(range * range / mse);
}

// One workgroup per (tile, channel, image): the SSIM map of the valid 7x7 windows whose top-left corner lies in the tile's 32 x 32 outputs,
// summed. Both images' 38 x 38 inputs are staged in LDS; the five moments' horizontal 7-sums, then their vertical 7-sums, are formed in float64,
// where the products of float32 values are exact: the cancellation of u_xx - u_x^2 on flat regions costs nothing.
__global__ __launch_bounds__(256) void ssim_tile_kernel(const ImgSrc a, const ImgSrc b, int H, int W, int tiles_x, double c1, double c2,
                                                        double* __restrict__ partial) {
    __shared__ float xa[SSIM_IN][SSIM_IN + 1], xb[SSIM_IN][SSIM_IN + 1];
    __shared__ double hs[5][SSIM_IN][SSIM_T];
    __shared__ double red[256];
    const int n = blockIdx.z, c = blockIdx.y, C = gridDim.y;
    const int y0 = (blockIdx.x / tiles_x) * SSIM_T, x0 = (blockIdx.x % tiles_x) * SSIM_T;
    const int Hv = H - (SSIM_WIN - 1), Wv = W - (SSIM_WIN - 1);
    const float* pa = a.p + n * a.sn + c * a.sc;
    const float* pb = b.p + n * b.sn + c * b.sc;
    for (int i = threadIdx.x; i < SSIM_IN * SSIM_IN; i += 256) {
        const int r = i / SSIM_IN, q = i % SSIM_IN, y = y0 + r, x = x0 + q;
        const bool in = y < H && x < W;
        xa[r][q] = in ? pa[y * a.sh + x * a.sw] : 0.f;
        xb[r][q] = in ? pb[y * b.sh + x * b.sw] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SSIM_IN * SSIM_T; i += 256) {
        const int r = i / SSIM_T, q = i % SSIM_T;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const double u = xa[r][q + k], v = xb[r][q + k];
            sx += u;
            sy += v;
            sxx = fma(u, u, sxx);
            syy = fma(v, v, syy);
            sxy = fma(u, v, sxy);
        }
        hs[0][r][q] = sx;
        hs[1][r][q] = sy;
        hs[2][r][q] = sxx;
        hs[3][r][q] = syy;
        hs[4][r][q] = sxy;
    }
    __syncthreads();
    constexpr double inv_np = 1.0 / (SSIM_WIN * SSIM_WIN), cov_norm = (double)(SSIM_WIN * SSIM_WIN) / (SSIM_WIN * SSIM_WIN - 1);
    double acc = 0.0;
    for (int i = threadIdx.x; i < SSIM_T * SSIM_T; i += 256) {
        const int r = i / SSIM_T, q = i % SSIM_T;
        if (y0 + r >= Hv || x0 + q >= Wv) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k)
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] += hs[j][r + k][q];
        const double ux = m[0] * inv_np, uy = m[1] * inv_np;
        const double vx = cov_norm * (m[2] * inv_np - ux * ux), vy = cov_norm * (m[3] * inv_np - uy * uy);
        const double vxy = cov_norm * (m[4] * inv_np - ux * uy);
        acc += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }
    const double s = block_sum256(acc, red);
    if (threadIdx.x == 0) partial[((long long)n * C + c) * gridDim.x + blockIdx.x] = s;
}

// out[n] = (sum over channels, then tiles, of image n's partials) / (C (H - 6) (W - 6))
__global__ void ssim_finalize_kernel(const double* __restrict__ partial, int N, int per_image, double count, double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int k = 0; k < per_image; ++k) s += partial[(long long)n * per_image + k];
    out[n] = s / count;
}

// LPIPS distance of one tap on the channels-last activations f [2N][HW][C] (image n against image n + N): per pixel
//   d = sum_c w[c] (f0[c] / (|f0| + 1e-10) - f1[c] / (|f1| + 1e-10))^2,
// partial[n][blockIdx.x] = sum of d over the pixels workgroup (blockIdx.x, n) visits. A pixel's channels are held by LPR = min(64, C / 4) lanes
// as float4s (64 / LPR pixels per wave); the two norms and d are reduced across those lanes with xor shuffles, so every lane of a group
// holds the same sums. The difference is formed per channel: no expansion that cancels for near-identical images.
template <int C>
__global__ __launch_bounds__(256) void lpips_tap_kernel(const float* __restrict__ f, int N, int HW, const float* __restrict__ w,
                                                        double* __restrict__ partial) {
    constexpr int LPR = C / 4 < 64 ? C / 4 : 64;
    constexpr int V = C / (4 * LPR);
    constexpr int PPW = 64 / LPR;
    const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane & (LPR - 1);
    const float4* f0 = (const float4*)(f + (long long)n * HW * C);
    const float4* f1 = (const float4*)(f + (long long)(n + N) * HW * C);
    float4 wv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) wv[v] = ((const float4*)w)[v * LPR + g];
    double acc = 0.0;
    for (int base = (blockIdx.x * 4 + wave) * PPW; base < HW; base += METRIC_BLOCKS * 4 * PPW) {
        const int p = base + lane / LPR;
        const bool valid = p < HW;
        float4 a[V], b[V];
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const long long o = (long long)p * (C / 4) + v * LPR + g;
            a[v] = valid ? f0[o] : make_float4(0.f, 0.f, 0.f, 0.f);
            b[v] = valid ? f1[o] : make_float4(0.f, 0.f, 0.f, 0.f);
            s0 += a[v].x * a[v].x + a[v].y * a[v].y + a[v].z * a[v].z + a[v].w * a[v].w;
            s1 += b[v].x * b[v].x + b[v].y * b[v].y + b[v].z * b[v].z + b[v].w * b[v].w;
        }
#pragma unroll
        for (int m = LPR / 2; m > 0; m >>= 1) {
            s0 += __shfl_xor(s0, m, 64);
            s1 += __shfl_xor(s1, m, 64);
        }
        const float na = sqrtf(s0) + 1e-10f, nb = sqrtf(s1) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float ex = a[v].x / na - b[v].x / nb, ey = a[v].y / na - b[v].y / nb;
            const float ez = a[v].z / na - b[v].z / nb, ew = a[v].w / na - b[v].w / nb;
            d += wv[v].x * ex * ex + wv[v].y * ey * ey + wv[v].z * ez * ez + wv[v].w * ew * ew;
        }
#pragma unroll
        for (int m = LPR / 2; m > 0; m >>= 1) d += __shfl_xor(d, m, 64);
        if (g == 0 && valid) acc += (double)d;
    }
    __shared__ double red[256];
    const double s = block_sum256(acc, red);
    if (threadIdx.x == 0) partial[(long long)n * METRIC_BLOCKS + blockIdx.x] = s;
}

// out[n] = sum over the five taps k of (sum of partial[k][n][*] in block order) / hw[k]
__global__ void lpips_finalize_kernel(const double* __restrict__ partial, int N, int hw0, int hw1, int hw2, int hw3, int hw4, float* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int hw[5] = {hw0, hw1, hw2, hw3, hw4};
    double r = 0.0;
    for (int k = 0; k < 5; ++k) {
        double s = 0.0;
        for (int j = 0; j < METRIC_BLOCKS; ++j) s += partial[((long long)k * N + n) * METRIC_BLOCKS + j];
        r += s / hw[k];
    }
    out[n] = (float)r;
}

static int ssim_tiles(int H, int W) {
    return ((H - (SSIM_WIN - 1) + SSIM_T - 1) / SSIM_T) * ((W - (SSIM_WIN - 1) + SSIM_T - 1) / SSIM_T);
}

}  // namespace forge

using namespace forge;

extern "C" int forge_metric_blocks(void) { return METRIC_BLOCKS; }

extern "C" int forge_ssim_tiles(int H, int W) { return (H >= SSIM_WIN && W >= SSIM_WIN) ? ssim_tiles(H, W) : -1; }

extern "C" int forge_psnr(const float* a, long long a_sn, long long a_sc, long long a_sh, long long a_sw, const float* b, long long b_sn, long long b_sc,
                          long long b_sh, long long b_sw, int N, int C, int H, int W, double data_range, double* partial, double* out,
                          forge_stream_t stream) {
    FORGE_REQUIRE(a && b && partial && out, FORGE_EINVAL, "forge_psnr: null pointer argument");
    FORGE_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, FORGE_EINVAL, "forge_psnr: bad dims N=%d C=%d H=%d W=%d", N, C, H, W);
    FORGE_REQUIRE(N <= 65535, FORGE_ESHAPE, "forge_psnr: N=%d (at most 65535 images per launch)", N);
    FORGE_REQUIRE(data_range > 0.0, FORGE_EINVAL, "forge_psnr: data_range must be positive");
    const ImgSrc sa{a, a_sn, a_sc, a_sh, a_sw}, sb{b, b_sn, b_sc, b_sh, b_sw};
    hipLaunchKernelGGL(psnr_partial_kernel, dim3(METRIC_BLOCKS, N), dim3(256), 0, (hipStream_t)stream, sa, sb, C, H, W, partial);
    FORGE_LAUNCH_CHECK("forge_psnr");
    hipLaunchKernelGGL(psnr_finalize_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, partial, N, (double)C * H * W, data_range, out);
    FORGE_LAUNCH_CHECK("forge_psnr");
    return 0;
}

extern "C" int forge_ssim(const float* a, long long a_sn, long long a_sc, long long a_sh, long long a_sw, const float* b, long long b_sn, long long b_sc,
                          long long b_sh, long long b_sw, int N, int C, int H, int W, double data_range, double* partial, double* out,
                          forge_stream_t stream) {
    FORGE_REQUIRE(a && b && partial && out, FORGE_EINVAL, "forge_ssim: null pointer argument");
    FORGE_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, FORGE_EINVAL, "forge_ssim: bad dims N=%d C=%d H=%d W=%d", N, C, H, W);
    FORGE_REQUIRE(H >= SSIM_WIN && W >= SSIM_WIN, FORGE_ESHAPE, "forge_ssim: %dx%d is smaller than the 7x7 window", H, W);
    FORGE_REQUIRE(N <= 65535 && C <= 65535, FORGE_ESHAPE, "forge_ssim: N=%d C=%d (at most 65535 each per launch)", N, C);
    FORGE_REQUIRE(data_range > 0.0, FORGE_EINVAL, "forge_ssim: data_range must be positive");
    const ImgSrc sa{a, a_sn, a_sc, a_sh, a_sw}, sb{b, b_sn, b_sc, b_sh, b_sw};
    const int tiles_x = (W - (SSIM_WIN - 1) + SSIM_T - 1) / SSIM_T, tiles = ssim_tiles(H, W);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(tiles, C, N), dim3(256), 0, (hipStream_t)stream, sa, sb, H, W, tiles_x, c1, c2, partial);
    FORGE_LAUNCH_CHECK("forge_ssim");
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, partial, N, C * tiles,
                       (double)C * (H - (SSIM_WIN - 1)) * (W - (SSIM_WIN - 1)), out);
    FORGE_LAUNCH_CHECK("forge_ssim");
    return 0;
}

extern "C" int forge_lpips_tap(const float* f, int N, int HW, int C, const float* w, double* partial, forge_stream_t stream) {
    FORGE_REQUIRE(f && w && partial, FORGE_EINVAL, "forge_lpips_tap: null pointer argument");
    FORGE_REQUIRE(N > 0 && HW > 0, FORGE_EINVAL, "forge_lpips_tap: bad dims N=%d HW=%d", N, HW);
    FORGE_REQUIRE(N <= 65535, FORGE_ESHAPE, "forge_lpips_tap: N=%d (at most 65535 pairs per launch)", N);
    FORGE_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, FORGE_ESHAPE, "forge_lpips_tap: C=%d (64, 128, 256 or 512)", C);
    FORGE_REQUIRE(((unsigned long long)f % 16) == 0 && ((unsigned long long)w % 16) == 0, FORGE_ESHAPE, "forge_lpips_tap: f and w must be 16-byte aligned");
    const dim3 grid(METRIC_BLOCKS, N);
    switch (C) {
        case 64: hipLaunchKernelGGL(lpips_tap_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, f, N, HW, w, partial); break;
        case 128: hipLaunchKernelGGL(lpips_tap_kernel<128>, grid, dim3(256), 0, (hipStream_t)stream, f, N, HW, w, partial); break;
        case 256: hipLaunchKernelGGL(lpips_tap_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, f, N, HW, w, partial); break;
        default: hipLaunchKernelGGL(lpips_tap_kernel<512>, grid, dim3(256), 0, (hipStream_t)stream, f, N, HW, w, partial); break;
    }
    FORGE_LAUNCH_CHECK("forge_lpips_tap");
    return 0;
}

extern "C" int forge_lpips_finalize(const double* partial, int N, int hw0, int hw1, int hw2, int hw3, int hw4, float* out, forge_stream_t stream) {
    FORGE_REQUIRE(partial && out, FORGE_EINVAL, "forge_lpips_finalize: null pointer argument");
    FORGE_REQUIRE(N > 0 && hw0 > 0 && hw1 > 0 && hw2 > 0 && hw3 > 0 && hw4 > 0, FORGE_EINVAL, "forge_lpips_finalize: bad dims");
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, partial, N, hw0, hw1, hw2, hw3, hw4, out);
    FORGE_LAUNCH_CHECK("forge_lpips_finalize");
    return 0;
}
