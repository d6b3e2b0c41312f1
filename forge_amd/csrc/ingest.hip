// ingest.hip - photographs to the model's input tensors on the device (include/forge_hip.h section h): Pillow's 8-bit Lanczos resize of the colour
// image, its nearest-neighbour resize of the mask, the background modes of the reference's loaders and the division by 255, bit for bit.
//
// Two passes, because the contract has an 8-bit image between them (Pillow clips and rounds after the horizontal pass):
//   ingest_h_kernel  one source row x 256 output columns per workgroup. The row's pixels are staged in LDS in chunks of H_CHUNK: 16-byte global
//                    loads into a byte image that keeps the global address modulo 16 (rows need not be aligned), then one in-LDS pass packs
//                    each pixel to a dword, applying the composite over white / the pre-mask on the way. Every thread then walks the taps of its
//                    output column that fall into the chunk (coefficients tap-major: coalesced) and writes one packed pixel of the intermediate.
//   ingest_v_kernel  one output pixel per thread, consecutive threads along Wo: intermediate rows are read coalesced, the coefficient is
//                    uniform per output row. Epilogue: clip, the mask's nearest tap from the source, /255, the mask product, the three outputs.
// Tap counts and row lengths are unbounded: both kernels loop. No atomics, no allocation, no host synchronisation.
#include <climits>
#include <cmath>

#include "common.h"

namespace forge {
namespace {

constexpr int PRECISION_BITS = 22;
constexpr int H_THREADS = 256;   // output columns per workgroup of the horizontal pass
constexpr int H_CHUNK = 2048;    // source pixels staged per step: 8 KiB of raw bytes at 4 channels + 8 KiB of packed pixels
constexpr int V_THREADS = 256;

enum { BG_BLACK = 0, BG_WHITE = 1, BG_PREMASKED = 2 };

// ---- host: the coefficient table --------------------------------------------------------------------------------------------------------
double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

double lanczos3(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

struct Window {
    double scale, support, inv;
    Window(int n_in, int n_out) {
        scale = (double)n_in / n_out;
        const double fs = scale < 1.0 ? 1.0 : scale;
        support = 3.0 * fs;
        inv = 1.0 / fs;
    }
    double center(int i) const { return (i + 0.5) * scale; }
    void span(int i, int n_in, int& first, int& count) const {
        const double c = center(i);
        first = (int)(c - support + 0.5);
        if (first < 0) first = 0;
        int last = (int)(c + support + 0.5);
        if (last > n_in) last = n_in;
        count = last - first;
    }
    double weight(int i, int first, int j) const { return lanczos3((j + first - center(i) + 0.5) * inv); }
};

// ---- device -----------------------------------------------------------------------------------------------------------------------------
// One axis' table on the device, n = its output size, K = the row length: first[n] | count[n] | nearest[n] | k[K][n] (tap-major).
struct Table {
    const int *first, *count, *nearest, *k;
    __device__ Table(const int* t, int n) : first(t), count(t + n), nearest(t + 2 * n), k(t + 3 * (size_t)n) {}
};

// A table is the caller's: whatever it holds, no tap leaves the source (first in 0 .. n_in, count in 0 .. min(K, n_in - first)).
__device__ __forceinline__ void taps_of(const Table& t, int i, int n_in, int K, int& first, int& count) {
    first = min(max(t.first[i], 0), n_in);
    count = min(max(t.count[i], 0), min(K, n_in - first));
}

__device__ __forceinline__ unsigned over_white(unsigned c, unsigned a) {
    const unsigned t = c * a + 255u * (255u - a) + 128u;
    return (t + (t >> 8)) >> 8;
}

__device__ __forceinline__ unsigned clip8(int acc) { return (unsigned)min(max(acc >> PRECISION_BITS, 0), 255); }

template <int C>
__global__ __launch_bounds__(H_THREADS) void ingest_h_kernel(const unsigned char* __restrict__ src, long long image_stride, int row_stride, int H, int W,
                                                              int Wo, const int* __restrict__ tab, int K, int mode, unsigned* __restrict__ ws,
                                                              int ngroup) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[H_CHUNK * C + 32];
    __shared__ unsigned px[H_CHUNK];
    const int tid = threadIdx.x;
    unsigned b = blockIdx.x;
    const int group = b % ngroup;
    b /= ngroup;
    const int row = b % H, img = b / H;
    const int x = group * H_THREADS + tid;
    const bool live = x < Wo;
    const Table t(tab, Wo);
    int f = 0, c = 0;
    if (live) taps_of(t, x, W, K, f, c);
    // the workgroup's source span: first and first + count do not decrease with x
    int p_lo, p_hi, cl;
    taps_of(t, group * H_THREADS, W, K, p_lo, cl);
    taps_of(t, min(group * H_THREADS + H_THREADS, Wo) - 1, W, K, p_hi, cl);
    p_hi += cl;
    const unsigned char* rowp = src + img * image_stride + (long long)row * row_stride;
    int ar = 1 << (PRECISION_BITS - 1), ag = ar, ab = ar;
    for (int base = p_lo; base < p_hi; base += H_CHUNK) {
        const int n = min(H_CHUNK, p_hi - base);
        const unsigned char* g0 = rowp + (long long)base * C;
        const int nbytes = n * C;
        const int mis = (int)((unsigned long long)g0 & 15);   // byte i of the chunk lives at raw[mis + i]: 16-byte global words land on 16-byte LDS words
        const int head = min(nbytes, (16 - mis) & 15);
        const int nvec = (nbytes - head) >> 4;
        const int tail0 = head + (nvec << 4);
        for (int v = tid; v < nvec; v += H_THREADS)
            *reinterpret_cast<uint4*>(raw + mis + head + (v << 4)) = *reinterpret_cast<const uint4*>(g0 + head + (v << 4));
        if (tid < head) raw[mis + tid] = g0[tid];
        if (tid >= 64 && tid - 64 < nbytes - tail0) raw[mis + tail0 + tid - 64] = g0[tail0 + tid - 64];
        __syncthreads();
        for (int p = tid; p < n; p += H_THREADS) {
            const unsigned char* q = raw + mis + p * C;
            unsigned r, g, bl, a = 255;
            if (C == 4 && (mis & 3) == 0) {
                const unsigned v = *reinterpret_cast<const unsigned*>(q);
                r = v & 255, g = (v >> 8) & 255, bl = (v >> 16) & 255, a = v >> 24;
            } else {
                r = q[0], g = q[1], bl = q[2];
                if (C == 4) a = q[3];
            }
            if (C == 4 && mode == BG_WHITE) {
                r = over_white(r, a), g = over_white(g, a), bl = over_white(bl, a);
            } else if (C == 4 && mode == BG_PREMASKED && a == 0) {
                r = g = bl = 0;
            }
            px[p] = r | (g << 8) | (bl << 16);
        }
        __syncthreads();
        const int j1 = min(c, base + n - f);
        for (int j = max(0, base - f); j < j1; ++j) {
            const unsigned p = px[f + j - base];
            const int kk = t.k[(size_t)j * Wo + x];
            ar += kk * (int)(p & 255);
            ag += kk * (int)((p >> 8) & 255);
            ab += kk * (int)((p >> 16) & 255);
        }
        __syncthreads();   // the next chunk overwrites both images
    }
    if (live) ws[((long long)img * H + row) * Wo + x] = clip8(ar) | (clip8(ag) << 8) | (clip8(ab) << 16);
}

template <int C>
__global__ __launch_bounds__(V_THREADS) void ingest_v_kernel(const unsigned* __restrict__ ws, const unsigned char* __restrict__ src, long long image_stride,
                                                              int row_stride, int H, int W, int Ho, int Wo, const int* __restrict__ tab_y, int Ky,
                                                              const int* __restrict__ tab_x, int mode, float* __restrict__ images,
                                                              float* __restrict__ masks, unsigned char* __restrict__ bytes, int nblock) {
    const int img = blockIdx.x / nblock;
    const int idx = (blockIdx.x % nblock) * V_THREADS + threadIdx.x;
    if (idx >= Ho * Wo) return;
    const int y = idx / Wo, x = idx % Wo;
    const Table ty(tab_y, Ho), tx(tab_x, Wo);
    int f, c;
    taps_of(ty, y, H, Ky, f, c);
    const unsigned* col = ws + (long long)img * H * Wo + x;
    int ar = 1 << (PRECISION_BITS - 1), ag = ar, ab = ar;
    for (int j = 0; j < c; ++j) {
        const unsigned p = col[(long long)(f + j) * Wo];
        const int kk = ty.k[(size_t)j * Ho + y];
        ar += kk * (int)(p & 255);
        ag += kk * (int)((p >> 8) & 255);
        ab += kk * (int)((p >> 16) & 255);
    }
    const unsigned r = clip8(ar), g = clip8(ag), bl = clip8(ab);
    const int sy = min(max(ty.nearest[y], 0), H - 1), sx = min(max(tx.nearest[x], 0), W - 1);
    const unsigned char* q = src + img * image_stride + (long long)sy * row_stride + (long long)sx * C;
    const float m = (C == 4 ? q[3] > 0 : (q[0] > 0) | (q[1] > 0)) ? 1.f : 0.f;   // 3 channels: blue plays no part (forge_hip.h)
    const long long plane = (long long)Ho * Wo;
    if (images) {
        const float s = mode == BG_BLACK ? m : 1.f;
        float* o = images + (long long)img * 3 * plane + idx;
        o[0] = (float)r / 255.f * s;
        o[plane] = (float)g / 255.f * s;
        o[2 * plane] = (float)bl / 255.f * s;
    }
    if (masks) masks[(long long)img * plane + idx] = m;
    if (bytes) {
        unsigned char* o = bytes + ((long long)img * plane + idx) * 3;
        o[0] = (unsigned char)r, o[1] = (unsigned char)g, o[2] = (unsigned char)bl;
    }
}

template <int C>
int launch(const unsigned char* src, int N, int H, int W, long long image_stride, int row_stride, const int* tab_x, int Kx, const int* tab_y, int Ky,
           int Ho, int Wo, int mode, unsigned* ws, float* images, float* masks, unsigned char* bytes, hipStream_t stream) {
    const int ngroup = (Wo + H_THREADS - 1) / H_THREADS;
    ingest_h_kernel<C><<<dim3((unsigned)((long long)N * H * ngroup)), dim3(H_THREADS), 0, stream>>>(src, image_stride, row_stride, H, W, Wo, tab_x, Kx, mode,
                                                                                                     ws, ngroup);
    FORGE_LAUNCH_CHECK("forge_ingest_rgba8 (horizontal pass)");
    const int nblock = (Ho * Wo + V_THREADS - 1) / V_THREADS;
    ingest_v_kernel<C><<<dim3((unsigned)((long long)N * nblock)), dim3(V_THREADS), 0, stream>>>(ws, src, image_stride, row_stride, H, W, Ho, Wo, tab_y, Ky,
                                                                                                 tab_x, mode, images, masks, bytes, nblock);
    FORGE_LAUNCH_CHECK("forge_ingest_rgba8 (vertical pass)");
    return 0;
}

}  // namespace
}  // namespace forge

using namespace forge;

extern "C" int forge_resample_taps(int n_in, int n_out) {
#pragma clang fp contract(off)
    FORGE_REQUIRE(n_in > 0 && n_out > 0, FORGE_EINVAL, "forge_resample_taps: non-positive size (n_in=%d n_out=%d)", n_in, n_out);
    const Window w(n_in, n_out);
    int K = 0;
    for (int i = 0; i < n_out; ++i) {
        int first, count;
        w.span(i, n_in, first, count);
        if (count > K) K = count;
    }
    return K;
}

extern "C" int forge_resample_coeffs(int n_in, int n_out, int* first, int* count, int* k) {
#pragma clang fp contract(off)
    FORGE_REQUIRE(first && count && k, FORGE_EINVAL, "forge_resample_coeffs: null pointer");
    const int K = forge_resample_taps(n_in, n_out);
    if (K < 0) return K;
    const Window w(n_in, n_out);
    for (int i = 0; i < n_out; ++i) {
        w.span(i, n_in, first[i], count[i]);
        double sum = 0.0;
        for (int j = 0; j < count[i]; ++j) sum += w.weight(i, first[i], j);
        int* row = k + (size_t)i * K;
        for (int j = 0; j < K; ++j) {
            if (j >= count[i]) {
                row[j] = 0;
                continue;
            }
            double v = w.weight(i, first[i], j);   // evaluated twice rather than kept: nothing is allocated here
            if (sum != 0.0) v /= sum;
            row[j] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
    }
    return 0;
}

extern "C" int forge_resample_nearest(int n_in, int n_out, int* index) {
#pragma clang fp contract(off)
    FORGE_REQUIRE(n_in > 0 && n_out > 0, FORGE_EINVAL, "forge_resample_nearest: non-positive size (n_in=%d n_out=%d)", n_in, n_out);
    FORGE_REQUIRE(index, FORGE_EINVAL, "forge_resample_nearest: null pointer");
    const double s = (double)n_in / n_out;
    double p = s * 0.5;
    for (int i = 0; i < n_out; ++i) {
        const int v = (int)p;
        index[i] = v < n_in ? v : n_in - 1;
        p += s;
    }
    return 0;
}

extern "C" int forge_ingest_rgba8(const unsigned char* src, int N, int H, int W, int C, long long image_stride, long long row_stride, const int* table_x,
                                  int Kx, const int* table_y, int Ky, int Ho, int Wo, int background, void* workspace, long long workspace_bytes,
                                  float* images, float* masks, unsigned char* bytes, forge_stream_t stream) {
    FORGE_REQUIRE(src && table_x && table_y && workspace, FORGE_EINVAL, "forge_ingest_rgba8: null pointer");
    FORGE_REQUIRE(N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && Kx > 0 && Ky > 0, FORGE_EINVAL,
                  "forge_ingest_rgba8: non-positive dimension (N=%d H=%d W=%d Ho=%d Wo=%d Kx=%d Ky=%d)", N, H, W, Ho, Wo, Kx, Ky);
    FORGE_REQUIRE(C == 3 || C == 4, FORGE_EINVAL, "forge_ingest_rgba8: C=%d, need 3 or 4 channels", C);
    FORGE_REQUIRE(background >= BG_BLACK && background <= BG_PREMASKED, FORGE_EINVAL, "forge_ingest_rgba8: unknown background mode %d", background);
    FORGE_REQUIRE(row_stride >= (long long)W * C, FORGE_EINVAL, "forge_ingest_rgba8: row stride %lld below W C = %lld", row_stride, (long long)W * C);
    FORGE_REQUIRE(N == 1 || image_stride >= (H - 1) * row_stride + (long long)W * C, FORGE_EINVAL, "forge_ingest_rgba8: image stride %lld: images overlap",
                  image_stride);
    FORGE_REQUIRE(H * row_stride <= INT_MAX && (long long)H * Wo * 4 <= INT_MAX && (long long)Ho * Wo * 3 <= INT_MAX, FORGE_ESHAPE,
                  "forge_ingest_rgba8: an image (H=%d row stride=%lld) or its intermediate (H Wo = %lld pixels) exceeds 32-bit offsets", H, row_stride,
                  (long long)H * Wo);
    const long long ngroup = (Wo + H_THREADS - 1) / H_THREADS, nblock = ((long long)Ho * Wo + V_THREADS - 1) / V_THREADS;
    FORGE_REQUIRE(N * (long long)H * ngroup <= INT_MAX && N * nblock <= INT_MAX, FORGE_ESHAPE, "forge_ingest_rgba8: N=%d images of this size exceed one launch's grid",
                  N);
    FORGE_REQUIRE(workspace_bytes >= (long long)N * H * Wo * 4 && ((unsigned long long)workspace & 3) == 0, FORGE_EINVAL,
                  "forge_ingest_rgba8: workspace of %lld bytes, need %lld (4-byte aligned)", workspace_bytes, (long long)N * H * Wo * 4);
    hipStream_t s = (hipStream_t)stream;
    if (C == 4)
        return launch<4>(src, N, H, W, image_stride, (int)row_stride, table_x, Kx, table_y, Ky, Ho, Wo, background, (unsigned*)workspace, images, masks, bytes, s);
    return launch<3>(src, N, H, W, image_stride, (int)row_stride, table_x, Kx, table_y, Ky, Ho, Wo, background, (unsigned*)workspace, images, masks, bytes, s);
}
