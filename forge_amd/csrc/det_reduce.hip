// det_reduce.hip — the fixed-order slab reduction of the deterministic weight / pose gradients (common.h).
//
// Thread = 4 consecutive output elements: one float4 load per slab (a wave reads 1 KB contiguous rows of every slab), float64 partial
// sums in increasing slab order, one rounding to fp32, then (accumulate) exactly one fp32 add of the prior value. HBM-bound: it reads the
// slab set once and writes the output once.
#include "common.h"

namespace forge {

__global__ __launch_bounds__(256) void det_reduce_kernel(const float4* __restrict__ ws, long long nslab, long long slab4, long long outer4,
                                                          long long E4, long long total4, float4* __restrict__ out, int accumulate) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const long long o = i / E4, e = i - o * E4;
        const float4* p = ws + o * outer4 + e;
        double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
        long long s = 0;
        for (; s + 4 <= nslab; s += 4) {                 // four loads in flight, added in slab order
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = p[(s + k) * slab4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { sx += (double)v[k].x; sy += (double)v[k].y; sz += (double)v[k].z; sw += (double)v[k].w; }
        }
        for (; s < nslab; ++s) {
            const float4 v = p[s * slab4];
            sx += (double)v.x; sy += (double)v.y; sz += (double)v.z; sw += (double)v.w;
        }
        float4 r = make_float4((float)sx, (float)sy, (float)sz, (float)sw);
        if (accumulate) {
            const float4 q = out[i];
            r.x = q.x + r.x; r.y = q.y + r.y; r.z = q.z + r.z; r.w = q.w + r.w;
        }
        out[i] = r;
    }
}

int det_reduce(const float* ws, long long nslab, long long slab, long long nouter, long long outer, long long E, float* out, int accumulate,
               hipStream_t stream, const char* fn) {
    FORGE_REQUIRE(ws && out && nslab > 0 && nouter > 0 && E > 0, FORGE_EINVAL, "%s: bad slab reduction", fn);
    FORGE_REQUIRE(E % 4 == 0 && slab % 4 == 0 && outer % 4 == 0 && ((unsigned long long)ws & 15) == 0 && ((unsigned long long)out & 15) == 0,
                  FORGE_ESHAPE, "%s: slab reduction needs 16-byte aligned rows", fn);
    const long long total4 = nouter * E / 4;
    long long grid = (total4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(det_reduce_kernel, dim3((unsigned)grid), dim3(256), 0, stream, (const float4*)ws, nslab, slab / 4, outer / 4, E / 4, total4,
                       (float4*)out, accumulate);
    FORGE_LAUNCH_CHECK(fn);
    return 0;
}

}  // namespace forge
