// common.h — shared host/device helpers for libforge_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "../../include/forge_hip.h"

namespace forge {

void set_error(const char* fmt, ...);

#define FORGE_REQUIRE(cond, code, ...)            \
    do {                                          \
        if (!(cond)) {                            \
            ::forge::set_error(__VA_ARGS__);      \
            return (code);                        \
        }                                         \
    } while (0)

#define FORGE_LAUNCH_CHECK(what)                                                        \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            ::forge::set_error("%s: launch failed: %s", what, hipGetErrorString(e_));   \
            return (int)e_;                                                             \
        }                                                                               \
    } while (0)

// Raise a kernel's dynamic-LDS limit once PER DEVICE (the attribute is per device; a process may drive several GPUs). hipGetDevice
// and the attribute call touch no stream, so this is safe under stream capture.
#define FORGE_SET_MAX_LDS_ONCE(kernel_ptr, bytes)                                                                      \
    do {                                                                                                               \
        static bool done_[64] = {};                                                                                    \
        int dev_ = 0;                                                                                                  \
        (void)hipGetDevice(&dev_);                                                                                     \
        if (dev_ >= 0 && dev_ < 64 && !done_[dev_]) {                                                                  \
            (void)hipFuncSetAttribute((const void*)(kernel_ptr), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
            done_[dev_] = true;                                                                                        \
        }                                                                                                              \
    } while (0)

constexpr int NUM_XCD = 8;   // MI355X: 8 XCDs, workgroup b is dispatched to XCD b % 8

// Bijective remap of a linear workgroup id so that each XCD (private 4 MiB L2) gets one
// CONTIGUOUS chunk of the logical grid instead of every 8th workgroup. Speed only — results
// never depend on placement.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg) {
    const unsigned q = nwg / NUM_XCD, r = nwg % NUM_XCD;
    const unsigned xcd = bid % NUM_XCD, k = bid / NUM_XCD;
    const unsigned base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}

// ATen's source index / weights of a bilinear resize with align_corners = False (area_pixel_compute_source_index + upsample_bilinear2d_out_frame):
//   src = max(scale (dst + 0.5) - 0.5, 0), scale = in / out;  i1 = (int)src, ip = i1 < in - 1, l1 = src - i1, l0 = 1 - l1
__device__ __forceinline__ void bilinear_src(int dst, float scale, int n_in, int& i1, int& ip, float& l0, float& l1) {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i1 = (int)src;
    ip = (i1 < n_in - 1) ? 1 : 0;
    l1 = src - (float)i1;
    l0 = 1.f - l1;
}

__device__ __forceinline__ float4 f4_fma(float w, float4 v, float4 a) {
    a.x = fmaf(w, v.x, a.x);
    a.y = fmaf(w, v.y, a.y);
    a.z = fmaf(w, v.z, a.z);
    a.w = fmaf(w, v.w, a.w);
    return a;
}

// Deterministic mode (the *_det entry points): kernels that would add partial sums with fp32 atomics store them into slabs of the caller's
// workspace instead, and det_reduce sums the slabs in slab order:
//   out[o][e] = (accumulate ? out[o][e] : 0) + S,  S = sum_{s = 0..nslab-1} ws[o outer + s slab + e]  (float64, in s order, rounded once)
// e < E; E, slab and outer multiples of 4 floats, ws / out 16-byte aligned. DET_SLAB_BYTES caps one launch's slab set (a plan rule on shapes).
constexpr long long DET_SLAB_BYTES = 64ll << 20;
int det_reduce(const float* ws, long long nslab, long long slab, long long nouter, long long outer, long long E, float* out, int accumulate,
               hipStream_t stream, const char* fn);

// hardware fp32 atomic add (global_atomic_add_f32), no CAS loop
__device__ __forceinline__ void atomic_add_f32(float* p, float v) { unsafeAtomicAdd(p, v); }

// ---- LDS-DMA (gfx950): global memory -> LDS without staging registers -------------------------------------------------------------
// lds_dma16(rsrc, voff, lds): `buffer_load_dwordx4 v, s[rsrc], 0 offen lds` with M0 = lds. Every lane of the wave loads the 16 bytes at
// buffer byte offset voff[lane] and the hardware writes them to LDS byte address lds + 16 lane (lds must be wave-uniform); lanes whose
// offset lies outside the buffer's num_records write zeros (the halo / ragged-edge padding of every GEMM here). It is inline assembly
// on purpose: the compiler's waitcnt insertion does not see these loads, so the K loops place their own `s_waitcnt vmcnt(0)` directly
// in front of the barrier that publishes the stage, AFTER the step's MFMAs (the builtin form is drained before them). M0 is declared
// clobbered: the compiler must not keep a live M0 value (LDS / movrel / readlane uses) across the statement.
typedef int forge_v4i32 __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(16))) float f32x16;   // accumulator of the 32x32 fp32 MFMA

constexpr int RSRC_RAW_DWORD = 0x00020000;  // descriptor word 3 of a raw dword buffer, stride 0
constexpr unsigned OOB = 0x80000000u;      // byte offset beyond any buffer (< 2 GiB spans enforced on the host side): such a lane of an LDS-DMA load
                                           // lands as zeros - the zero padding of out-of-grid taps and of rows / columns beyond M / Cout costs neither
                                           // a branch nor a select

__device__ __forceinline__ forge_v4i32 make_rsrc_words(const void* base, long long bytes) {
    const unsigned long long p = (unsigned long long)base;
    forge_v4i32 r;
    // readfirstlane: the words must live in SGPRs (an "s" operand of the inline assembly) even where the compiler cannot prove the base uniform
    r.x = __builtin_amdgcn_readfirstlane((int)(p & 0xffffffffull)); r.y = __builtin_amdgcn_readfirstlane((int)((p >> 32) & 0xffffull));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes); r.w = RSRC_RAW_DWORD;
    return r;
}

// The same descriptor in the form the compiler's raw-buffer builtins take (their loads and stores are visible to its waitcnt insertion).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, RSRC_RAW_DWORD);
}

__device__ __forceinline__ float4 buf_load16(__amdgpu_buffer_rsrc_t r, unsigned off) {          // 16 bytes at byte offset off; zeros beyond the buffer
    typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4;
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    float4 f;
    __builtin_memcpy(&f, &v, 16);
    return f;
}

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"       // "clobber list contains reserved registers: m0" - the clobber is the point (see above)
__device__ __forceinline__ void lds_dma16(const forge_v4i32& rsrc, unsigned voff, unsigned lds) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds), "v"(voff), "s"(rsrc) : "memory", "m0");
}
#pragma clang diagnostic pop

__device__ __forceinline__ void lds_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// lds_dma_wait + barrier as ONE statement, for a K loop that also has ordinary stores in flight: the wave's LDS-DMA loads and stores have
// completed and its own LDS reads have returned, then s_barrier - nothing is scheduled between the wait and the barrier.
__device__ __forceinline__ void lds_dma_wait_barrier() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ unsigned lds_addr(const void* smem_ptr) {                             // LDS byte address of a __shared__ pointer
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const char*)smem_ptr;
}

}  // namespace forge
