// geom_common.h — what mesh.hip, bake.hip, geomdist.hip, tridist.hip, winding.hip, components.hip, align.hip and metrics.hip share, written once
// (header only: no translation unit; the one function it merely declares, stage_triangles, lives beside its kernel in tridist.hip).
//   wave / block primitives   wave_inclusive_scan, wave_sum, waves_before, block_exclusive_scan_inplace (integer scans: any order gives the same bits)
//   row spans                 row_span, mesh_spans: the rows of a padded or packed mesh array that one volume owns (forge_hip.h sections g1, g2, g3)
//   mesh rows                 MeshRows, mesh_rows, face_area, face_normal, clamp_count, apply_xf: what geomdist.hip and tridist.hip read a mesh and a pair by
//   triangle records          TRI_REC, TRI_TILE, stage_triangles: the staged face records tridist.hip and winding.hip search (defined in tridist.hip)
//   fixed-tree reductions     block_reduce256 / block_sum256 / block_max256: float64, ONE tree, so every caller keeps its bits
//   host side                 ws_align, ws_layout, volume_dims_ok, workspace_ok, level_ok: the argument checks of the workspace entry points
#pragma once
#include <cmath>

#include "common.h"

namespace forge {

// ------------------------------------------------------------------------------------------------------------------ wave and block primitives
// inclusive scan over the lanes of a wave64: the shuffle-up ladder
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// sum over the lanes of a wave64, valid in lane 0: the shuffle-down ladder
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// start + the totals of the waves before `wave` (wsum[w] = total of wave w, in LDS, complete)
template <class T>
__device__ __forceinline__ T waves_before(const T* wsum, int wave, T start) {
    for (int w = 0; w < wave; ++w) start += wsum[w];
    return start;
}

// p[0..n) -> its exclusive scan in place, by one workgroup of THREADS threads: chunks of THREADS elements with a running carry through LDS.
// Every thread of the workgroup must call it; every thread gets the total.
template <class T, int THREADS>
__device__ __forceinline__ T block_exclusive_scan_inplace(T* p, int n) {
    __shared__ T wsum[THREADS / 64];
    __shared__ T carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T carry = 0;
    for (int base = 0; base < n; base += THREADS) {
        const int i = base + tid;
        const T own = i < n ? p[i] : T(0);
        const T v = wave_inclusive_scan(own, lane);
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        const T before = waves_before(wsum, wave, carry);
        if (i < n) p[i] = before + v - own;
        if (tid == THREADS - 1) carry_s = before + v;
        __syncthreads();
        carry = carry_s;
    }
    return carry;
}

// ------------------------------------------------------------------------------------------------------------------------------- row spans
// The rows of a mesh array (vertices: col 0, faces: col 1) that volume `vol` owns: rows row0 .. row0 + room - 1.
//   offsets == nullptr (padded): every volume owns max_rows rows, volume v from row v max_rows;
//   offsets != nullptr (packed): the array has max_rows rows in all and volume v starts at offsets[v][col]; room is what is left from there
//   (not positive when the volume starts at or past the end). A NEGATIVE offset is never followed: room 0, the volume touches nothing.
struct RowSpan {
    long long row0, room;
};

__device__ __forceinline__ RowSpan row_span(const int* __restrict__ offsets, int vol, int col, long long max_rows) {
    if (offsets == nullptr) return {(long long)vol * max_rows, max_rows};
    const long long row0 = offsets[2 * vol + col];
    return {row0, row0 < 0 ? 0ll : max_rows - row0};
}

// Both spans of a mesh (vertex rows, face rows). A negative offset of EITHER array empties both: the volume touches no row of any array.
struct MeshSpans {
    RowSpan v, f;
};

__device__ __forceinline__ MeshSpans mesh_spans(const int* __restrict__ offsets, int vol, long long max_vertices, long long max_faces) {
    MeshSpans s = {row_span(offsets, vol, 0, max_vertices), row_span(offsets, vol, 1, max_faces)};
    if (s.v.row0 < 0 || s.f.row0 < 0) s.v.room = s.f.room = 0;
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------------ mesh rows
// The mesh arguments of forge_surface_sample and forge_nn_triangles (section g3), as the kernels take them.
struct MeshRows {
    const float* vertices;
    const int* faces;
    const int* counts;
    const int* offsets;
    int max_vertices, max_faces;                   // per mesh (offsets == nullptr) or in all (packed)
};

// rows of mesh v: first vertex / face row and how many of each are valid (a mesh that overflowed its capacity keeps the prefix that fitted)
__device__ __forceinline__ void mesh_rows(const MeshRows& m, int v, long long& v0, long long& f0, int& nv, int& nf) {
    const MeshSpans s = mesh_spans(m.offsets, v, m.max_vertices, m.max_faces);      // a negative offset of either array: the mesh is never followed
    v0 = s.v.row0;
    f0 = s.f.row0;
    nv = (int)max(min((long long)m.counts[2 * v], s.v.room), 0ll);
    nf = (int)max(min((long long)m.counts[2 * v + 1], s.f.room), 0ll);
}

// A_f in float64 from the fp32 corners: 0.5 |cross(b - a, c - a)|; 0 for a face with an index outside 0 .. nv - 1
__device__ __forceinline__ double face_area(const float* __restrict__ vert, const int* __restrict__ face, int nv) {
    const int ia = face[0], ib = face[1], ic = face[2];
    if ((unsigned)ia >= (unsigned)nv || (unsigned)ib >= (unsigned)nv || (unsigned)ic >= (unsigned)nv) return 0.0;
    const double ax = vert[3ll * ia], ay = vert[3ll * ia + 1], az = vert[3ll * ia + 2];
    const double e1x = (double)vert[3ll * ib] - ax, e1y = (double)vert[3ll * ib + 1] - ay, e1z = (double)vert[3ll * ib + 2] - az;
    const double e2x = (double)vert[3ll * ic] - ax, e2y = (double)vert[3ll * ic + 1] - ay, e2z = (double)vert[3ll * ic + 2] - az;
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

// n = normalize(cross(e1, e2)) in fp32, e1 = b - a, e2 = c - a: the face normal along the winding; n is left as it is (zero) when the cross product is zero
__device__ __forceinline__ void face_normal(float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float& nx, float& ny, float& nz) {
    const float cx = fmaf(e1y, e2z, -(e1z * e2y)), cy = fmaf(e1z, e2x, -(e1x * e2z)), cz = fmaf(e1x, e2y, -(e1y * e2x));
    const float len = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    if (len > 0.f) {
        nx = cx / len;
        ny = cy / len;
        nz = cz / len;
    }
}

// a valid-row count of a pair: count[b] clamped into 0 .. N, N without counts
__device__ __forceinline__ int clamp_count(const int* __restrict__ count, int b, int N) { return count != nullptr ? min(max(count[b], 0), N) : N; }

// row-major 3x4 (s R | t) applied to a point in place: the ONE fma chain of section g3's transforms
__device__ __forceinline__ void apply_xf(const float* __restrict__ m, float& x, float& y, float& z) {
    const float x0 = x, y0 = y, z0 = z;
    x = fmaf(m[2], z0, fmaf(m[1], y0, fmaf(m[0], x0, m[3])));
    y = fmaf(m[6], z0, fmaf(m[5], y0, fmaf(m[4], x0, m[7])));
    z = fmaf(m[10], z0, fmaf(m[9], y0, fmaf(m[8], x0, m[11])));
}

// ------------------------------------------------------------------------------------------------------------------------ triangle records
// What tridist.hip stages and tridist.hip and winding.hip search (section g3b: the workspace): one record of TRI_REC floats per face row,
// ax ay az bx | by bz cx cy | cz nx ny nz (three float4), all NaN for a face that is no candidate; walked in LDS tiles of TRI_TILE records.
constexpr int TRI_REC = 12;
constexpr int TRI_TILE = 256;                      // forge_nn_tile_faces()

// tridist.hip's staging launch (tri_stage_kernel) on `stream`: the records of every face row of the B meshes of m into rec, xf_mesh (nullable)
// applied to the corners. No launch without face rows. Returns 0 or the launch's error, reported under the entry's name fn.
int stage_triangles(const MeshRows& m, const float* xf_mesh, float4* rec, int B, hipStream_t stream, const char* fn);

// ------------------------------------------------------------------------------------------------------------------ fixed-tree reductions
// One double per thread of a 256-thread workgroup, combined by the fixed tree red[t] = op(red[t], red[t + s]), s = 128 .. 1; valid in thread 0.
// A caller that reduces several values through the same `red` back to back puts a __syncthreads() before each (geomdist.hip does).
template <class Op>
__device__ __forceinline__ double block_reduce256(double v, double* red, Op op) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double block_sum256(double v, double* red) {
    return block_reduce256(v, red, [](double a, double b) { return a + b; });
}

__device__ __forceinline__ double block_max256(double v, double* red) {
    return block_reduce256(v, red, [](double a, double b) { return fmax(a, b); });
}

// ------------------------------------------------------------------------------------------------------------------------------ host side
inline long long ws_align(long long b) { return (b + 255) & ~255ll; }

// off[0] = 0, off[k + 1] = off[k] + ws_align(bytes[k]): the sections of a workspace, each 256-byte aligned; off[N] is the size
template <int N>
inline void ws_layout(const long long (&bytes)[N], long long (&off)[N + 1]) {
    off[0] = 0;
    for (int k = 0; k < N; ++k) off[k + 1] = off[k] + ws_align(bytes[k]);
}

// what every volume entry point requires: positive extents, at most max_points grid points (D + pad)(H + pad)(W + pad) per volume (the caller's
// own bound: its indices are 32-bit; max_points <= 2^31, so no product here overflows), at most 65535 volumes (the grid's y extent)
inline int volume_dims_ok(const char* fn, int n, int D, int H, int W, int pad, long long max_points) {
    FORGE_REQUIRE(n >= 1 && D >= 1 && H >= 1 && W >= 1, FORGE_EINVAL, "%s: n=%d D=%d H=%d W=%d must be positive", fn, n, D, H, W);
    const long long hw = ((long long)H + pad) * ((long long)W + pad);
    FORGE_REQUIRE(hw <= max_points && ((long long)D + pad) * hw <= max_points, FORGE_ESHAPE,
                  "%s: D H W = %d x %d x %d: per-volume indices are 32-bit (at most %lld grid points of (D+%d)(H+%d)(W+%d))", fn, D, H, W, max_points, pad, pad,
                  pad);
    FORGE_REQUIRE(n <= 65535, FORGE_ESHAPE, "%s: n=%d volumes in one call (at most 65535)", fn, n);
    return 0;
}

inline int workspace_ok(const char* fn, const void* workspace, long long bytes, long long need) {
    FORGE_REQUIRE(bytes >= need, FORGE_EINVAL, "%s: workspace of %lld bytes, %lld needed", fn, bytes, need);
    FORGE_REQUIRE(((unsigned long long)workspace & 15ull) == 0, FORGE_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    return 0;
}

// a level the zero shell lies strictly below
inline bool level_ok(float level) { return level > 0.f && std::isfinite(level); }

}  // namespace forge
