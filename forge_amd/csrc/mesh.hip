// mesh.hip — triangle-mesh extraction from density volumes: marching tetrahedra on the Kuhn 6-tetrahedron split of every cell
// (include/forge_hip.h section g1 states the contract: grid points -1..N with a virtual zero shell, strict d > level, one welded vertex per
// active edge owned by the cell at the edge's min corner, a specified output order).
//
// Four kinds of launch, no atomics anywhere, every output index a pure function of the input (bitwise reproducible):
//   mesh_classify  one thread per cell of the (D+1)(H+1)(W+1) padded grid: 8 corner samples (shell by predication), the packed cell record,
//                  and the workgroup's vertex / triangle sums (wave64 shuffles, then LDS) -> one partial per 256 cells
//   mesh_scan      one workgroup per volume: exclusive scan of the partials in chunks of 1024 with a running carry; writes counts[n][2]
//   mesh_apply     per cell exclusive offsets = partial offset + workgroup scan of the cell counts
//   mesh_vertices / mesh_faces   one thread per cell; a cell without owned active edges / without triangles (the vast majority) leaves at once
// Resource use (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   mesh_classify 19 VGPR, 16 B LDS; mesh_scan 34 VGPR, 136 B LDS; mesh_apply 16 VGPR, 16 B LDS; mesh_vertices<false> 36 VGPR, <true> 40 VGPR, no LDS;
//   mesh_faces 57 VGPR, no LDS. No scratch in any of them; every kernel is at 8 waves per SIMD.
// Traffic at 129^3 cells: classify reads the density once (the 8 corner loads of neighbouring threads hit L1 / L2) and writes the 4-byte record
// of each cell (it shares an 8-byte slot with the vertex offset); apply reads the record and writes the two offsets of the cells that emit;
// vertex emission reads the slot, face emission the record, and after that only the surface's neighbourhood.
#include "geom_common.h"

namespace forge {

// ---- the case table: data in ONE place (forge_mesh_case_table copies it out; tests/mesh_cases.py restates the contract from that copy) ----
// Cell corner code c: bit 0 = +x (W), bit 1 = +y (H), bit 2 = +z (D). Edge direction k = 0..6 is the offset code k + 1.
// Tetrahedron q = 0..5 is the Kuhn path p0, p0 + e_a, p0 + e_a + e_b, p0 + (1,1,1) over the permutations (a, b, c) of (x, y, z) in
// lexicographic order; MESH_TET_FLIP is 1 where that path is negatively oriented (an odd permutation): its triangles swap their last two vertices.
// A tetrahedron's local corners 0 < 1 < 2 < 3 are nested offset codes, so its edge (i, j), i < j, is owned by cell + corner i with direction
// code corner j ^ corner i. MESH_CASE_TRI is written for a positively oriented tetrahedron; case = sum of 2^i over the INSIDE local corners;
// each triangle names three tetrahedron edges and is counter-clockwise seen from the outside (low-density) corners.
constexpr int MESH_TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
constexpr int MESH_TET_FLIP[6] = {0, 1, 1, 0, 0, 1};
constexpr int MESH_TET_EDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
constexpr int MESH_CASE_NTRI[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
constexpr int MESH_CASE_TRI[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}},   // 0000
    {{0, 1, 2}, {0, 0, 0}},   // 0001
    {{0, 4, 3}, {0, 0, 0}},   // 0010
    {{1, 2, 4}, {1, 4, 3}},   // 0011
    {{1, 3, 5}, {0, 0, 0}},   // 0100
    {{0, 3, 5}, {0, 5, 2}},   // 0101
    {{0, 4, 5}, {0, 5, 1}},   // 0110
    {{2, 4, 5}, {0, 0, 0}},   // 0111
    {{2, 5, 4}, {0, 0, 0}},   // 1000
    {{0, 5, 4}, {0, 1, 5}},   // 1001
    {{0, 5, 3}, {0, 2, 5}},   // 1010
    {{1, 5, 3}, {0, 0, 0}},   // 1011
    {{1, 4, 2}, {1, 3, 4}},   // 1100
    {{0, 3, 4}, {0, 0, 0}},   // 1101
    {{0, 2, 1}, {0, 0, 0}},   // 1110
    {{0, 0, 0}, {0, 0, 0}},   // 1111
};
constexpr int MESH_TABLE_INTS = 24 + 6 + 12 + 16 + 96;

// device copies, packed for the kernels: per tetrahedron its four corner codes (one byte each), per case its triangle count and the local
// corner pairs (2 + 2 bits per vertex, 4 bits per vertex, 12 bits per triangle) of up to two triangles
constexpr unsigned mesh_pack_tet(int q) {
    return (unsigned)MESH_TET_CORNER[q][0] | (unsigned)MESH_TET_CORNER[q][1] << 8 | (unsigned)MESH_TET_CORNER[q][2] << 16 | (unsigned)MESH_TET_CORNER[q][3] << 24;
}
constexpr unsigned mesh_pack_case(int m) {
    unsigned r = (unsigned)MESH_CASE_NTRI[m] << 24;
    for (int t = 0; t < 2; ++t)
        for (int v = 0; v < 3; ++v) {
            const int e = MESH_CASE_TRI[m][t][v];
            r |= (unsigned)(MESH_TET_EDGE[e][0] | MESH_TET_EDGE[e][1] << 2) << (12 * t + 4 * v);
        }
    return r;
}
__constant__ unsigned MESH_TET_DEV[6] = {mesh_pack_tet(0), mesh_pack_tet(1), mesh_pack_tet(2), mesh_pack_tet(3), mesh_pack_tet(4), mesh_pack_tet(5)};
constexpr unsigned mesh_pack_flip() {
    unsigned r = 0;
    for (int q = 0; q < 6; ++q) r |= (unsigned)MESH_TET_FLIP[q] << q;
    return r;
}
__constant__ unsigned MESH_TET_FLIP_DEV = mesh_pack_flip();
__constant__ unsigned MESH_CASE_DEV[16] = {mesh_pack_case(0),  mesh_pack_case(1),  mesh_pack_case(2),  mesh_pack_case(3), mesh_pack_case(4),  mesh_pack_case(5),
                                           mesh_pack_case(6),  mesh_pack_case(7),  mesh_pack_case(8),  mesh_pack_case(9), mesh_pack_case(10), mesh_pack_case(11),
                                           mesh_pack_case(12), mesh_pack_case(13), mesh_pack_case(14), mesh_pack_case(15)};

constexpr int MESH_THREADS = 256;          // cells per workgroup of classify / apply / emission = cells per partial
constexpr int MESH_SCAN_THREADS = 1024;
constexpr long long MESH_MAX_CELLS = 0x7fffffffll / 12;   // 12 triangles per cell at most: every per-volume offset fits an int32

// cell record: bits 0..6 owned-edge mask (direction k active), bits 8..11 triangle count 0..12, bits 16..23 the inside bits of the 8 corners
__device__ __forceinline__ unsigned mesh_rec_mask(unsigned rec) { return rec & 0x7fu; }
__device__ __forceinline__ unsigned mesh_rec_ntri(unsigned rec) { return (rec >> 8) & 0xfu; }
__device__ __forceinline__ unsigned mesh_rec_inside(unsigned rec) { return (rec >> 16) & 0xffu; }

struct MeshGrid {
    int D, H, W;          // volume extents
    int Hc, Wc;           // padded cell grid: (D+1) x (H+1) x (W+1)
    int cells;            // per volume
    int nblk;             // partials per volume
};

// the zero-padded field at grid point (z, y, x), any integer index: zero outside 0..N-1
__device__ __forceinline__ float mesh_field(const float* __restrict__ d, const MeshGrid& g, int z, int y, int x) {
    const bool in = (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W;
    return in ? d[((long long)z * g.H + y) * g.W + x] : 0.f;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_classify(const float* __restrict__ density, float level, MeshGrid g, uint2* __restrict__ cell,
                                                              unsigned long long* __restrict__ partial) {
    __shared__ unsigned wsum[MESH_THREADS / 64];
    const int vol = blockIdx.y, tid = threadIdx.x;
    const int lin = blockIdx.x * MESH_THREADS + tid;
    unsigned packed = 0;
    if (lin < g.cells) {
        const int cx = lin % g.Wc, cy = (lin / g.Wc) % g.Hc, cz = lin / (g.Wc * g.Hc);
        const float* d = density + (long long)vol * g.D * g.H * g.W;
        unsigned inside = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = mesh_field(d, g, cz - 1 + (c >> 2), cy - 1 + ((c >> 1) & 1), cx - 1 + (c & 1));
            inside |= (v > level ? 1u : 0u) << c;
        }
        unsigned ntri = 0, mask = 0;
        if (inside != 0u && inside != 0xffu) {
            mask = ((inside >> 1) ^ ((inside & 1u) ? 0x7fu : 0u)) & 0x7fu;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const unsigned tc = MESH_TET_DEV[q];
                const unsigned m = ((inside >> (tc & 7u)) & 1u) | ((inside >> ((tc >> 8) & 7u)) & 1u) << 1 | ((inside >> ((tc >> 16) & 7u)) & 1u) << 2 |
                                   ((inside >> ((tc >> 24) & 7u)) & 1u) << 3;
                ntri += MESH_CASE_DEV[m] >> 24;
            }
        }
        cell[(long long)vol * g.cells + lin].x = mask | ntri << 8 | inside << 16;
        packed = (unsigned)__popc(mask) | ntri << 16;
    }
    const unsigned s = wave_sum(packed);            // < 2^16 per thread and half (vertices low, triangles high): no carry between the halves
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < MESH_THREADS / 64; ++w) t += wsum[w];
        partial[(long long)vol * g.nblk + blockIdx.x] = (unsigned long long)(t & 0xffffu) | (unsigned long long)(t >> 16) << 32;
    }
}

// partial[vol][0..nblk) (vertices low word, triangles high word) -> its exclusive scan in place; counts[vol] = the totals
__global__ __launch_bounds__(MESH_SCAN_THREADS) void mesh_scan(unsigned long long* __restrict__ partial, int nblk, int* __restrict__ counts) {
    const int vol = blockIdx.x;
    const unsigned long long carry = block_exclusive_scan_inplace<unsigned long long, MESH_SCAN_THREADS>(partial + (long long)vol * nblk, nblk);
    if (threadIdx.x == 0) {
        counts[2 * vol] = (int)(unsigned)(carry & 0xffffffffull);
        counts[2 * vol + 1] = (int)(unsigned)(carry >> 32);
    }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_apply(uint2* __restrict__ cell, unsigned* __restrict__ toff, const unsigned long long* __restrict__ partial,
                                                           MeshGrid g) {
    __shared__ unsigned wsum[MESH_THREADS / 64];
    const int vol = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lin = blockIdx.x * MESH_THREADS + tid;
    const long long at = (long long)vol * g.cells + lin;
    unsigned own = 0;
    if (lin < g.cells) {
        const unsigned rec = cell[at].x;
        own = (unsigned)__popc(mesh_rec_mask(rec)) | mesh_rec_ntri(rec) << 16;
    }
    const unsigned inc = wave_inclusive_scan(own, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    const unsigned before = waves_before(wsum, wave, 0u);
    if (lin < g.cells && own != 0u) {            // offsets of cells that emit nothing are never read
        const unsigned long long po = partial[(long long)vol * g.nblk + blockIdx.x];
        const unsigned ex = before + inc - own;
        cell[at].y = (unsigned)(po & 0xffffffffull) + (ex & 0xffffu);
        toff[at] = (unsigned)(po >> 32) + (ex >> 16);
    }
}

struct MeshEmit {
    float level;
    float ex, ey, ez;                // world half extents e = 0.5 (N - 1) volume_size / N of W, H, D
    float dx, dy, dz;                // max(N - 1, 1) of W, H, D
    int max_vertices, max_faces;     // rows of the output arrays: per volume (offsets == nullptr) or in all (packed), see row_span
    int C;
};

// gradient of the zero-padded field at a grid point, per axis (f(p + 1) - f(p - 1)) N: the world-space central difference up to the
// common factor 2 volume_size, which the normalisation drops
__device__ __forceinline__ void mesh_gradient(const float* __restrict__ d, const MeshGrid& g, int z, int y, int x, float (&o)[3]) {
    o[0] = (mesh_field(d, g, z, y, x + 1) - mesh_field(d, g, z, y, x - 1)) * (float)g.W;
    o[1] = (mesh_field(d, g, z, y + 1, x) - mesh_field(d, g, z, y - 1, x)) * (float)g.H;
    o[2] = (mesh_field(d, g, z + 1, y, x) - mesh_field(d, g, z - 1, y, x)) * (float)g.D;
}

__device__ __forceinline__ float mesh_world(int ia, int ib, float t, float den, float e) {
    const float idx = (float)ia + (float)(ib - ia) * t;       // (ib - ia) t is exact: one rounding
    return ((2.f * idx) / den - 1.f) * e;                     // three roundings
}

template <bool FEAT>
__global__ __launch_bounds__(MESH_THREADS) void mesh_vertices(const float* __restrict__ density, const float* __restrict__ features,
                                                              const uint2* __restrict__ cell, const int* __restrict__ counts,
                                                              const int* __restrict__ offsets, MeshGrid g, MeshEmit p, float* __restrict__ vertices,
                                                              float* __restrict__ normals, float* __restrict__ vfeat, int* __restrict__ status) {
    const int vol = blockIdx.y;
    const int lin = blockIdx.x * MESH_THREADS + threadIdx.x;
    const MeshSpans spans = mesh_spans(offsets, vol, p.max_vertices, p.max_faces);
    const RowSpan span = spans.v;
    const long long rows = span.row0 + span.room;                                              // first row this volume may not write
    if (blockIdx.x == 0 && threadIdx.x == 0) status[vol] = (counts[2 * vol] > span.room || counts[2 * vol + 1] > spans.f.room) ? FORGE_MESH_OVERFLOW : 0;
    if (lin >= g.cells) return;
    const uint2 rc = cell[(long long)vol * g.cells + lin];
    const unsigned mask = mesh_rec_mask(rc.x);
    if (mask == 0u) return;
    const unsigned inside = mesh_rec_inside(rc.x);
    const int cx = lin % g.Wc, cy = (lin / g.Wc) % g.Hc, cz = lin / (g.Wc * g.Hc);
    const int x0 = cx - 1, y0 = cy - 1, z0 = cz - 1;
    const float* d = density + (long long)vol * g.D * g.H * g.W;
    const float d0 = mesh_field(d, g, z0, y0, x0);
    float g0[3];
    mesh_gradient(d, g, z0, y0, x0, g0);
    long long row = span.row0 + rc.y;
    for (int k = 0; k < 7; ++k) {
        if (!((mask >> k) & 1u)) continue;
        if (row >= rows) return;                               // capacity reached: rows ascend with k
        const int code = k + 1;
        const int x1 = x0 + (code & 1), y1 = y0 + ((code >> 1) & 1), z1 = z0 + (code >> 2);
        const float d1 = mesh_field(d, g, z1, y1, x1);
        float g1[3];
        mesh_gradient(d, g, z1, y1, x1, g1);
        const bool a_is_0 = inside & 1u;                       // a = the inside endpoint
        const float da = a_is_0 ? d0 : d1, db = a_is_0 ? d1 : d0;
        const int xa = a_is_0 ? x0 : x1, ya = a_is_0 ? y0 : y1, za = a_is_0 ? z0 : z1;
        const int xb = a_is_0 ? x1 : x0, yb = a_is_0 ? y1 : y0, zb = a_is_0 ? z1 : z0;
        const float t = (p.level - da) / (db - da);
        float* vo = vertices + row * 3;
        vo[0] = mesh_world(xa, xb, t, p.dx, p.ex);
        vo[1] = mesh_world(ya, yb, t, p.dy, p.ey);
        vo[2] = mesh_world(za, zb, t, p.dz, p.ez);
        float n[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float ga = a_is_0 ? g0[a] : g1[a], gb = a_is_0 ? g1[a] : g0[a];
            n[a] = fmaf(t, gb - ga, ga);
        }
        const float len = sqrtf(fmaf(n[0], n[0], fmaf(n[1], n[1], n[2] * n[2])));
        float* no = normals + row * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) no[a] = len > 0.f ? -n[a] / len : 0.f;
        if (FEAT) {
            const bool in_a = (unsigned)za < (unsigned)g.D && (unsigned)ya < (unsigned)g.H && (unsigned)xa < (unsigned)g.W;
            const bool in_b = (unsigned)zb < (unsigned)g.D && (unsigned)yb < (unsigned)g.H && (unsigned)xb < (unsigned)g.W;
            const float4* fa = reinterpret_cast<const float4*>(features + ((((long long)vol * g.D + za) * g.H + ya) * g.W + xa) * p.C);
            const float4* fb = reinterpret_cast<const float4*>(features + ((((long long)vol * g.D + zb) * g.H + yb) * g.W + xb) * p.C);
            float4* fo = reinterpret_cast<float4*>(vfeat + row * p.C);
            for (int c = 0; c < p.C / 4; ++c) {
                const float4 va = in_a ? fa[c] : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 vb = in_b ? fb[c] : make_float4(0.f, 0.f, 0.f, 0.f);
                fo[c] = make_float4(fmaf(t, vb.x - va.x, va.x), fmaf(t, vb.y - va.y, va.y), fmaf(t, vb.z - va.z, va.z), fmaf(t, vb.w - va.w, va.w));
            }
        }
        ++row;
    }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_faces(const uint2* __restrict__ cell, const unsigned* __restrict__ toff, const int* __restrict__ offsets,
                                                           MeshGrid g, MeshEmit p, int* __restrict__ faces) {
    const int vol = blockIdx.y;
    const int lin = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (lin >= g.cells) return;
    const uint2* cv = cell + (long long)vol * g.cells;
    const unsigned rec = cv[lin].x;
    if (mesh_rec_ntri(rec) == 0u) return;
    const unsigned inside = mesh_rec_inside(rec);
    const RowSpan span = mesh_spans(offsets, vol, p.max_vertices, p.max_faces).f;
    const long long rows = span.row0 + span.room;
    long long row = span.row0 + toff[(long long)vol * g.cells + lin];
    for (int q = 0; q < 6; ++q) {
        const unsigned tc = MESH_TET_DEV[q];
        const unsigned m = ((inside >> (tc & 7u)) & 1u) | ((inside >> ((tc >> 8) & 7u)) & 1u) << 1 | ((inside >> ((tc >> 16) & 7u)) & 1u) << 2 |
                           ((inside >> ((tc >> 24) & 7u)) & 1u) << 3;
        const unsigned cs = MESH_CASE_DEV[m];
        const int nt = (int)(cs >> 24);
        const bool flip = (MESH_TET_FLIP_DEV >> q) & 1u;
        for (int t = 0; t < nt; ++t) {
            if (row >= rows) return;                           // capacity reached: rows ascend with (q, t)
            int idx[3];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const unsigned e = (cs >> (12 * t + 4 * v)) & 0xfu;
                const unsigned ci = (tc >> (8 * (e & 3u))) & 7u, cj = (tc >> (8 * (e >> 2))) & 7u;       // nested corner codes, ci inside cj
                // the owner of an ACTIVE edge is a cell of the padded grid (an edge that starts on the far shell has both ends outside)
                const int owner = lin + (int)(ci & 1u) + (int)((ci >> 1) & 1u) * g.Wc + (int)(ci >> 2) * g.Wc * g.Hc;
                const int k = (int)(cj ^ ci) - 1;
                const uint2 oc = cv[owner < g.cells ? owner : lin];
                idx[v] = (int)(oc.y + (unsigned)__popc(mesh_rec_mask(oc.x) & ((1u << k) - 1u)));
            }
            int* fo = faces + row * 3;
            fo[0] = idx[0];
            fo[1] = flip ? idx[2] : idx[1];
            fo[2] = flip ? idx[1] : idx[2];
            ++row;
        }
    }
}

// workspace of n volumes: cell records [n][cells] uint2 | triangle offsets [n][cells] uint32 | partials [n][nblk] uint64
static int mesh_grid(int n, int D, int H, int W, MeshGrid& g, long long (&off)[4], const char* fn) {
    const int rc = volume_dims_ok(fn, n, D, H, W, 1, MESH_MAX_CELLS);       // cells, 12 triangles each: vertex and triangle offsets are 32-bit
    if (rc != 0) return rc;
    const long long cells = ((long long)D + 1) * ((long long)H + 1) * ((long long)W + 1);
    g.D = D; g.H = H; g.W = W; g.Hc = H + 1; g.Wc = W + 1;
    g.cells = (int)cells;
    g.nblk = (int)((cells + MESH_THREADS - 1) / MESH_THREADS);
    ws_layout({(long long)n * cells * 8, (long long)n * cells * 4, (long long)n * g.nblk * 8}, off);
    return 0;
}

}  // namespace forge

extern "C" long long forge_mesh_workspace_bytes(int n, int D, int H, int W) {
    using namespace forge;
    MeshGrid g;
    long long off[4];
    const int rc = mesh_grid(n, D, H, W, g, off, "forge_mesh_workspace_bytes");
    return rc != 0 ? (long long)rc : off[3];
}

extern "C" int forge_mesh_case_table(int* table, int capacity) {
    using namespace forge;
    FORGE_REQUIRE(table != nullptr, FORGE_EINVAL, "forge_mesh_case_table: null pointer");
    FORGE_REQUIRE(capacity >= MESH_TABLE_INTS, FORGE_EINVAL, "forge_mesh_case_table: capacity %d < %d ints", capacity, MESH_TABLE_INTS);
    int* o = table;
    for (int q = 0; q < 6; ++q)
        for (int c = 0; c < 4; ++c) *o++ = MESH_TET_CORNER[q][c];
    for (int q = 0; q < 6; ++q) *o++ = MESH_TET_FLIP[q];
    for (int e = 0; e < 6; ++e)
        for (int c = 0; c < 2; ++c) *o++ = MESH_TET_EDGE[e][c];
    for (int m = 0; m < 16; ++m) *o++ = MESH_CASE_NTRI[m];
    for (int m = 0; m < 16; ++m)
        for (int t = 0; t < 2; ++t)
            for (int v = 0; v < 3; ++v) *o++ = MESH_CASE_TRI[m][t][v];
    return 0;
}

extern "C" int forge_mesh_count(const float* density, int n, int D, int H, int W, float level, void* workspace, long long workspace_bytes, int* counts,
                                forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(density && workspace && counts, FORGE_EINVAL, "forge_mesh_count: null pointer");
    FORGE_REQUIRE(level_ok(level), FORGE_EINVAL, "forge_mesh_count: level=%g must be finite and > 0 (the virtual shell is zero)", (double)level);
    MeshGrid g;
    long long off[4];
    int rc = mesh_grid(n, D, H, W, g, off, "forge_mesh_count");
    if (rc == 0) rc = workspace_ok("forge_mesh_count", workspace, workspace_bytes, off[3]);
    if (rc != 0) return rc;
    char* ws = (char*)workspace;
    uint2* cell = (uint2*)(ws + off[0]);
    unsigned* toff = (unsigned*)(ws + off[1]);
    unsigned long long* partial = (unsigned long long*)(ws + off[2]);
    const dim3 grid(g.nblk, n);
    hipLaunchKernelGGL(mesh_classify, grid, dim3(MESH_THREADS), 0, (hipStream_t)stream, density, level, g, cell, partial);
    FORGE_LAUNCH_CHECK("forge_mesh_count (classify)");
    hipLaunchKernelGGL(mesh_scan, dim3(n), dim3(MESH_SCAN_THREADS), 0, (hipStream_t)stream, partial, g.nblk, counts);
    FORGE_LAUNCH_CHECK("forge_mesh_count (scan)");
    hipLaunchKernelGGL(mesh_apply, grid, dim3(MESH_THREADS), 0, (hipStream_t)stream, cell, toff, partial, g);
    FORGE_LAUNCH_CHECK("forge_mesh_count (apply)");
    return 0;
}

extern "C" int forge_mesh_emit(const float* density, const float* features, int n, int C, int D, int H, int W, float level, float volume_size,
                               const void* workspace, long long workspace_bytes, const int* counts, const int* offsets, int max_vertices, int max_faces,
                               float* vertices, float* normals, int* faces, float* vertex_features, int* status, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(density && workspace && counts && status, FORGE_EINVAL, "forge_mesh_emit: null pointer");
    FORGE_REQUIRE(max_vertices >= 0 && max_faces >= 0, FORGE_EINVAL, "forge_mesh_emit: max_vertices=%d max_faces=%d must not be negative", max_vertices,
                  max_faces);
    FORGE_REQUIRE((vertices && normals) || max_vertices == 0, FORGE_EINVAL, "forge_mesh_emit: null vertices / normals with max_vertices=%d", max_vertices);
    FORGE_REQUIRE(faces || max_faces == 0, FORGE_EINVAL, "forge_mesh_emit: null faces with max_faces=%d", max_faces);
    FORGE_REQUIRE(level_ok(level), FORGE_EINVAL, "forge_mesh_emit: level=%g must be finite and > 0 (the virtual shell is zero)", (double)level);
    FORGE_REQUIRE(volume_size > 0.f && std::isfinite(volume_size), FORGE_EINVAL, "forge_mesh_emit: volume_size=%g must be finite and > 0", (double)volume_size);
    if (features != nullptr) {
        FORGE_REQUIRE(C >= 4 && C % 4 == 0, FORGE_ESHAPE, "forge_mesh_emit: C=%d must be a positive multiple of 4 (float4 rows)", C);
        FORGE_REQUIRE(vertex_features || max_vertices == 0, FORGE_EINVAL, "forge_mesh_emit: features without vertex_features");
        FORGE_REQUIRE((((unsigned long long)features | (unsigned long long)vertex_features) & 15ull) == 0, FORGE_EINVAL,
                      "forge_mesh_emit: features and vertex_features must be 16-byte aligned");
    }
    MeshGrid g;
    long long off[4];
    int rc = mesh_grid(n, D, H, W, g, off, "forge_mesh_emit");
    if (rc == 0) rc = workspace_ok("forge_mesh_emit", workspace, workspace_bytes, off[3]);
    if (rc != 0) return rc;
    FORGE_REQUIRE(offsets != nullptr || ((long long)n * max_vertices <= 0x7fffffffll && (long long)n * max_faces <= 0x7fffffffll), FORGE_ESHAPE,
                  "forge_mesh_emit: n * max_vertices or n * max_faces beyond 2^31 - 1 rows");
    const char* ws = (const char*)workspace;
    const uint2* cell = (const uint2*)(ws + off[0]);
    const unsigned* toff = (const unsigned*)(ws + off[1]);
    MeshEmit p;
    p.level = level;
    const int N[3] = {W, H, D};
    float e[3], den[3];
    for (int a = 0; a < 3; ++a) {
        e[a] = (float)(0.5 * (double)(N[a] - 1) * (double)volume_size / (double)N[a]);
        den[a] = (float)(N[a] > 1 ? N[a] - 1 : 1);
    }
    p.ex = e[0]; p.ey = e[1]; p.ez = e[2];
    p.dx = den[0]; p.dy = den[1]; p.dz = den[2];
    p.max_vertices = max_vertices;
    p.max_faces = max_faces;
    p.C = features != nullptr ? C : 0;
    const dim3 grid(g.nblk, n);
    if (features != nullptr)
        hipLaunchKernelGGL(mesh_vertices<true>, grid, dim3(MESH_THREADS), 0, (hipStream_t)stream, density, features, cell, counts, offsets, g, p, vertices,
                           normals, vertex_features, status);
    else
        hipLaunchKernelGGL(mesh_vertices<false>, grid, dim3(MESH_THREADS), 0, (hipStream_t)stream, density, features, cell, counts, offsets, g, p, vertices,
                           normals, vertex_features, status);
    FORGE_LAUNCH_CHECK("forge_mesh_emit (vertices)");
    hipLaunchKernelGGL(mesh_faces, grid, dim3(MESH_THREADS), 0, (hipStream_t)stream, cell, toff, offsets, g, p, faces);
    FORGE_LAUNCH_CHECK("forge_mesh_emit (faces)");
    return 0;
}
