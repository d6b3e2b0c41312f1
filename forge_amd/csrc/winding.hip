// winding.hip — generalized winding numbers (include/forge_hip.h section g3c states the contract): for every query the sum of the signed solid
// angles of its pair's triangles over 4 pi: 1 inside a closed mesh wound as g1 winds it, 0 outside, and defined for any triangle soup. Brute
// force over (query, face) pairs in the shape of forge_nn_triangles (tridist.hip). No atomics, no allocation, nothing read back: the entry can
// sit in a captured graph, and every bit of every output is reproducible.
//
// Two launches.
//   tri_stage_kernel  tridist.hip's, through stage_triangles (geom_common.h): the same records of TRI_REC floats, NaN for a face that is no
//                     candidate. The normal in a record is not read here.
//   winding_kernel    grid = (query blocks, pairs), no split over the faces (no combine, no atomics). A 256-thread workgroup owns 256 queries,
//                     one per lane in registers (transformed on load), and walks the records in tiles of WN_T = TRI_TILE faces:
//   * thread t loads record t of the NEXT tile into registers before the current tile is summed and stores it into the LDS tile after the
//     barrier: the global latency sits behind WN_T pairs of arithmetic per lane;
//   * the inner loop reads a record AT THE SAME ADDRESS IN EVERY LANE (identical addresses broadcast: no bank conflicts) and evaluates
//     Van Oosterom and Strackee's half angle, atan2(A . (B x C), la lb lc + (A.B) lc + (B.C) la + (C.A) lb), branch-free;
//   * atan2 is written out here (atan2_poly): one reciprocal, an odd polynomial on [0, 1], the octant and the sign by selects - the contract
//     names its expression order, which a library's atan2f would not let it do, and it carries none of the scaling and special cases of one;
//   * a term that is NaN adds 0 (one compare, one select): the record of a non-candidate, the tail of the last tile, a query on a vertex (0 / 0);
//   * the 8 terms of a GROUP of consecutive faces are summed in fp32 from 0, group totals in float64 in increasing group index. A tile is
//     whole groups and starts at a multiple of WN_G, so the grouping is by face index and the tile size is not in the bits.
// No `a * b + c` is left for the compiler to contract: every fma is written out, so the header's order is the order.
#include "geom_common.h"

namespace forge {

constexpr int WN_THREADS = 256;
constexpr int WN_Q = WN_THREADS;                   // queries per workgroup: one per lane, as nn_triangles_kernel
constexpr int WN_T = TRI_TILE;                     // faces per LDS tile (one per thread)
constexpr int WN_G = 8;                            // faces per fp32 group sum (section g3c: part of the contract, unlike the tile)
static_assert(WN_T == WN_THREADS && WN_T % WN_G == 0, "thread t stages record t of a tile; a tile is whole groups");

struct WnRec {
    float4 r0, r1;
    float r2;                                      // cz: the normal of the record is not read
};

__device__ __forceinline__ float wn_dot(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }

// atan2(y, x) in section g3c's order: t = min(|x|, |y|) / max(|x|, |y|) by one reciprocal, atan(t) = t + t s P(s) with s = t t (P: degree 7,
// within 1.1 ulp of atan on [0, 1] in exact fma arithmetic), then the octant by two selects and the sign of y. x = y = 0 gives 0 inf = NaN.
__device__ __forceinline__ float atan2_poly(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = mn * __builtin_amdgcn_rcpf(mx);                  // v_rcp_f32: 1 ulp
    const float s = t * t;
    float p = 2.920691855e-03f;
    p = fmaf(p, s, -1.636792719e-02f);
    p = fmaf(p, s, 4.321185872e-02f);
    p = fmaf(p, s, -7.552213967e-02f);
    p = fmaf(p, s, 1.066600457e-01f);
    p = fmaf(p, s, -1.421105564e-01f);
    p = fmaf(p, s, 1.999377310e-01f);
    p = fmaf(p, s, -3.333315253e-01f);
    float r = fmaf(p * s, t, t);
    r = ay > ax ? 1.57079637f - r : r;
    r = x < 0.f ? 3.14159274f - r : r;
    return copysignf(r, y);
}

// theta_f of one record seen from the query, or 0 where it is NaN
__device__ __forceinline__ float wn_term(float qx, float qy, float qz, const float4& r0, const float4& r1, float r2) {
    const float Ax = r0.x - qx, Ay = r0.y - qy, Az = r0.z - qz;
    const float Bx = r0.w - qx, By = r1.x - qy, Bz = r1.y - qz;
    const float Cx = r1.z - qx, Cy = r1.w - qy, Cz = r2 - qz;
    const float la = __builtin_amdgcn_sqrtf(wn_dot(Ax, Ay, Az, Ax, Ay, Az));                     // v_sqrt_f32: 1 ulp
    const float lb = __builtin_amdgcn_sqrtf(wn_dot(Bx, By, Bz, Bx, By, Bz));
    const float lc = __builtin_amdgcn_sqrtf(wn_dot(Cx, Cy, Cz, Cx, Cy, Cz));
    const float nx = fmaf(By, Cz, -(Bz * Cy)), ny = fmaf(Bz, Cx, -(Bx * Cz)), nz = fmaf(Bx, Cy, -(By * Cx));
    const float num = wn_dot(Ax, Ay, Az, nx, ny, nz);
    const float ab = wn_dot(Ax, Ay, Az, Bx, By, Bz), bc = wn_dot(Bx, By, Bz, Cx, Cy, Cz), ca = wn_dot(Cx, Cy, Cz, Ax, Ay, Az);
    const float den = fmaf(ca, lb, fmaf(bc, la, fmaf(ab, lc, (la * lb) * lc)));
    const float th = atan2_poly(num, den);
    return th == th ? th : 0.f;
}

__global__ __launch_bounds__(WN_THREADS) void winding_kernel(const float* __restrict__ q, const int* __restrict__ q_count,
                                                             const float* __restrict__ xf_q, MeshRows m, const float4* __restrict__ rec, int Nq,
                                                             float* __restrict__ w_out) {
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * WN_Q;
    const int nq = clamp_count(q_count, b, Nq);
    long long v0, f0;
    int nv, nf;
    mesh_rows(m, b, v0, f0, nv, nf);
    const float4* recb = rec + 3 * f0;
    const float* qb = q + 3ll * b * Nq;

    const int i = q0 + (int)threadIdx.x;           // this lane's query
    const int il = min(i, Nq - 1);                 // a lane past the end sums for a copy of the last row and writes nothing
    float qx = qb[3ll * il], qy = qb[3ll * il + 1], qz = qb[3ll * il + 2];
    if (xf_q != nullptr) apply_xf(xf_q + 12 * b, qx, qy, qz);
    double sum = 0.0;

    __shared__ __attribute__((aligned(16))) float4 tile[WN_T][3];
    const int ntiles = q0 < nq ? (nf + WN_T - 1) / WN_T : 0;          // workgroup-uniform; a block of rows past q_count sums nothing
    auto fetch = [&](int t, WnRec& s) {
        const int j = t * WN_T + (int)threadIdx.x;
        s.r0.x = s.r0.y = s.r0.z = s.r0.w = s.r1.x = s.r1.y = s.r1.z = s.r1.w = s.r2 = NAN;        // the tail of the last tile
        if (j < nf) {                              // j < nf rows from f0 lie inside the workspace (one record per face row)
            s.r0 = recb[3ll * j];
            s.r1 = recb[3ll * j + 1];
            s.r2 = recb[3ll * j + 2].x;
        }
    };
    WnRec s;
    fetch(0, s);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                           // every wave is done with the previous tile
        tile[threadIdx.x][0] = s.r0;
        tile[threadIdx.x][1] = s.r1;
        tile[threadIdx.x][2].x = s.r2;
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1, s);       // in flight while this tile is summed
#pragma unroll 1
        for (int g = 0; g < WN_T / WN_G; ++g) {
            float gs = 0.f;
#pragma unroll
            for (int e = 0; e < WN_G; ++e) {       // one address in every lane: broadcast reads
                const float4 r0 = tile[g * WN_G + e][0], r1 = tile[g * WN_G + e][1];
                gs += wn_term(qx, qy, qz, r0, r1, tile[g * WN_G + e][2].x);
            }
            sum += (double)gs;
        }
    }
    if (i < Nq) w_out[(long long)b * Nq + i] = i < nq ? (float)(sum * 0.15915494309189535) : 0.f;       // 1 / (2 pi)
}

}  // namespace forge

extern "C" long long forge_winding_workspace_bytes(int n_mesh, int max_faces, int packed) {
    using namespace forge;
    FORGE_REQUIRE(n_mesh >= 1 && max_faces >= 0, FORGE_EINVAL, "forge_winding_workspace_bytes: n_mesh=%d max_faces=%d", n_mesh, max_faces);
    FORGE_REQUIRE(n_mesh <= 65535, FORGE_ESHAPE, "forge_winding_workspace_bytes: n_mesh=%d (at most 65535)", n_mesh);
    const long long rows = packed ? (long long)max_faces : (long long)n_mesh * max_faces;
    FORGE_REQUIRE(rows <= 0x7fffffffll, FORGE_ESHAPE, "forge_winding_workspace_bytes: %lld face rows beyond 2^31 - 1", rows);
    return rows * (TRI_REC * 4) + 16;              // forge_nn_triangles_workspace_bytes: the same records
}

extern "C" int forge_winding_number(const float* q, const int* q_count, const float* xf_q, const float* vertices, const int* faces, const int* counts,
                                    const int* offsets, const float* xf_mesh, int B, int Nq, int max_vertices, int max_faces, void* workspace,
                                    long long workspace_bytes, float* w, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && Nq >= 1, FORGE_EINVAL, "forge_winding_number: B=%d and Nq=%d must be at least 1", B, Nq);
    FORGE_REQUIRE(max_vertices >= 0 && max_faces >= 0, FORGE_EINVAL, "forge_winding_number: negative capacity (%d, %d)", max_vertices, max_faces);
    FORGE_REQUIRE(B <= 65535, FORGE_ESHAPE, "forge_winding_number: B=%d pairs in one call (at most 65535)", B);
    const long long rows_f = offsets != nullptr ? (long long)max_faces : (long long)B * max_faces;
    const long long rows_v = offsets != nullptr ? (long long)max_vertices : (long long)B * max_vertices;
    FORGE_REQUIRE(rows_f <= 0x7fffffffll && rows_v <= 0x7fffffffll && Nq <= 0x7fffffff - WN_Q && max_faces <= 0x7fffffff - WN_T, FORGE_ESHAPE,
                  "forge_winding_number: vertex, face or query rows beyond 32-bit rows");
    FORGE_REQUIRE(q && counts && workspace && w, FORGE_EINVAL, "forge_winding_number: null pointer");
    FORGE_REQUIRE((vertices || max_vertices == 0) && (faces || max_faces == 0), FORGE_EINVAL,
                  "forge_winding_number: null pointer (rows) with capacities (%d, %d)", max_vertices, max_faces);
    const long long need = forge_winding_workspace_bytes(B, max_faces, offsets != nullptr);
    const int rc = workspace_ok("forge_winding_number", workspace, workspace_bytes, need);
    if (rc != 0) return rc;
    MeshRows m;
    m.vertices = vertices; m.faces = faces; m.counts = counts; m.offsets = offsets;
    m.max_vertices = max_vertices; m.max_faces = max_faces;
    float4* rec = (float4*)workspace;
    const int rs = stage_triangles(m, xf_mesh, rec, B, (hipStream_t)stream, "forge_winding_number");
    if (rs != 0) return rs;
    hipLaunchKernelGGL(winding_kernel, dim3((unsigned)((Nq + WN_Q - 1) / WN_Q), (unsigned)B), dim3(WN_THREADS), 0, (hipStream_t)stream, q, q_count, xf_q,
                       m, (const float4*)rec, Nq, w);
    FORGE_LAUNCH_CHECK("forge_winding_number");
    return 0;
}
