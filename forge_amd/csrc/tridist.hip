// tridist.hip — exact point-to-triangle distances (include/forge_hip.h section g3b states the contract): for every query the closest triangle of
// its pair's mesh, brute force, in the style of forge_nn_points (geomdist.hip). No atomics, no allocation, nothing read back: the entry can sit in
// a captured graph, and every bit of every output is reproducible.
//
// Two launches.
//   tri_stage_kernel    one thread per face row: resolves the row layout (mesh_rows), gathers the three corners, applies xf_mesh, computes the
//                       face normal, and writes a packed record of TRI_REC floats (a | b | c | n) into the workspace. A face that is no candidate
//                       (an index outside the mesh, zero float64 area) is written as a record of NaN: the search needs no test.
//   nn_triangles_kernel grid = (query blocks, pairs), no split over the faces (no merge, no atomics). A 256-thread workgroup owns 256 queries,
//                       one per lane in registers (transformed on load), and walks the records in tiles of NT_T = 256 faces:
//   * thread t loads record t of the NEXT tile into registers before the current tile is scored and stores it into the LDS tile after the
//     barrier: the global latency sits behind NT_T pairs of arithmetic per lane;
//   * the inner loop reads a record with three ds_read_b128 AT THE SAME ADDRESS IN EVERY LANE (identical addresses broadcast: no bank conflicts)
//     and scores it against the lane's query with tri_closest: branch-free, selects only, because the lanes of a wave hold different queries
//     and would diverge in every region test;
//   * the minimum is tracked per GROUP of NT_G = 8 consecutive faces (fminf drops a NaN operand), the group by one strict compare and two
//     selects; the face is found afterwards: the first record of the winning group whose distance, by the same expression on the same operands,
//     equals the minimum. That re-scan also yields the closest point and carries the normal;
//   * a tile's tail past the face count is filled with NaN records, so the inner loop has no bounds test;
//   * groups are visited in increasing index and the compare is strict, the re-scan takes the first equal distance: the lowest face wins a tie.
// tri_closest has no `a * b + c` left for the compiler to contract: every fma is written out, so the scan and the re-scan agree bit for bit.
#include "geom_common.h"

namespace forge {

constexpr int NT_THREADS = 256;
constexpr int NT_Q = NT_THREADS;                   // queries per workgroup: one per lane, as nn_points_kernel measured to be right
constexpr int NT_T = TRI_TILE;                     // faces per LDS tile (one per thread)
constexpr int NT_G = 8;                            // faces per group: the minimum is tracked per group, its face found afterwards
static_assert(NT_T == NT_THREADS && NT_T % NT_G == 0, "thread t stages record t of a tile; a tile is whole groups");

struct TriRec {
    float4 r0, r1, r2;
};

__global__ __launch_bounds__(NT_THREADS) void tri_stage_kernel(MeshRows m, const float* __restrict__ xf_mesh, float4* __restrict__ rec) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * NT_THREADS + (int)threadIdx.x;
    long long v0, f0;
    int nv, nf;
    mesh_rows(m, b, v0, f0, nv, nf);
    if (j >= nf) return;                           // nf rows from f0 lie inside the face array, hence inside the workspace (one record per face row)
    const float* vert = m.vertices + 3 * v0;
    const int* fi = m.faces + 3 * (f0 + j);
    float4 r0, r1, r2;
    r0.x = r0.y = r0.z = r0.w = r1.x = r1.y = r1.z = r1.w = r2.x = r2.y = r2.z = r2.w = NAN;
    if (face_area(vert, fi, nv) != 0.0) {          // in range and with area (a NaN area passes: its corners are NaN already)
        const int ia = fi[0], ib = fi[1], ic = fi[2];
        float ax = vert[3ll * ia], ay = vert[3ll * ia + 1], az = vert[3ll * ia + 2];
        float bx = vert[3ll * ib], by = vert[3ll * ib + 1], bz = vert[3ll * ib + 2];
        float cx = vert[3ll * ic], cy = vert[3ll * ic + 1], cz = vert[3ll * ic + 2];
        if (xf_mesh != nullptr) {
            const float* x = xf_mesh + 12 * b;
            apply_xf(x, ax, ay, az);
            apply_xf(x, bx, by, bz);
            apply_xf(x, cx, cy, cz);
        }
        float nx = 0.f, ny = 0.f, nz = 0.f;
        face_normal(bx - ax, by - ay, bz - az, cx - ax, cy - ay, cz - az, nx, ny, nz);
        r0 = make_float4(ax, ay, az, bx);
        r1 = make_float4(by, bz, cx, cy);
        r2 = make_float4(cz, nx, ny, nz);
    }
    float4* o = rec + 3 * (f0 + j);
    o[0] = r0;
    o[1] = r1;
    o[2] = r2;
}

// The staging launch, for every entry that searches the records (geom_common.h declares it): one record per face row of every mesh into rec.
int stage_triangles(const MeshRows& m, const float* xf_mesh, float4* rec, int B, hipStream_t stream, const char* fn) {
    if (m.max_faces > 0) {
        hipLaunchKernelGGL(tri_stage_kernel, dim3((unsigned)((m.max_faces + NT_THREADS - 1) / NT_THREADS), (unsigned)B), dim3(NT_THREADS), 0, stream, m,
                           xf_mesh, rec);
        FORGE_LAUNCH_CHECK(fn);
    }
    return 0;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }

// The closest point of triangle (a, b, c) to the query (qx, qy, qz), RELATIVE to the query, and its squared length: section g3b's arithmetic, in
// its order. The corners are taken relative to the query first; the region tests follow Ericson (Real-Time Collision Detection, 5.1.5) in his
// order of precedence (A, B, edge AB, C, edge AC, edge BC, interior), applied here from the last to the first so that the first one that holds
// decides. Every region is written as P = A + v ab + w ac with (v, w) = (vn, wn) / den: one reciprocal on every path. A NaN anywhere fails every
// test, takes the interior path and gives a NaN distance.
__device__ __forceinline__ float tri_closest(float qx, float qy, float qz, const float4& r0, const float4& r1, const float4& r2, float& Px, float& Py,
                                             float& Pz) {
    const float Ax = r0.x - qx, Ay = r0.y - qy, Az = r0.z - qz;
    const float Bx = r0.w - qx, By = r1.x - qy, Bz = r1.y - qz;
    const float Cx = r1.z - qx, Cy = r1.w - qy, Cz = r2.x - qz;
    const float abx = Bx - Ax, aby = By - Ay, abz = Bz - Az;
    const float acx = Cx - Ax, acy = Cy - Ay, acz = Cz - Az;
    const float n1 = dot3(abx, aby, abz, Ax, Ay, Az), n2 = dot3(acx, acy, acz, Ax, Ay, Az);      // n_k = -d_k of Ericson: the query is the origin
    const float n3 = dot3(abx, aby, abz, Bx, By, Bz), n4 = dot3(acx, acy, acz, Bx, By, Bz);
    const float n5 = dot3(abx, aby, abz, Cx, Cy, Cz), n6 = dot3(acx, acy, acz, Cx, Cy, Cz);
    const float vc = fmaf(n1, n4, -(n3 * n2)), vb = fmaf(n5, n2, -(n1 * n6)), va = fmaf(n3, n6, -(n5 * n4));
    const float t34 = n3 - n4, t65 = n6 - n5;
    float vn = vb, wn = vc, den = (va + vb) + vc;                                                 // interior
    const bool eBC = va <= 0.f && t34 >= 0.f && t65 >= 0.f;
    vn = eBC ? t65 : vn;
    wn = eBC ? t34 : wn;
    den = eBC ? t34 + t65 : den;
    const bool eAC = vb <= 0.f && n2 <= 0.f && n6 >= 0.f;
    vn = eAC ? 0.f : vn;
    wn = eAC ? n2 : wn;
    den = eAC ? n2 - n6 : den;
    const bool vC = n6 <= 0.f && n5 >= n6;
    vn = vC ? 0.f : vn;
    wn = vC ? 1.f : wn;
    den = vC ? 1.f : den;
    const bool eAB = vc <= 0.f && n1 <= 0.f && n3 >= 0.f;
    vn = eAB ? n1 : vn;
    wn = eAB ? 0.f : wn;
    den = eAB ? n1 - n3 : den;
    const bool vB = n3 <= 0.f && n4 >= n3;
    vn = vB ? 1.f : vn;
    wn = vB ? 0.f : wn;
    den = vB ? 1.f : den;
    const bool vA = n1 >= 0.f && n2 >= 0.f;
    vn = vA ? 0.f : vn;
    wn = vA ? 0.f : wn;
    den = vA ? 1.f : den;
    const float r = __builtin_amdgcn_rcpf(den);    // v_rcp_f32: 1 ulp
    const float v = vn * r, w = wn * r;
    Px = fmaf(w, acx, fmaf(v, abx, Ax));
    Py = fmaf(w, acy, fmaf(v, aby, Ay));
    Pz = fmaf(w, acz, fmaf(v, abz, Az));
    return fmaf(Pz, Pz, fmaf(Py, Py, Px * Px));
}

__global__ __launch_bounds__(NT_THREADS) void nn_triangles_kernel(const float* __restrict__ q, const int* __restrict__ q_count,
                                                                  const float* __restrict__ xf_q, MeshRows m, const float4* __restrict__ rec, int Nq,
                                                                  float* __restrict__ d2_out, int* __restrict__ face_out,
                                                                  float* __restrict__ closest_out, float* __restrict__ normal_out) {
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * NT_Q;
    const int nq = clamp_count(q_count, b, Nq);
    long long v0, f0;
    int nv, nf;
    mesh_rows(m, b, v0, f0, nv, nf);
    const float4* recb = rec + 3 * f0;
    const float* qb = q + 3ll * b * Nq;

    const int i = q0 + (int)threadIdx.x;           // this lane's query
    const int il = min(i, Nq - 1);                 // a lane past the end scores a copy of the last row and writes nothing
    float qx = qb[3ll * il], qy = qb[3ll * il + 1], qz = qb[3ll * il + 2];
    if (xf_q != nullptr) apply_xf(xf_q + 12 * b, qx, qy, qz);
    float best = INFINITY;
    int bg = -1;                                   // the group of NT_G consecutive faces that holds the minimum

    __shared__ __attribute__((aligned(16))) float4 tile[NT_T][3];
    const int ntiles = q0 < nq ? (nf + NT_T - 1) / NT_T : 0;          // workgroup-uniform; a block of rows past q_count searches nothing
    auto fetch = [&](int t, TriRec& s) {
        const int j = t * NT_T + (int)threadIdx.x;
        s.r0.x = s.r0.y = s.r0.z = s.r0.w = s.r1.x = s.r1.y = s.r1.z = s.r1.w = s.r2.x = s.r2.y = s.r2.z = s.r2.w = NAN;       // the tail of the last tile
        if (j < nf) {
            s.r0 = recb[3ll * j];
            s.r1 = recb[3ll * j + 1];
            s.r2 = recb[3ll * j + 2];
        }
    };
    TriRec s;
    float Px, Py, Pz;
    fetch(0, s);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                           // every wave is done with the previous tile
        tile[threadIdx.x][0] = s.r0;
        tile[threadIdx.x][1] = s.r1;
        tile[threadIdx.x][2] = s.r2;
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1, s);       // in flight while this tile is scored
        const int group0 = t * (NT_T / NT_G);
#pragma unroll 1
        for (int g = 0; g < NT_T / NT_G; ++g) {
            float mn = INFINITY;
#pragma unroll
            for (int e = 0; e < NT_G; ++e) {       // one address in every lane: broadcast reads
                const float4 r0 = tile[g * NT_G + e][0], r1 = tile[g * NT_G + e][1], r2 = tile[g * NT_G + e][2];
                mn = fminf(mn, tri_closest(qx, qy, qz, r0, r1, r2, Px, Py, Pz));                  // fminf drops a NaN operand
            }
            const bool lt = mn < best;             // strict, groups in increasing index: the first group that holds the minimum keeps it
            best = lt ? mn : best;
            bg = lt ? group0 + g : bg;
        }
    }
    // the face: the first record of the winning group whose distance IS the minimum (the same expression on the same operands)
    int bi = -1;
    float cx = 0.f, cy = 0.f, cz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (bg >= 0) {
        for (int e = NT_G - 1; e >= 0; --e) {
            const int j = bg * NT_G + e;
            if (j < nf) {
                const float4 r0 = recb[3ll * j], r1 = recb[3ll * j + 1], r2 = recb[3ll * j + 2];
                if (tri_closest(qx, qy, qz, r0, r1, r2, Px, Py, Pz) == best) {
                    bi = j;
                    cx = qx + Px;
                    cy = qy + Py;
                    cz = qz + Pz;
                    nx = r2.y;
                    ny = r2.z;
                    nz = r2.w;
                }
            }
        }
    }
    if (i < Nq) {
        const bool valid = i < nq;
        const long long row = (long long)b * Nq + i;
        d2_out[row] = valid ? best : 0.f;
        face_out[row] = valid ? bi : -1;
        if (closest_out != nullptr) {
            closest_out[3 * row] = valid ? cx : 0.f;
            closest_out[3 * row + 1] = valid ? cy : 0.f;
            closest_out[3 * row + 2] = valid ? cz : 0.f;
        }
        if (normal_out != nullptr) {
            normal_out[3 * row] = valid ? nx : 0.f;
            normal_out[3 * row + 1] = valid ? ny : 0.f;
            normal_out[3 * row + 2] = valid ? nz : 0.f;
        }
    }
}

}  // namespace forge

extern "C" int forge_nn_tile_faces(void) { return forge::NT_T; }

extern "C" long long forge_nn_triangles_workspace_bytes(int n_mesh, int max_faces, int packed) {
    using namespace forge;
    FORGE_REQUIRE(n_mesh >= 1 && max_faces >= 0, FORGE_EINVAL, "forge_nn_triangles_workspace_bytes: n_mesh=%d max_faces=%d", n_mesh, max_faces);
    FORGE_REQUIRE(n_mesh <= 65535, FORGE_ESHAPE, "forge_nn_triangles_workspace_bytes: n_mesh=%d (at most 65535)", n_mesh);
    const long long rows = packed ? (long long)max_faces : (long long)n_mesh * max_faces;
    FORGE_REQUIRE(rows <= 0x7fffffffll, FORGE_ESHAPE, "forge_nn_triangles_workspace_bytes: %lld face rows beyond 2^31 - 1", rows);
    return rows * (TRI_REC * 4) + 16;              // never 0: an empty batch still has a workspace to point at
}

extern "C" int forge_nn_triangles(const float* q, const int* q_count, const float* xf_q, const float* vertices, const int* faces, const int* counts,
                                  const int* offsets, const float* xf_mesh, int B, int Nq, int max_vertices, int max_faces, void* workspace,
                                  long long workspace_bytes, float* d2, int* face, float* closest, float* normal, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && Nq >= 1, FORGE_EINVAL, "forge_nn_triangles: B=%d and Nq=%d must be at least 1", B, Nq);
    FORGE_REQUIRE(max_vertices >= 0 && max_faces >= 0, FORGE_EINVAL, "forge_nn_triangles: negative capacity (%d, %d)", max_vertices, max_faces);
    FORGE_REQUIRE(B <= 65535, FORGE_ESHAPE, "forge_nn_triangles: B=%d pairs in one call (at most 65535)", B);
    const long long rows_f = offsets != nullptr ? (long long)max_faces : (long long)B * max_faces;
    const long long rows_v = offsets != nullptr ? (long long)max_vertices : (long long)B * max_vertices;
    FORGE_REQUIRE(rows_f <= 0x7fffffffll && rows_v <= 0x7fffffffll && Nq <= 0x7fffffff - NT_Q && max_faces <= 0x7fffffff - NT_T, FORGE_ESHAPE,
                  "forge_nn_triangles: vertex, face or query rows beyond 32-bit rows");
    FORGE_REQUIRE(q && counts && workspace && d2 && face, FORGE_EINVAL, "forge_nn_triangles: null pointer");
    FORGE_REQUIRE((vertices || max_vertices == 0) && (faces || max_faces == 0), FORGE_EINVAL,
                  "forge_nn_triangles: null pointer (rows) with capacities (%d, %d)", max_vertices, max_faces);
    const long long need = forge_nn_triangles_workspace_bytes(B, max_faces, offsets != nullptr);
    const int rc = workspace_ok("forge_nn_triangles", workspace, workspace_bytes, need);
    if (rc != 0) return rc;
    MeshRows m;
    m.vertices = vertices; m.faces = faces; m.counts = counts; m.offsets = offsets;
    m.max_vertices = max_vertices; m.max_faces = max_faces;
    float4* rec = (float4*)workspace;
    const int rs = stage_triangles(m, xf_mesh, rec, B, (hipStream_t)stream, "forge_nn_triangles");
    if (rs != 0) return rs;
    hipLaunchKernelGGL(nn_triangles_kernel, dim3((unsigned)((Nq + NT_Q - 1) / NT_Q), (unsigned)B), dim3(NT_THREADS), 0, (hipStream_t)stream, q, q_count,
                       xf_q, m, (const float4*)rec, Nq, d2, face, closest, normal);
    FORGE_LAUNCH_CHECK("forge_nn_triangles");
    return 0;
}
