// geomdist.hip — scoring a surface against another (include/forge_hip.h section g3 states the contract): deterministic area-proportional samples
// of triangle meshes, exact brute-force nearest neighbours between two point sets, and the reduction of the distances to accuracy /
// completeness / Chamfer / Hausdorff / F-score / normal consistency. No atomics, no allocation, nothing read back: every entry can sit in a
// captured graph, and every bit of every output is reproducible.
//
// forge_nn_points is the hot path: 10^5 x 10^5 points are 10^10 pairs of fp32 VALU work. One launch, grid = (query blocks, pairs), no split over
// the references (so no merge and no atomics). A 256-thread workgroup owns NN_Q = 256 queries, one per lane in registers (transformed on load),
// and walks the references in tiles of NN_T = 256 points:
//   * thread t loads point t of the NEXT tile into registers before the current tile is scored, and stores it into the LDS tile (three planes
//     x | y | z) after the barrier: the global latency sits behind NN_T pairs of arithmetic per lane;
//   * the inner loop reads four references per plane with one ds_read_b128 AT THE SAME ADDRESS IN EVERY LANE (identical addresses broadcast: no
//     bank conflicts) and scores them against the lane's query: 3 subtractions, 1 multiply, 2 fmas per pair, no branch;
//   * the minimum is tracked per GROUP of NN_G = 8 consecutive references: 8 distances, their minimum (v_min3_f32: 4 instructions), one strict
//     compare and two selects per group - 113 vector instructions per 16 pairs in the compiled loop, 7.06 per pair, against 10 per pair with a
//     compare and two selects (and a move of the scalar index) for every reference. The index is found afterwards: the first reference of the
//     winning group whose distance, by the same expression on the same operands, equals the minimum - 8 more pairs per query;
//   * a tile's tail past p_count is filled with NaN coordinates: fminf drops a NaN operand, so the inner loop has no bounds test;
//   * groups are visited in increasing index and the compare is strict, the re-scan takes the first equal distance: the lowest index wins a tie
//     however the loop is unrolled.
// One query per lane was chosen on measurement (variants of this file with 1, 2 and 4 queries per lane and groups of 8 and 16, same bits from
// all; device events): 1 x 1e5 x 1e5: 2.02 / 3.11 / 5.52 ms; 8 x 1e5 x 1e5: 10.7 / 11.5 / 13.1 ms; groups of 16 change neither. With no split over
// the references a pair of 1e5 points is 1563 waves with one query per lane - 1.5 per SIMD - and half or a quarter of that with more: the device
// runs out of waves long before the LDS reads per pair matter. From the host clock (tools/geometry_metrics_probe.py,
// profiles/r25_geometry_metrics_probe.txt): 1.92 ms = 5.2 T pairs/s at one pair, 11.5 ms = 6.9 T pairs/s = 49 T lane-instructions/s at eight:
// 62 % of 1024 SIMDs x 32 lanes x 2.4 GHz; chunked torch.cdist + min takes 47.0 and 396 ms.
// The difference form (q - p)^2 is deliberate (see g3): |q|^2 + |p|^2 - 2 q.p on the matrix cores cancels to nothing exactly where the metric is
// used, between two samplings of nearly the same surface.
#include "geom_common.h"

namespace forge {

constexpr int NN_THREADS = 256;
constexpr int NN_Q = NN_THREADS;                   // queries per workgroup: one per lane (measured: see above)
constexpr int NN_T = 256;                          // references per LDS tile (one per thread)
constexpr int NN_G = 8;                            // references per group: the minimum is tracked per group, its index found afterwards
static_assert(NN_T == NN_THREADS && NN_G % 4 == 0 && NN_T % (2 * NN_G) == 0, "thread t stages reference t of a tile; groups are whole float4 reads");

constexpr int SCAN_THREADS = 256;                  // one workgroup scans one mesh: thread t owns the faces t chunk .. (t+1) chunk - 1
constexpr int SAMPLE_THREADS = 256;
constexpr int GEOM_BLOCKS = 64;                    // per-(pair, direction) partials of forge_geom_metrics
constexpr int GEOM_PARTIAL = 8;                    // doubles per partial: sum d, sum d^2, max d, count(d < tau_k) x 4, sum |n.n|

// ------------------------------------------------------------------------------------------------------------------------ surface sampling
// cum[f0 + f] = A_0 + ... + A_f, float64, in a FIXED order: thread t sums its chunk in increasing f, thread 0 adds the 256 chunk sums in increasing
// t, then every thread rewrites its chunk as (sum of the chunks before it) + its own running sum. status[v] = FORGE_GEOM_EMPTY iff the total is 0
// or not finite.
__global__ __launch_bounds__(SCAN_THREADS) void surface_scan_kernel(MeshRows m, double* __restrict__ cum, int* __restrict__ status) {
    const int v = blockIdx.x;
    long long v0, f0;
    int nv, nf;
    mesh_rows(m, v, v0, f0, nv, nf);
    const float* vert = m.vertices + 3 * v0;
    const int* faces = m.faces + 3 * f0;
    const int chunk = (nf + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min((int)threadIdx.x * chunk, nf), hi = min(lo + chunk, nf);
    double s = 0.0;
    for (int f = lo; f < hi; ++f) s += face_area(vert, faces + 3ll * f, nv);
    __shared__ double before[SCAN_THREADS + 1];
    before[threadIdx.x + 1] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int t = 0; t < SCAN_THREADS; ++t) {
            const double c = before[t + 1];
            before[t] = run;
            run += c;
        }
        before[SCAN_THREADS] = run;
        status[v] = (run > 0.0 && run <= 1.79769313486231570e308) ? 0 : FORGE_GEOM_EMPTY;       // NaN fails both compares
    }
    __syncthreads();
    const double base = before[threadIdx.x];
    s = 0.0;
    for (int f = lo; f < hi; ++f) {
        s += face_area(vert, faces + 3ll * f, nv);
        cum[f0 + f] = base + s;
    }
}

__global__ __launch_bounds__(SAMPLE_THREADS) void surface_sample_kernel(MeshRows m, const double* __restrict__ cum, const int* __restrict__ status,
                                                                        int n_samples, float* __restrict__ points, float* __restrict__ normals,
                                                                        int* __restrict__ face, float* __restrict__ bary) {
    const int v = blockIdx.y;
    const int i = blockIdx.x * SAMPLE_THREADS + threadIdx.x;
    if (i >= n_samples) return;
    long long v0, f0;
    int nv, nf;
    mesh_rows(m, v, v0, f0, nv, nf);
    const long long row = (long long)v * n_samples + i;
    // barycentrics: the R2 sequence in 32-bit wrap-around arithmetic, 24 bits each, folded into the triangle on the integers
    unsigned k1 = ((unsigned)i * 3242174889u) >> 8, k2 = ((unsigned)i * 2447445414u) >> 8;
    if (k1 + k2 > (1u << 24)) {
        k1 = (1u << 24) - k1;
        k2 = (1u << 24) - k2;
    }
    const float r1 = (float)k1 * 0x1p-24f, r2 = (float)k2 * 0x1p-24f;
    bary[2 * row] = r1;
    bary[2 * row + 1] = r2;
    float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    int f = -1;
    if (status[v] == 0 && nf > 0) {
        const double* c = cum + f0;
        const double u = ((double)i + 0.5) / (double)n_samples * c[nf - 1];
        int lo = 0, hi = nf - 1;                   // the first f with cum[f] > u; cum[nf - 1] > u, clamped all the same
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (c[mid] > u) hi = mid; else lo = mid + 1;
        }
        f = lo;
        const int* fi = m.faces + 3 * (f0 + f);
        const int ia = fi[0], ib = fi[1], ic = fi[2];
        if ((unsigned)ia < (unsigned)nv && (unsigned)ib < (unsigned)nv && (unsigned)ic < (unsigned)nv) {     // a chosen face has A_f > 0, so it is in range
            const float* vert = m.vertices + 3 * v0;
            const float ax = vert[3ll * ia], ay = vert[3ll * ia + 1], az = vert[3ll * ia + 2];
            const float e1x = vert[3ll * ib] - ax, e1y = vert[3ll * ib + 1] - ay, e1z = vert[3ll * ib + 2] - az;
            const float e2x = vert[3ll * ic] - ax, e2y = vert[3ll * ic + 1] - ay, e2z = vert[3ll * ic + 2] - az;
            px = fmaf(r2, e2x, fmaf(r1, e1x, ax));
            py = fmaf(r2, e2y, fmaf(r1, e1y, ay));
            pz = fmaf(r2, e2z, fmaf(r1, e1z, az));
            face_normal(e1x, e1y, e1z, e2x, e2y, e2z, nx, ny, nz);
        } else {
            f = -1;
        }
    }
    points[3 * row] = px;
    points[3 * row + 1] = py;
    points[3 * row + 2] = pz;
    normals[3 * row] = nx;
    normals[3 * row + 1] = ny;
    normals[3 * row + 2] = nz;
    face[row] = f;
}

// ----------------------------------------------------------------------------------------------------------------------- nearest neighbours
__global__ __launch_bounds__(NN_THREADS) void nn_points_kernel(const float* __restrict__ q, const float* __restrict__ p,
                                                               const int* __restrict__ q_count, const int* __restrict__ p_count,
                                                               const float* __restrict__ xf, int Nq, int Np, float* __restrict__ d2_out,
                                                               int* __restrict__ idx_out, float* __restrict__ q_xf) {
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * NN_Q;
    const int nq = clamp_count(q_count, b, Nq), np = clamp_count(p_count, b, Np);
    const float* qb = q + 3ll * b * Nq;
    const float* pb = p + 3ll * b * Np;
    float* d2b = d2_out + (long long)b * Nq;
    int* idxb = idx_out + (long long)b * Nq;

    const int i = q0 + (int)threadIdx.x;           // this lane's query
    const int il = min(i, Nq - 1);                 // a lane past the end scores a copy of the last row and writes nothing
    float qx = qb[3ll * il], qy = qb[3ll * il + 1], qz = qb[3ll * il + 2];
    if (xf != nullptr) apply_xf(xf + 12 * b, qx, qy, qz);
    if (q_xf != nullptr && i < Nq) {               // the queries as they are scored: the references of the caller's opposite direction
        float* o = q_xf + 3ll * ((long long)b * Nq + i);
        o[0] = qx;
        o[1] = qy;
        o[2] = qz;
    }
    float best = INFINITY;
    int bg = -1;                                   // the group of NN_G consecutive references that holds the minimum

    __shared__ __attribute__((aligned(16))) float tile[3][NN_T];
    const int ntiles = q0 < nq ? (np + NN_T - 1) / NN_T : 0;          // workgroup-uniform; a block of rows past q_count searches nothing
    auto fetch = [&](int t, float& x, float& y, float& z) {
        const int j = t * NN_T + (int)threadIdx.x;
        x = y = z = NAN;                           // the tail of the last tile: a NaN distance never wins
        if (j < np) {
            x = pb[3ll * j];
            y = pb[3ll * j + 1];
            z = pb[3ll * j + 2];
        }
    };
    auto dist2 = [&](float px, float py, float pz) {                 // the ONE expression of d2: the scan and the re-scan agree bit for bit
        const float dx = qx - px, dy = qy - py, dz = qz - pz;
        return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    };
    float sx, sy, sz;
    fetch(0, sx, sy, sz);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                           // every wave is done with the previous tile
        tile[0][threadIdx.x] = sx;
        tile[1][threadIdx.x] = sy;
        tile[2][threadIdx.x] = sz;
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1, sx, sy, sz);        // in flight while this tile is scored
        const int group0 = t * (NN_T / NN_G);
#pragma unroll 2
        for (int g = 0; g < NN_T / NN_G; ++g) {
            float m = INFINITY;
#pragma unroll
            for (int e = 0; e < NN_G; e += 4) {    // one address in every lane: a broadcast read
                const float4 X = *reinterpret_cast<const float4*>(&tile[0][g * NN_G + e]);
                const float4 Y = *reinterpret_cast<const float4*>(&tile[1][g * NN_G + e]);
                const float4 Z = *reinterpret_cast<const float4*>(&tile[2][g * NN_G + e]);
                m = fminf(fminf(m, dist2(X.x, Y.x, Z.x)), dist2(X.y, Y.y, Z.y));                             // fminf drops a NaN operand
                m = fminf(fminf(m, dist2(X.z, Y.z, Z.z)), dist2(X.w, Y.w, Z.w));
            }
            const bool lt = m < best;              // strict, groups in increasing index: the first group that holds the minimum keeps it
            best = lt ? m : best;
            bg = lt ? group0 + g : bg;
        }
    }
    // the index: the first reference of the winning group whose distance IS the minimum (the same expression on the same operands)
    int bi = -1;
    if (bg >= 0) {
        for (int e = NN_G - 1; e >= 0; --e) {
            const int j = bg * NN_G + e;
            if (j < np && dist2(pb[3ll * j], pb[3ll * j + 1], pb[3ll * j + 2]) == best) bi = j;
        }
    }
    if (i < Nq) {
        d2b[i] = i < nq ? best : 0.f;
        idxb[i] = i < nq ? bi : -1;
    }
}

// -------------------------------------------------------------------------------------------------------------------------------- metrics
struct GeomTau {
    double tau[FORGE_GEOM_MAX_THRESHOLDS];
    int n;
};

// grid (GEOM_BLOCKS, 2, B): direction 0 scores A -> B (rows of A, normals of B gathered through idx), direction 1 B -> A.
// partial[((b 2 + dir) GEOM_BLOCKS + block) 8 + ..] = sum d | sum d^2 | max d | count(d < tau_k), k = 0..3 | sum |n_from . n_to[idx]|
// hit_ab / hit_ba (forge_geom_metrics_hits; both or neither): the "to" normal of row i is hit[i], row-aligned with the queries, and idx is not read.
__global__ __launch_bounds__(256) void geom_partial_kernel(const float* __restrict__ d2_ab, const int* __restrict__ idx_ab,
                                                           const float* __restrict__ d2_ba, const int* __restrict__ idx_ba,
                                                           const float* __restrict__ hit_ab, const float* __restrict__ hit_ba,
                                                           const float* __restrict__ normals_a, const float* __restrict__ normals_b,
                                                           const int* __restrict__ a_count, const int* __restrict__ b_count, int Na, int Nb,
                                                           GeomTau tau, double* __restrict__ partial) {
    const int b = blockIdx.z, dir = blockIdx.y;
    const int N = dir == 0 ? Na : Nb, M = dir == 0 ? Nb : Na;
    const int n = clamp_count(dir == 0 ? a_count : b_count, b, N);
    const float* d2 = (dir == 0 ? d2_ab : d2_ba) + (long long)b * N;
    const bool aligned = hit_ab != nullptr;
    const int* idx = aligned ? nullptr : (dir == 0 ? idx_ab : idx_ba) + (long long)b * N;
    const float* nf = normals_a == nullptr ? nullptr : (dir == 0 ? normals_a : normals_b) + 3ll * b * N;
    const float* nt = normals_a == nullptr ? nullptr : aligned ? (dir == 0 ? hit_ab : hit_ba) + 3ll * b * N : (dir == 0 ? normals_b : normals_a) + 3ll * b * M;
    double sd = 0.0, sd2 = 0.0, md = 0.0, sn = 0.0, cnt[FORGE_GEOM_MAX_THRESHOLDS] = {0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < n; i += GEOM_BLOCKS * 256) {
        const double v = (double)d2[i];
        const double d = sqrt(v);
        sd += d;
        sd2 += v;
        md = fmax(md, d);
#pragma unroll
        for (int k = 0; k < FORGE_GEOM_MAX_THRESHOLDS; ++k) cnt[k] += (k < tau.n && d < tau.tau[k]) ? 1.0 : 0.0;
        const int j = nf == nullptr ? -1 : aligned ? i : idx[i];        // the row of the "to" normal; without normals idx is not read (it may be null)
        if (nf != nullptr && (aligned || (unsigned)j < (unsigned)M)) {
            const double dot = fma((double)nf[3ll * i + 2], (double)nt[3ll * j + 2],
                                   fma((double)nf[3ll * i + 1], (double)nt[3ll * j + 1], (double)nf[3ll * i] * (double)nt[3ll * j]));
            sn += fabs(dot);
        }
    }
    __shared__ double red[256];
    double* out = partial + (((long long)b * 2 + dir) * GEOM_BLOCKS + blockIdx.x) * GEOM_PARTIAL;
    // `red` is reused back to back: the barrier before each reduction lets every thread finish with the previous one
    auto sum = [&](double v) { __syncthreads(); return block_sum256(v, red); };
    auto maxi = [&](double v) { __syncthreads(); return block_max256(v, red); };
    const double r0 = sum(sd), r1 = sum(sd2), r2 = maxi(md);
    double rc[FORGE_GEOM_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < FORGE_GEOM_MAX_THRESHOLDS; ++k) rc[k] = sum(cnt[k]);
    const double r7 = sum(sn);
    if (threadIdx.x == 0) {
        out[0] = r0;
        out[1] = r1;
        out[2] = r2;
#pragma unroll
        for (int k = 0; k < FORGE_GEOM_MAX_THRESHOLDS; ++k) out[3 + k] = rc[k];
        out[7] = r7;
    }
}

// one thread per pair: the partials of each direction summed in block order, then the metrics (layout: FORGE_GEOM_* in forge_hip.h)
__global__ void geom_finalize_kernel(const double* __restrict__ partial, const int* __restrict__ a_count, const int* __restrict__ b_count, int B,
                                     int Na, int Nb, int n_tau, int have_normals, double* __restrict__ out, int* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double mean_d[2], mean_d2[2], max_d[2], frac[2][FORGE_GEOM_MAX_THRESHOLDS], nc[2];
    const int cnt[2] = {clamp_count(a_count, b, Na), clamp_count(b_count, b, Nb)};
    for (int dir = 0; dir < 2; ++dir) {
        double s[GEOM_PARTIAL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double* p = partial + ((long long)b * 2 + dir) * GEOM_BLOCKS * GEOM_PARTIAL;
        for (int k = 0; k < GEOM_BLOCKS; ++k)
            for (int e = 0; e < GEOM_PARTIAL; ++e) s[e] = e == 2 ? fmax(s[e], p[k * GEOM_PARTIAL + e]) : s[e] + p[k * GEOM_PARTIAL + e];
        const double n = (double)cnt[dir];         // 0 rows: 0 / 0 = NaN in every mean
        mean_d[dir] = s[0] / n;
        mean_d2[dir] = s[1] / n;
        max_d[dir] = cnt[dir] > 0 ? s[2] : (double)NAN;
        for (int k = 0; k < FORGE_GEOM_MAX_THRESHOLDS; ++k) frac[dir][k] = s[3 + k] / n;
        nc[dir] = have_normals ? s[7] / n : (double)NAN;
    }
    double* o = out + (long long)b * FORGE_GEOM_OUT_DOUBLES;
    o[FORGE_GEOM_ACCURACY] = mean_d[0];
    o[FORGE_GEOM_COMPLETENESS] = mean_d[1];
    o[FORGE_GEOM_CHAMFER_L1] = 0.5 * (mean_d[0] + mean_d[1]);
    o[FORGE_GEOM_CHAMFER_L2] = mean_d2[0] + mean_d2[1];
    o[FORGE_GEOM_HAUSDORFF] = (max_d[0] != max_d[0] || max_d[1] != max_d[1]) ? (double)NAN : fmax(max_d[0], max_d[1]);
    o[FORGE_GEOM_NORMAL_CONSISTENCY] = 0.5 * (nc[0] + nc[1]);
    for (int k = 0; k < FORGE_GEOM_MAX_THRESHOLDS; ++k) {
        const double P = k < n_tau ? frac[0][k] : (double)NAN, R = k < n_tau ? frac[1][k] : (double)NAN;
        o[FORGE_GEOM_PRECISION + k] = P;
        o[FORGE_GEOM_RECALL + k] = R;
        o[FORGE_GEOM_FSCORE + k] = (P + R == 0.0) ? 0.0 : 2.0 * P * R / (P + R);
    }
    status[b] = (cnt[0] == 0 || cnt[1] == 0) ? FORGE_GEOM_EMPTY : 0;
}

}  // namespace forge

extern "C" int forge_nn_queries_per_block(void) { return forge::NN_Q; }
extern "C" int forge_nn_tile_points(void) { return forge::NN_T; }
extern "C" int forge_geom_scan_threads(void) { return forge::SCAN_THREADS; }

extern "C" long long forge_surface_sample_workspace_bytes(int n_mesh, int max_faces, int packed) {
    using namespace forge;
    FORGE_REQUIRE(n_mesh >= 1 && max_faces >= 0, FORGE_EINVAL, "forge_surface_sample_workspace_bytes: n_mesh=%d max_faces=%d", n_mesh, max_faces);
    FORGE_REQUIRE(n_mesh <= 65535, FORGE_ESHAPE, "forge_surface_sample_workspace_bytes: n_mesh=%d (at most 65535)", n_mesh);
    const long long rows = packed ? (long long)max_faces : (long long)n_mesh * max_faces;
    FORGE_REQUIRE(rows <= 0x7fffffffll, FORGE_ESHAPE, "forge_surface_sample_workspace_bytes: %lld face rows beyond 2^31 - 1", rows);
    return ((rows * 8 + 15) / 16) * 16 + 16;       // never 0: an empty batch still has a workspace to point at
}

extern "C" int forge_surface_sample(const float* vertices, const int* faces, const int* counts, const int* offsets, int n_mesh, int max_vertices,
                                    int max_faces, int n_samples, void* workspace, long long workspace_bytes, float* points, float* normals,
                                    int* face, float* bary, int* status, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(n_mesh >= 1 && n_samples >= 1, FORGE_EINVAL, "forge_surface_sample: n_mesh=%d and n_samples=%d must be at least 1", n_mesh, n_samples);
    FORGE_REQUIRE(max_vertices >= 0 && max_faces >= 0, FORGE_EINVAL, "forge_surface_sample: negative capacity (%d, %d)", max_vertices, max_faces);
    FORGE_REQUIRE(n_mesh <= 65535, FORGE_ESHAPE, "forge_surface_sample: n_mesh=%d meshes in one call (at most 65535)", n_mesh);
    const long long rows_f = offsets != nullptr ? (long long)max_faces : (long long)n_mesh * max_faces;
    const long long rows_v = offsets != nullptr ? (long long)max_vertices : (long long)n_mesh * max_vertices;
    FORGE_REQUIRE(rows_f <= 0x7fffffffll && rows_v <= 0x7fffffffll && (long long)n_mesh * n_samples <= 0x7fffffffll - SAMPLE_THREADS, FORGE_ESHAPE,
                  "forge_surface_sample: vertex, face or sample rows beyond 2^31 - 1");
    FORGE_REQUIRE(counts && workspace && points && normals && face && bary && status, FORGE_EINVAL, "forge_surface_sample: null pointer");
    FORGE_REQUIRE((vertices || max_vertices == 0) && (faces || max_faces == 0), FORGE_EINVAL,
                  "forge_surface_sample: null pointer (rows) with capacities (%d, %d)", max_vertices, max_faces);
    const long long need = forge_surface_sample_workspace_bytes(n_mesh, max_faces, offsets != nullptr);
    const int rc = workspace_ok("forge_surface_sample", workspace, workspace_bytes, need);
    if (rc != 0) return rc;
    MeshRows m;
    m.vertices = vertices; m.faces = faces; m.counts = counts; m.offsets = offsets;
    m.max_vertices = max_vertices; m.max_faces = max_faces;
    double* cum = (double*)workspace;
    hipLaunchKernelGGL(surface_scan_kernel, dim3((unsigned)n_mesh), dim3(SCAN_THREADS), 0, (hipStream_t)stream, m, cum, status);
    FORGE_LAUNCH_CHECK("forge_surface_sample");
    const dim3 grid((unsigned)((n_samples + SAMPLE_THREADS - 1) / SAMPLE_THREADS), (unsigned)n_mesh);
    hipLaunchKernelGGL(surface_sample_kernel, grid, dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, m, (const double*)cum, (const int*)status, n_samples,
                       points, normals, face, bary);
    FORGE_LAUNCH_CHECK("forge_surface_sample");
    return 0;
}

extern "C" int forge_nn_points(const float* q, const float* p, const int* q_count, const int* p_count, const float* xf, int B, int Nq, int Np,
                               float* d2, int* idx, float* q_xf, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && Nq >= 1 && Np >= 1, FORGE_EINVAL, "forge_nn_points: B=%d Nq=%d Np=%d must be at least 1", B, Nq, Np);
    FORGE_REQUIRE(q && p && d2 && idx, FORGE_EINVAL, "forge_nn_points: null pointer");
    FORGE_REQUIRE(B <= 65535, FORGE_ESHAPE, "forge_nn_points: B=%d pairs in one call (at most 65535)", B);
    FORGE_REQUIRE(Nq <= 0x7fffffff - NN_Q && Np <= 0x7fffffff - NN_T, FORGE_ESHAPE, "forge_nn_points: Nq=%d or Np=%d beyond 32-bit rows", Nq, Np);
    const dim3 grid((unsigned)((Nq + NN_Q - 1) / NN_Q), (unsigned)B);
    hipLaunchKernelGGL(nn_points_kernel, grid, dim3(NN_THREADS), 0, (hipStream_t)stream, q, p, q_count, p_count, xf, Nq, Np, d2, idx, q_xf);
    FORGE_LAUNCH_CHECK("forge_nn_points");
    return 0;
}

extern "C" long long forge_geom_metrics_partial_doubles(int B) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && B <= 65535, FORGE_EINVAL, "forge_geom_metrics_partial_doubles: B=%d outside 1 .. 65535", B);
    return (long long)B * 2 * GEOM_BLOCKS * GEOM_PARTIAL;
}

// the one launch sequence of forge_geom_metrics (idx_*: the "to" normals gathered) and forge_geom_metrics_hits (hit_*: row-aligned)
static int geom_metrics_launch(const char* fn, const float* d2_ab, const int* idx_ab, const float* d2_ba, const int* idx_ba, const float* hit_ab,
                               const float* hit_ba, const float* normals_a, const float* normals_b, const int* a_count, const int* b_count, int B, int Na,
                               int Nb, const double* tau, int n_tau, double* partial, double* out, int* status, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(B >= 1 && Na >= 1 && Nb >= 1, FORGE_EINVAL, "%s: B=%d Na=%d Nb=%d must be at least 1", fn, B, Na, Nb);
    FORGE_REQUIRE(n_tau >= 0 && n_tau <= FORGE_GEOM_MAX_THRESHOLDS, FORGE_EINVAL, "%s: %d thresholds (at most %d)", fn, n_tau, FORGE_GEOM_MAX_THRESHOLDS);
    FORGE_REQUIRE(tau != nullptr || n_tau == 0, FORGE_EINVAL, "%s: null pointer (tau) with %d thresholds", fn, n_tau);
    GeomTau t;
    t.n = n_tau;
    for (int k = 0; k < FORGE_GEOM_MAX_THRESHOLDS; ++k) {
        t.tau[k] = k < n_tau ? tau[k] : 0.0;
        FORGE_REQUIRE(std::isfinite(t.tau[k]), FORGE_EINVAL, "%s: threshold %d = %g is not finite", fn, k, t.tau[k]);
    }
    FORGE_REQUIRE(d2_ab && d2_ba && partial && out && status, FORGE_EINVAL, "%s: null pointer", fn);
    FORGE_REQUIRE(((unsigned long long)partial & 7ull) == 0 && ((unsigned long long)out & 7ull) == 0, FORGE_EINVAL,
                  "%s: partial and out must be 8-byte aligned", fn);
    FORGE_REQUIRE(B <= 65535, FORGE_ESHAPE, "%s: B=%d pairs in one call (at most 65535)", fn, B);
    hipLaunchKernelGGL(geom_partial_kernel, dim3(GEOM_BLOCKS, 2, (unsigned)B), dim3(256), 0, (hipStream_t)stream, d2_ab, idx_ab, d2_ba, idx_ba, hit_ab,
                       hit_ba, normals_a, normals_b, a_count, b_count, Na, Nb, t, partial);
    FORGE_LAUNCH_CHECK(fn);
    hipLaunchKernelGGL(geom_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const double*)partial, a_count, b_count,
                       B, Na, Nb, n_tau, normals_a != nullptr ? 1 : 0, out, status);
    FORGE_LAUNCH_CHECK(fn);
    return 0;
}

extern "C" int forge_geom_metrics(const float* d2_ab, const int* idx_ab, const float* d2_ba, const int* idx_ba, const float* normals_a,
                                  const float* normals_b, const int* a_count, const int* b_count, int B, int Na, int Nb, const double* tau, int n_tau,
                                  double* partial, double* out, int* status, forge_stream_t stream) {
    FORGE_REQUIRE(idx_ab && idx_ba, FORGE_EINVAL, "forge_geom_metrics: null pointer");
    FORGE_REQUIRE((normals_a == nullptr) == (normals_b == nullptr), FORGE_EINVAL, "forge_geom_metrics: give the normals of both sides, or of neither");
    return geom_metrics_launch("forge_geom_metrics", d2_ab, idx_ab, d2_ba, idx_ba, nullptr, nullptr, normals_a, normals_b, a_count, b_count, B, Na, Nb, tau,
                               n_tau, partial, out, status, stream);
}

extern "C" int forge_geom_metrics_hits(const float* d2_ab, const float* hit_ab, const float* d2_ba, const float* hit_ba, const float* normals_a,
                                       const float* normals_b, const int* a_count, const int* b_count, int B, int Na, int Nb, const double* tau,
                                       int n_tau, double* partial, double* out, int* status, forge_stream_t stream) {
    const int given = (hit_ab != nullptr) + (hit_ba != nullptr) + (normals_a != nullptr) + (normals_b != nullptr);
    FORGE_REQUIRE(given == 0 || given == 4, FORGE_EINVAL, "forge_geom_metrics_hits: give the normals and the hit normals of both sides, or none of the four");
    return geom_metrics_launch("forge_geom_metrics_hits", d2_ab, nullptr, d2_ba, nullptr, hit_ab, hit_ba, normals_a, normals_b, a_count, b_count, B, Na, Nb,
                               tau, n_tau, partial, out, status, stream);
}
