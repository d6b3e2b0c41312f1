// bake.hip — visibility-aware vertex colours for extracted meshes (include/forge_hip.h section g2 states the contract): every vertex of
// forge_mesh_emit is projected into the posed images of its volume, and each view's colour is weighted by how well the vertex faces the camera
// and by the transmittance of the density field along the segment from the vertex to the camera centre (the field of the ray-marcher and of the
// mesh: align_corners=True trilinear sampling with zero padding). No depth maps, no rasteriser, no atomics.
//
// One launch. A vertex is served by a GROUP of 8 consecutive lanes of a wave64 (32 vertices per 256-thread workgroup, grid = row blocks x volumes):
// one thread per vertex would leave the device nearly empty (20 k vertices = 80 waves on 256 CUs), and the cost is the V S trilinear gathers.
//   * the group loops the views in increasing v; view2vol, the camera and the gain are workgroup-uniform (a workgroup serves one volume);
//   * projection, facing and the bilinear image weights are computed by all 8 lanes alike (a few dozen operations against S / 8 gathers of 8 taps),
//     so every branch is uniform within the group and the shuffles below always meet active partners;
//   * lane j marches the samples s = j (mod 8) in increasing s and multiplies its own (1 - a_s); the 8 partial products are combined by the fixed
//     xor butterfly 1, 2, 4 (a product is commutative: both partners of a pair compute the same bits, all 8 lanes end with the same T);
//   * samples that cannot touch the volume's support box multiply by exactly 1 and are skipped: a conservative sample interval per (vertex, view),
//     then the exact per-sample test "no tap in range" - the bits do not change;
//   * lane j < C owns colour channel j (its own four image taps, its own running sum); lane 0 writes weight and best.
// Vertices come out of forge_mesh_emit ordered by cell index, so neighbouring groups march neighbouring segments through a volume that sits in
// the L2 (1 MiB at 64^3).
// Resource use (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): 78 VGPR, no LDS, no scratch, 6 waves per SIMD.
// Measured (tools/bake_probe.py, profiles/r19_bake_probe.txt; 3 + 28 views at 256^2 per volume): 0.173 ms at one 64^3 volume (20 k vertices), 3.39 ms at
// eight 128^3 volumes (649 k vertices): 115 G gathering samples/s, 11 % of the L2 bound on their taps. No counters were taken; by arithmetic the
// launch is bound by instruction issue, not by the caches: 3.39 ms on 1024 SIMDs at 2.4 GHz and two cycles per wave64 instruction is about 1700
// issued instructions per wave and view, and the kernel is about 1000 instructions long with 24 correctly rounded divisions - the set-up per view
// (projection, facing, interval) and, per marched sample, three divisions and the index arithmetic of the 8 taps.
#include "geom_common.h"

namespace forge {

constexpr int BAKE_THREADS = 256;
constexpr int BAKE_GROUP = 8;                             // lanes per vertex
constexpr int BAKE_ROWS = BAKE_THREADS / BAKE_GROUP;      // vertices per workgroup

struct BakeParams {
    int n, max_vertices;              // rows per volume (offsets == nullptr) or in all (packed), see row_span
    int D, H, W;
    float hx, hy, hz;
    int C, Hi, Wi, V;
    int S;
    float step, offset;
    int cos_power;
    float z_near, w_min;
    int mode;
    float fill;
};

// the zero-padded trilinear sample at index position (px, py, pz) <-> (W, H, D); any = false (and 0) when no tap is in range
__device__ __forceinline__ float bake_sample(const float* __restrict__ d, int D, int H, int W, float px, float py, float pz, bool& any) {
    px = fminf(fmaxf(px, -2.f), (float)W + 1.f);
    py = fminf(fmaxf(py, -2.f), (float)H + 1.f);
    pz = fminf(fmaxf(pz, -2.f), (float)D + 1.f);
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const bool vx0 = (unsigned)x0 < (unsigned)W, vx1 = (unsigned)(x0 + 1) < (unsigned)W;
    const bool vy0 = (unsigned)y0 < (unsigned)H, vy1 = (unsigned)(y0 + 1) < (unsigned)H;
    const bool vz0 = (unsigned)z0 < (unsigned)D, vz1 = (unsigned)(z0 + 1) < (unsigned)D;
    any = (vx0 | vx1) & (vy0 | vy1) & (vz0 | vz1);
    if (!any) return 0.f;
    const float wxa = vx0 ? (fx + 1.f) - px : 0.f, wxb = vx1 ? px - fx : 0.f;
    const float wya = vy0 ? (fy + 1.f) - py : 0.f, wyb = vy1 ? py - fy : 0.f;
    const float wza = vz0 ? (fz + 1.f) - pz : 0.f, wzb = vz1 ? pz - fz : 0.f;
    const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);       // clamped: every load is inside the volume, weight 0 where virtual
    const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
    const int za = min(max(z0, 0), D - 1), zb = min(max(z0 + 1, 0), D - 1);
    const float* r00 = d + (za * H + ya) * W;
    const float* r01 = d + (za * H + yb) * W;
    const float* r10 = d + (zb * H + ya) * W;
    const float* r11 = d + (zb * H + yb) * W;
    float v = 0.f;
    v = fmaf(wxa * wya * wza, r00[xa], v);
    v = fmaf(wxb * wya * wza, r00[xb], v);
    v = fmaf(wxa * wyb * wza, r01[xa], v);
    v = fmaf(wxb * wyb * wza, r01[xb], v);
    v = fmaf(wxa * wya * wzb, r10[xa], v);
    v = fmaf(wxb * wya * wzb, r10[xb], v);
    v = fmaf(wxa * wyb * wzb, r11[xa], v);
    v = fmaf(wxb * wyb * wzb, r11[xb], v);
    return v;
}

// Conservative sample interval [s0, s1] of the segment o + t u, t_s = (s + 0.5) step: outside it no sample has a tap in range (the index
// position alpha + beta t must lie in (-1, N) on all three axes; a margin in pixels and one sample either way cover the fp32 rounding).
__device__ __forceinline__ void bake_interval(const float (&o)[3], const float (&u)[3], const BakeParams& p, int s_end, int& s0, int& s1) {
    const float hh[3] = {p.hx, p.hy, p.hz};
    const int N[3] = {p.W, p.H, p.D};
    float lo = -INFINITY, hi = INFINITY;
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float sc = 0.5f * (float)(N[a] - 1);
        const float alpha = (o[a] / hh[a] + 1.f) * sc, beta = (u[a] / hh[a]) * sc;
        const float pmin = -1.01f, pmax = (float)N[a] + 0.01f;
        if (fabsf(beta) < 1e-20f) {
            empty |= !(alpha > pmin && alpha < pmax);
        } else {
            const float t1 = (pmin - alpha) / beta, t2 = (pmax - alpha) / beta;
            lo = fmaxf(lo, fminf(t1, t2));
            hi = fminf(hi, fmaxf(t1, t2));
        }
    }
    s0 = 0;
    s1 = -1;
    if (empty || !(lo <= hi)) return;
    const float fs0 = floorf(lo / p.step - 0.5f) - 1.f, fs1 = ceilf(hi / p.step - 0.5f) + 1.f;
    if (fs1 < 0.f || fs0 > (float)(s_end - 1)) return;
    s0 = (int)fmaxf(fs0, 0.f);
    s1 = (int)fminf(fs1, (float)(s_end - 1));
}

__global__ __launch_bounds__(BAKE_THREADS) void mesh_bake_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                 const int* __restrict__ counts, const int* __restrict__ offsets,
                                                                 const float* __restrict__ density, const float* __restrict__ images,
                                                                 const float* __restrict__ view_weight, const float* __restrict__ cams,
                                                                 const int* __restrict__ view2vol, const float* __restrict__ view_gain, BakeParams p,
                                                                 float* __restrict__ colors, float* __restrict__ weight, int* __restrict__ best) {
    const int vol = blockIdx.y;
    const int j = threadIdx.x & (BAKE_GROUP - 1);
    const long long local = (long long)blockIdx.x * BAKE_ROWS + (threadIdx.x / BAKE_GROUP);
    const RowSpan span = mesh_spans(offsets, vol, p.max_vertices, 0).v;                                   // the faces' capacity plays no part here
    const long long have = min((long long)counts[2 * vol], span.room);                                    // a negative offset of either array: none
    if (local >= have) return;                                                                            // the whole group leaves together
    const long long row = span.row0 + local;

    const float px = vertices[row * 3], py = vertices[row * 3 + 1], pz = vertices[row * 3 + 2];
    const float nx = normals[row * 3], ny = normals[row * 3 + 1], nz = normals[row * 3 + 2];
    const bool flat = nx == 0.f && ny == 0.f && nz == 0.f;                                                // zero normal: facing 1, no offset
    const float o[3] = {flat ? px : px + p.offset * nx, flat ? py : py + p.offset * ny, flat ? pz : pz + p.offset * nz};
    const float* dens = density + (long long)vol * p.D * p.H * p.W;
    const long long plane = (long long)p.Hi * p.Wi;
    const float scx = (float)(p.W - 1), scy = (float)(p.H - 1), scz = (float)(p.D - 1);

    float wsum = 0.f, wbest = 0.f, acc = 0.f, cbest = 0.f;
    int ibest = -1;
    for (int v = 0; v < p.V; ++v) {
        if (view2vol[v] != vol) continue;                                                                 // also drops indices outside 0 .. n-1
        const float* cam = cams + v * 16;
        const float xc = cam[0] * px + cam[1] * py + cam[2] * pz + cam[9];
        const float yc = cam[3] * px + cam[4] * py + cam[5] * pz + cam[10];
        const float zc = cam[6] * px + cam[7] * py + cam[8] * pz + cam[11];
        if (!(zc >= p.z_near)) continue;
        const float x = (cam[12] * xc) / zc + cam[14] - 0.5f, y = (cam[13] * yc) / zc + cam[15] - 0.5f;
        if (!(x >= 0.f && x <= (float)(p.Wi - 1) && y >= 0.f && y <= (float)(p.Hi - 1))) continue;
        // direction to the camera centre c = -R^T T, facing
        const float cx = -(cam[0] * cam[9] + cam[3] * cam[10] + cam[6] * cam[11]);
        const float cy = -(cam[1] * cam[9] + cam[4] * cam[10] + cam[7] * cam[11]);
        const float cz = -(cam[2] * cam[9] + cam[5] * cam[10] + cam[8] * cam[11]);
        const float dx = cx - px, dy = cy - py, dz = cz - pz;
        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        const float u[3] = {dx / dist, dy / dist, dz / dist};
        float facing = 1.f;
        if (!flat) {
            const float c = fmaxf(nx * u[0] + ny * u[1] + nz * u[2], 0.f);
            facing = c;
            for (int k = 1; k < p.cos_power; ++k) facing *= c;
        }
        // bilinear taps: the far index is clamped, its weight is 0 there
        const float fx0 = floorf(x), fy0 = floorf(y);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int x1 = min(x0 + 1, p.Wi - 1), y1 = min(y0 + 1, p.Hi - 1);
        const float ax = x - fx0, ay = y - fy0;
        const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
        const int i00 = y0 * p.Wi + x0, i01 = y0 * p.Wi + x1, i10 = y1 * p.Wi + x0, i11 = y1 * p.Wi + x1;
        float m = 1.f;
        if (view_weight != nullptr) {
            const float* mw = view_weight + (long long)v * plane;
            m = w00 * mw[i00] + w01 * mw[i01] + w10 * mw[i10] + w11 * mw[i11];
        }
        float c = 0.f;
        if (j < p.C) {
            const float* im = images + ((long long)v * p.C + j) * plane;
            c = w00 * im[i00] + w01 * im[i01] + w10 * im[i10] + w11 * im[i11];
        }
        // transmittance: lane j multiplies the samples s = j (mod 8) in increasing s; the butterfly combines the 8 partial products
        float T = 1.f;
        if (facing > 0.f) {                                   // facing = 0: the weight is 0 whatever T in [0, 1] is
            const float lim = (dist / p.step) + 0.5f;         // t_s < dist needs s < dist / step - 0.5: a bound on s; the exact test is per sample
            const int s_end = (int)fminf((float)p.S, fmaxf(lim + 1.f, 0.f));
            int s0, s1;
            bake_interval(o, u, p, s_end, s0, s1);
            for (int s = s0 + ((j - s0) & (BAKE_GROUP - 1)); s <= s1; s += BAKE_GROUP) {
                const float t = ((float)s + 0.5f) * p.step;
                if (!(t < dist)) break;                       // t_s increases with s: every later sample of this lane has a_s = 0 too
                const float qx = (((o[0] + t * u[0]) / p.hx + 1.f) / 2.f) * scx;
                const float qy = (((o[1] + t * u[1]) / p.hy + 1.f) / 2.f) * scy;
                const float qz = (((o[2] + t * u[2]) / p.hz + 1.f) / 2.f) * scz;
                bool any;
                const float d = bake_sample(dens, p.D, p.H, p.W, qx, qy, qz, any);
                if (!any) continue;                           // a_s = 0: a factor of exactly 1
                T *= 1.f - fminf(fmaxf(d, 0.f), 1.f);
            }
#pragma unroll
            for (int k = 1; k < BAKE_GROUP; k <<= 1) T *= __shfl_xor(T, k, 64);
        }
        const float gain = view_gain != nullptr ? view_gain[v] : 1.f;
        const float w = gain * m * T * facing;
        wsum += w;
        acc = fmaf(w, c, acc);
        if (w > wbest) {                                      // strict: ties go to the lowest v; never taken unless w > 0
            wbest = w;
            ibest = v;
            cbest = c;
        }
    }
    const bool filled = ibest < 0 || !(wsum >= p.w_min);
    if (j < p.C) colors[row * p.C + j] = filled ? p.fill : (p.mode == 0 ? acc / wsum : cbest);
    if (j == 0) {
        weight[row] = wsum;
        best[row] = ibest;
    }
}

}  // namespace forge

extern "C" int forge_mesh_bake(const float* vertices, const float* normals, const int* counts, const int* offsets, int n, int max_vertices,
                               const float* density, int D, int H, int W, float hx, float hy, float hz, const float* images, const float* view_weight,
                               int C, int Hi, int Wi, const float* cam, const int* view2vol, const float* view_gain, int V, int S, float step,
                               float offset, int cos_power, float z_near, float w_min, int mode, float fill, float* colors, float* weight, int* best,
                               forge_stream_t stream) {
    using namespace forge;
    const int rc = volume_dims_ok("forge_mesh_bake", n, D, H, W, 0, 0x7fffffffll);
    if (rc != 0) return rc;
    FORGE_REQUIRE(Hi >= 1 && Wi >= 1, FORGE_EINVAL, "forge_mesh_bake: Hi=%d Wi=%d must be positive", Hi, Wi);
    FORGE_REQUIRE(max_vertices >= 0, FORGE_EINVAL, "forge_mesh_bake: max_vertices=%d must not be negative", max_vertices);
    FORGE_REQUIRE(V >= 1 && S >= 1, FORGE_EINVAL, "forge_mesh_bake: V=%d and S=%d must be at least 1", V, S);
    FORGE_REQUIRE(step > 0.f && std::isfinite(step), FORGE_EINVAL, "forge_mesh_bake: step=%g must be finite and > 0", (double)step);
    FORGE_REQUIRE(hx > 0.f && hy > 0.f && hz > 0.f && std::isfinite(hx) && std::isfinite(hy) && std::isfinite(hz), FORGE_EINVAL,
                  "forge_mesh_bake: half extents (%g, %g, %g) must be finite and > 0", (double)hx, (double)hy, (double)hz);
    FORGE_REQUIRE(offset >= 0.f && std::isfinite(offset), FORGE_EINVAL, "forge_mesh_bake: offset=%g must be finite and not negative", (double)offset);
    FORGE_REQUIRE(w_min >= 0.f && std::isfinite(w_min), FORGE_EINVAL, "forge_mesh_bake: w_min=%g must be finite and not negative", (double)w_min);
    FORGE_REQUIRE(z_near > 0.f && std::isfinite(z_near), FORGE_EINVAL, "forge_mesh_bake: z_near=%g must be finite and > 0", (double)z_near);
    FORGE_REQUIRE(cos_power >= 1 && cos_power <= 8, FORGE_EINVAL, "forge_mesh_bake: cos_power=%d outside 1 .. 8", cos_power);
    FORGE_REQUIRE(mode == 0 || mode == 1, FORGE_EINVAL, "forge_mesh_bake: mode=%d (0 blend, 1 best view)", mode);
    FORGE_REQUIRE(C >= 1 && C <= 4, FORGE_ESHAPE, "forge_mesh_bake: C=%d image channels outside 1 .. 4", C);
    FORGE_REQUIRE((long long)Hi * Wi <= 0x7fffffffll, FORGE_ESHAPE, "forge_mesh_bake: an image of %d x %d pixels is beyond 32-bit indices", Hi, Wi);
    FORGE_REQUIRE(V <= 0x7fffffff / 16, FORGE_ESHAPE, "forge_mesh_bake: V=%d views beyond 32-bit camera offsets", V);
    FORGE_REQUIRE(offsets != nullptr || (long long)n * max_vertices <= 0x7fffffffll, FORGE_ESHAPE, "forge_mesh_bake: n * max_vertices beyond 2^31 - 1 rows");
    FORGE_REQUIRE(counts && density && images && cam && view2vol, FORGE_EINVAL, "forge_mesh_bake: null pointer");
    if (max_vertices == 0) return 0;                          // zero rows: nothing to launch
    FORGE_REQUIRE(vertices && normals && colors && weight && best, FORGE_EINVAL, "forge_mesh_bake: null pointer (rows) with max_vertices=%d", max_vertices);
    BakeParams p;
    p.n = n; p.max_vertices = max_vertices;
    p.D = D; p.H = H; p.W = W;
    p.hx = hx; p.hy = hy; p.hz = hz;
    p.C = C; p.Hi = Hi; p.Wi = Wi; p.V = V;
    p.S = S; p.step = step; p.offset = offset; p.cos_power = cos_power;
    p.z_near = z_near; p.w_min = w_min; p.mode = mode; p.fill = fill;
    const dim3 grid((unsigned)(((long long)max_vertices + BAKE_ROWS - 1) / BAKE_ROWS), (unsigned)n);
    hipLaunchKernelGGL(mesh_bake_kernel, grid, dim3(BAKE_THREADS), 0, (hipStream_t)stream, vertices, normals, counts, offsets, density, images, view_weight,
                       cam, view2vol, view_gain, p, colors, weight, best);
    FORGE_LAUNCH_CHECK("forge_mesh_bake");
    return 0;
}
