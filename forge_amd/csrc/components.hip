// components.hip — connected components of density volumes under the Kuhn adjacency, their statistics, and the selection that drops floaters
// (include/forge_hip.h section g4 states the contract: inside iff d > level, 14 neighbours = the edges mesh.hip marches over, components numbered
// by their lowest linear index, integer statistics, a cleaned volume that keeps the extracted surface an ordered sub-mesh).
//
// Union-find with ONE invariant, held by every store ever made to a parent slot: parent[x] <= x for an inside voxel (-1 for an outside one, never
// touched again). A root is therefore its component's lowest linear index, every walk up the forest moves to a strictly smaller index and ends
// after at most x steps WHATEVER value a load returns (a stale parent is an older value of the slot, so it is <= x too), and no kernel ever waits
// for another workgroup: there is no flag, no ticket, no "repeat until unchanged".
//
// Launches of forge_components_label (V = D H W voxels per volume, T = 8):
//   cc_local    one workgroup per T^3 tile: inside test, union of the tile's voxels over the 7 positive directions in LDS (ds atomics), then
//               parent[x] = the global index of the tile-local root, size[x] = 0 at tile-local roots (the only voxels that can stay roots)
//   cc_seam     one thread per voxel; a voxel on a +x / +y / +z tile face unions with its inside neighbours in the adjacent tiles on the global
//               parent array. The one launch in which workgroups write words other workgroups read: EVERY parent access in it is an agent-scope
//               atomic (relaxed load, fetch_min), so no access can be served from a non-coherent L1 / L2 line; and the union is correct under stale
//               reads all the same (see cc_union).
//   cc_flatten  plain loads of the now final forest: root[x] = find(x) (-1 outside), the root's size by integer atomicAdd aggregated per wave
//               (lanes that share a root add once; a wave inside the object issues ONE atomic), the number of roots per 256 voxels -> partial
//   cc_scan     one workgroup per volume: exclusive scan of the partials in chunks of 1024 with a running carry; counts[v] = K_v
//   cc_rank     rank of every root = partial offset + workgroup scan of the is-root flags, stored in the root's parent slot (the forest is no
//               longer needed); per 256 voxels the best (size, lowest index) root as one 64-bit key -> pmax
//   cc_labels   labels[x] = rank[root[x]] + 1 (0 outside); only when labels are asked for
// forge_components_stats: cc_stats_init (rows below K_v: box = (INT_MAX.., 0..), sums 0; rows from K_v on: zero; the overflow bit), cc_stats
// (sizes copied from the root's slot; box and coordinate sums by integer atomicMin / atomicMax / 64-bit atomicAdd, reduced per wave and root first).
// forge_components_select: cc_winner (one workgroup per volume: the maximum of pmax = L_v and the winning root, the fraction threshold in float64),
// cc_select (out = density bits, or +0.0f for inside voxels of removed components).
// Integer atomics only: every output bit is independent of arrival order. No floating-point atomic, no inline assembly, vector stores only.
//
// Resource use (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch and no spills in any kernel:
//   cc_local 10 VGPR, 2048 B LDS (the tile's parents); cc_seam 12 VGPR, no LDS; cc_flatten 8 VGPR, 16 B LDS; cc_scan 24 VGPR, 68 B LDS;
//   cc_rank 14 VGPR, 48 B LDS; cc_labels 4 VGPR, no LDS; cc_stats_init 12 VGPR, no LDS; cc_stats 43 VGPR, no LDS; cc_winner 17 VGPR, 128 B LDS;
//   cc_select 10 VGPR, no LDS. Every kernel is at 8 waves per SIMD.
// Bytes moved by design per voxel (int32 / float32 words): cc_local reads density 4, writes parent 4 (+ 4 at tile-local roots); cc_seam touches
// only inside voxels on tile faces; cc_flatten reads parent 4 (+ the walk, cache hits), writes root 4; cc_rank reads root 4 (+ size, writes rank
// at roots); cc_labels reads root 4, writes labels 4; cc_stats reads root 4; cc_select reads density 4 and root 4, writes out 4 (size gathered at
// the root: one line per wave inside the object). keep_components = local + seam + flatten + scan + rank + winner + select: 32 bytes per voxel;
// label_components adds 8 (labels) + 4 (stats) = 44 bytes per voxel.
// These byte counts size the workspace traffic; they are not a roofline the kernels approach: cc_seam launches a thread per voxel though only
// tile-face voxels work, the per-wave grouping takes up to 64 passes on dusty fields, and at 64^3 .. 8 x 128^3 the launches are latency-bound.
#include <climits>

#include "geom_common.h"

namespace forge {

constexpr int CC_T = 8;                         // tile edge of cc_local, all three axes
constexpr int CC_TILE = CC_T * CC_T * CC_T;     // = its workgroup size: one voxel per thread
constexpr int CC_THREADS = 256;                 // voxels per workgroup of the linear kernels = voxels per partial
constexpr int CC_SCAN_THREADS = 1024;

struct CcGrid {
    int D, H, W;
    int V;                // voxels per volume, < 2^31 - 1
    int nblk;             // partials per volume
    int tw, th, ntile;    // tiles along W, along H, per volume
};

struct CcVol {            // per volume, in the workspace
    int K;                // components
    int L;                // largest size (0: no inside voxel)
    int winner;           // root of the largest component, ties to the lowest index (-1: none)
    int thr;              // ceil(min_fraction L), set by forge_components_select
};

// find: walk to the root. Terminates by construction: each step moves to a strictly smaller non-negative index, whatever the load returns
// (a value that is not smaller - the root's own index, or anything a corrupted slot could hold - ends the walk), so at most x steps.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* p, int x) {
    for (;;) {
        const int q = __hip_atomic_load(p + x, __ATOMIC_RELAXED, SCOPE);
        if ((unsigned)q >= (unsigned)x) return x;
        x = q;
    }
}

// union of the sets of a and b: link the larger root under the smaller one with fetch_min, which keeps parent[x] <= x.
// Correct under stale reads and under concurrent unions: find returns SOME member a' of a's set (a stale parent is a value the slot held, and every
// value a slot ever held joins two voxels of one final component). fetch_min(parent[a'], b') returns the slot's true value `old`: old == a' means a'
// was a root and now hangs under b' - done. Otherwise a' had already been linked to old < a' by someone else; the slot now holds min(old, b'), so
// whichever of the links a' - old, a' - b' was dropped is restored by uniting old with b' - the retry.
// Terminates by construction: after the finds a' <= a and b' <= b, a retry continues with old < a', so a + b decreases strictly with every
// retry and is bounded below by 0. Nothing here waits for another thread's progress.
template <int SCOPE>
__device__ __forceinline__ void cc_union(int* p, int a, int b) {
    for (;;) {
        a = cc_find<SCOPE>(p, a);
        b = cc_find<SCOPE>(p, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, SCOPE);
        if ((unsigned)old >= (unsigned)a) return;
        a = old;
    }
}

__global__ __launch_bounds__(CC_TILE) void cc_local(const float* __restrict__ density, float level, CcGrid g, int* __restrict__ parent,
                                                    int* __restrict__ size) {
    __shared__ int lp[CC_TILE];
    const int vol = blockIdx.y, t = threadIdx.x;
    const int tile = blockIdx.x;
    const int x0 = (tile % g.tw) * CC_T, y0 = ((tile / g.tw) % g.th) * CC_T, z0 = (tile / (g.tw * g.th)) * CC_T;
    const int lx = t & (CC_T - 1), ly = (t / CC_T) & (CC_T - 1), lz = t / (CC_T * CC_T);
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    const bool in_vol = x < g.W && y < g.H && z < g.D;
    const long long base = (long long)vol * g.V;
    const int gi = in_vol ? (z * g.H + y) * g.W + x : 0;
    const bool inside = in_vol && density[base + gi] > level;          // NaN compares false: outside
    lp[t] = inside ? t : -1;
    __syncthreads();
    if (inside) {
#pragma unroll
        for (int code = 1; code < 8; ++code) {
            const int ox = code & 1, oy = (code >> 1) & 1, oz = code >> 2;
            if (lx + ox >= CC_T || ly + oy >= CC_T || lz + oz >= CC_T) continue;      // the seam pass owns this edge
            const int nb = t + ox + oy * CC_T + oz * CC_T * CC_T;
            if (lp[nb] < 0) continue;                                                // -1 is never overwritten: a plain read is final
            cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, t, nb);
        }
    }
    __syncthreads();
    if (!in_vol) return;
    if (!inside) {
        parent[base + gi] = -1;
        return;
    }
    const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, t);        // the tile order (lz, ly, lx) is the order of the linear index
    const int rx = r & (CC_T - 1), ry = (r / CC_T) & (CC_T - 1), rz = r / (CC_T * CC_T);
    parent[base + gi] = ((z0 + rz) * g.H + y0 + ry) * g.W + x0 + rx;
    if (r == t) size[base + gi] = 0;
}

__global__ __launch_bounds__(CC_THREADS) void cc_seam(int* parent, CcGrid g) {
    const int vol = blockIdx.y;
    const long long lin64 = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (lin64 >= g.V) return;
    const int lin = (int)lin64;
    const int x = lin % g.W, y = (lin / g.W) % g.H, z = lin / (g.W * g.H);
    const bool bx = (x & (CC_T - 1)) == CC_T - 1, by = (y & (CC_T - 1)) == CC_T - 1, bz = (z & (CC_T - 1)) == CC_T - 1;
    if (!(bx || by || bz)) return;
    int* p = parent + (long long)vol * g.V;
    if (__hip_atomic_load(p + lin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
#pragma unroll
    for (int code = 1; code < 8; ++code) {
        const int ox = code & 1, oy = (code >> 1) & 1, oz = code >> 2;
        if (!((ox && bx) || (oy && by) || (oz && bz))) continue;                     // the neighbour is in this tile: cc_local did it
        if (x + ox >= g.W || y + oy >= g.H || z + oz >= g.D) continue;               // no adjacency across the border, nor across rows
        const int nb = lin + ox + oy * g.W + oz * g.W * g.H;
        if (__hip_atomic_load(p + nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
        cc_union<__HIP_MEMORY_SCOPE_AGENT>(p, lin, nb);
    }
}

// Calls f(mine, group, leader, key) once per distinct key among the wave's valid lanes: mine = this lane carries the key, group = the ballot of
// those lanes, leader = the lowest of them. Every lane of the wave must call it. Each pass clears at least the leader's bit of a wave-uniform
// mask: at most 64 passes, one when the whole wave shares a key. Nothing outside the wave is waited for.
template <class F>
__device__ __forceinline__ void cc_wave_groups(bool valid, int key, F&& f) {
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader, 64);
        const bool mine = valid && key == k;
        const unsigned long long group = __ballot(mine);
        f(mine, group, leader, k);
        todo &= ~group;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten(const int* __restrict__ parent, int* __restrict__ root, int* __restrict__ size,
                                                         int* __restrict__ partial, CcGrid g) {
    __shared__ int wsum[CC_THREADS / 64];
    const int vol = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const long long lin64 = (long long)blockIdx.x * CC_THREADS + tid;
    const long long base = (long long)vol * g.V;
    const int* p = parent + base;
    int r = -1;
    bool is_root = false;
    if (lin64 < g.V) {
        const int lin = (int)lin64;
        int q = p[lin];
        if (q >= 0) {
            is_root = q == lin;
            r = lin;
            while ((unsigned)q < (unsigned)r) {      // strictly smaller index every step: at most lin steps, whatever is loaded
                r = q;
                q = p[r];
            }
        }
        root[base + lin] = r;
    }
    int* sz = size + base;
    cc_wave_groups(r >= 0, r, [&](bool, unsigned long long group, int leader, int k) {
        if (lane == leader) atomicAdd(sz + k, __popcll(group));
    });
    const int c = __popcll(__ballot(is_root));
    if (lane == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < CC_THREADS / 64; ++w) s += wsum[w];
        partial[(long long)vol * g.nblk + blockIdx.x] = s;
    }
}

// partial[vol][0..nblk) -> its exclusive scan in place; counts[vol] = vols[vol].K = the total
__global__ __launch_bounds__(CC_SCAN_THREADS) void cc_scan(int* __restrict__ partial, int nblk, int* __restrict__ counts, CcVol* __restrict__ vols) {
    const int vol = blockIdx.x;
    const int carry = block_exclusive_scan_inplace<int, CC_SCAN_THREADS>(partial + (long long)vol * nblk, nblk);
    if (threadIdx.x == 0) {
        counts[vol] = carry;
        vols[vol].K = carry;
    }
}

// key of a root for the per-volume maximum: larger size first, then the LOWER index
__device__ __forceinline__ unsigned long long cc_key(int size, int index) {
    return (unsigned long long)(unsigned)size << 32 | (unsigned long long)(unsigned)(INT_MAX - index);
}

__global__ __launch_bounds__(CC_THREADS) void cc_rank(const int* __restrict__ root, const int* __restrict__ size, const int* __restrict__ partial,
                                                      int* __restrict__ rank, unsigned long long* __restrict__ pmax, CcGrid g) {
    __shared__ int wsum[CC_THREADS / 64];
    __shared__ unsigned long long wmax[CC_THREADS / 64];
    const int vol = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long lin64 = (long long)blockIdx.x * CC_THREADS + tid;
    const long long base = (long long)vol * g.V;
    const bool is_root = lin64 < g.V && root[base + lin64] == (int)lin64;
    unsigned long long key = is_root ? cc_key(size[base + lin64], (int)lin64) : 0ull;
    const unsigned long long flags = __ballot(is_root);
    const int before_lane = __popcll(flags & ((1ull << lane) - 1ull));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(key, o, 64);
        key = u > key ? u : key;
    }
    if (lane == 0) {
        wsum[wave] = __popcll(flags);
        wmax[wave] = key;
    }
    __syncthreads();
    if (is_root) {
        // the root's own parent slot: the forest is not read again
        rank[base + lin64] = waves_before(wsum, wave, partial[(long long)vol * g.nblk + blockIdx.x] + before_lane);
    }
    if (tid == 0) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int w = 0; w < CC_THREADS / 64; ++w) m = wmax[w] > m ? wmax[w] : m;
        pmax[(long long)vol * g.nblk + blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_labels(const int* __restrict__ root, const int* __restrict__ rank, int* __restrict__ labels, CcGrid g) {
    const long long lin64 = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (lin64 >= g.V) return;
    const long long base = (long long)blockIdx.y * g.V;
    const int r = root[base + lin64];
    labels[base + lin64] = r < 0 ? 0 : rank[base + r] + 1;
}

__global__ __launch_bounds__(CC_THREADS) void cc_stats_init(const CcVol* __restrict__ vols, int kmax, int* __restrict__ sizes, int* __restrict__ bbox,
                                                            long long* __restrict__ coord_sum, int* __restrict__ status) {
    const int vol = blockIdx.y;
    const int K = vols[vol].K;
    const int k = blockIdx.x * CC_THREADS + threadIdx.x;
    if (k == 0) status[vol] = K > kmax ? FORGE_COMPONENTS_OVERFLOW : 0;
    if (k >= kmax) return;
    const long long row = (long long)vol * kmax + k;
    const int lo = k < K ? INT_MAX : 0;
    sizes[row] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        bbox[row * 6 + a] = lo;
        bbox[row * 6 + 3 + a] = 0;
        coord_sum[row * 3 + a] = 0;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_stats(const int* __restrict__ root, const int* __restrict__ rank, const int* __restrict__ size,
                                                       int kmax, int* __restrict__ sizes, int* __restrict__ bbox,
                                                       unsigned long long* __restrict__ coord_sum, CcGrid g) {
    const int vol = blockIdx.y, lane = threadIdx.x & 63;
    const long long lin64 = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    const long long base = (long long)vol * g.V;
    int k = -1, c[3] = {0, 0, 0};
    if (lin64 < g.V) {
        const int lin = (int)lin64;
        const int r = root[base + lin];
        if (r >= 0) {
            k = rank[base + r];
            if (k >= kmax) k = -1;                   // past the capacity: the rows that fit are the first kmax components
            else if (r == lin) sizes[(long long)vol * kmax + k] = size[base + lin];
        }
        c[0] = lin % g.W;
        c[1] = (lin / g.W) % g.H;
        c[2] = lin / (g.W * g.H);
    }
    cc_wave_groups(k >= 0, k, [&](bool mine, unsigned long long, int leader, int kk) {
        unsigned long long s[3];
        int lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[a] = mine ? (unsigned long long)c[a] : 0ull;
            lo[a] = mine ? c[a] : INT_MAX;
            hi[a] = mine ? c[a] : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s[a] += __shfl_xor(s[a], o, 64);
                lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64));
                hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64));
            }
        if (lane == leader) {
            const long long row = (long long)vol * kmax + kk;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicAdd(coord_sum + row * 3 + a, s[a]);
                atomicMin(bbox + row * 6 + a, lo[a]);
                atomicMax(bbox + row * 6 + 3 + a, hi[a]);
            }
        }
    });
}

// thr = ceil(min_fraction * L) in float64: L < 2^31 converts exactly, the product is rounded once (IEEE multiply), ceil is exact
__global__ __launch_bounds__(CC_SCAN_THREADS) void cc_winner(const unsigned long long* __restrict__ pmax, int nblk, double min_fraction,
                                                             CcVol* __restrict__ vols) {
    __shared__ unsigned long long wmax[CC_SCAN_THREADS / 64];
    const int vol = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const unsigned long long* p = pmax + (long long)vol * nblk;
    unsigned long long key = 0ull;
    for (int i = tid; i < nblk; i += CC_SCAN_THREADS) key = p[i] > key ? p[i] : key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(key, o, 64);
        key = u > key ? u : key;
    }
    if (lane == 0) wmax[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int w = 0; w < CC_SCAN_THREADS / 64; ++w) m = wmax[w] > m ? wmax[w] : m;
        const int L = (int)(unsigned)(m >> 32);
        vols[vol].L = L;
        vols[vol].winner = L > 0 ? INT_MAX - (int)(unsigned)(m & 0xffffffffull) : -1;
        vols[vol].thr = (int)ceil(min_fraction * (double)L);
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_select(const unsigned* __restrict__ density, const int* __restrict__ root, const int* __restrict__ size,
                                                        const CcVol* __restrict__ vols, int keep_largest, int min_voxels, unsigned* __restrict__ out,
                                                        CcGrid g) {
    const long long lin64 = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (lin64 >= g.V) return;
    const int vol = blockIdx.y;
    const long long at = (long long)vol * g.V + lin64;
    const unsigned bits = density[at];               // moved as bits: NaN payloads and signed zeros survive
    const int r = root[at];
    bool keep = true;
    if (r >= 0) {
        const CcVol v = vols[vol];
        const int s = size[(long long)vol * g.V + r];
        keep = s >= min_voxels && s >= v.thr && (!keep_largest || r == v.winner);
    }
    out[at] = keep ? bits : 0u;
}

// workspace of n volumes: parent / rank [n][V] int32 | root [n][V] int32 | size [n][V] int32 | partial [n][nblk] int32 | pmax [n][nblk] uint64 |
// vols [n] CcVol
static int cc_grid(int n, int D, int H, int W, CcGrid& g, long long (&off)[7], const char* fn) {
    const int rc = volume_dims_ok(fn, n, D, H, W, 0, 0x7fffffffll - 1);      // voxels: indices are 32-bit, below 2^31 - 1
    if (rc != 0) return rc;
    const long long V = (long long)D * H * W;
    g.D = D; g.H = H; g.W = W;
    g.V = (int)V;
    g.nblk = (int)((V + CC_THREADS - 1) / CC_THREADS);
    g.tw = (W - 1) / CC_T + 1;                  // extents are >= 1; W + CC_T - 1 would overflow for W near 2^31
    g.th = (H - 1) / CC_T + 1;
    g.ntile = g.tw * g.th * ((D - 1) / CC_T + 1);
    ws_layout({(long long)n * V * 4, (long long)n * V * 4, (long long)n * V * 4, (long long)n * g.nblk * 4, (long long)n * g.nblk * 8,
               (long long)n * (long long)sizeof(CcVol)},
              off);
    return 0;
}

}  // namespace forge

extern "C" int forge_components_tile(void) { return forge::CC_T; }

extern "C" long long forge_components_workspace_bytes(int n, int D, int H, int W) {
    using namespace forge;
    CcGrid g;
    long long off[7];
    const int rc = cc_grid(n, D, H, W, g, off, "forge_components_workspace_bytes");
    return rc != 0 ? (long long)rc : off[6];
}

extern "C" int forge_components_label(const float* density, int n, int D, int H, int W, float level, void* workspace, long long workspace_bytes,
                                      int* labels, int* counts, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(density && workspace && counts, FORGE_EINVAL, "forge_components_label: null pointer");
    FORGE_REQUIRE(level_ok(level), FORGE_EINVAL, "forge_components_label: level=%g must be finite and > 0", (double)level);
    CcGrid g;
    long long off[7];
    int rc = cc_grid(n, D, H, W, g, off, "forge_components_label");
    if (rc != 0) return rc;
    rc = workspace_ok("forge_components_label", workspace, workspace_bytes, off[6]);
    if (rc != 0) return rc;
    char* ws = (char*)workspace;
    int* parent = (int*)(ws + off[0]);
    int* root = (int*)(ws + off[1]);
    int* size = (int*)(ws + off[2]);
    int* partial = (int*)(ws + off[3]);
    unsigned long long* pmax = (unsigned long long*)(ws + off[4]);
    CcVol* vols = (CcVol*)(ws + off[5]);
    hipStream_t s = (hipStream_t)stream;
    const dim3 lin(g.nblk, n);
    hipLaunchKernelGGL(cc_local, dim3(g.ntile, n), dim3(CC_TILE), 0, s, density, level, g, parent, size);
    FORGE_LAUNCH_CHECK("forge_components_label (local)");
    hipLaunchKernelGGL(cc_seam, lin, dim3(CC_THREADS), 0, s, parent, g);
    FORGE_LAUNCH_CHECK("forge_components_label (seam)");
    hipLaunchKernelGGL(cc_flatten, lin, dim3(CC_THREADS), 0, s, parent, root, size, partial, g);
    FORGE_LAUNCH_CHECK("forge_components_label (flatten)");
    hipLaunchKernelGGL(cc_scan, dim3(n), dim3(CC_SCAN_THREADS), 0, s, partial, g.nblk, counts, vols);
    FORGE_LAUNCH_CHECK("forge_components_label (scan)");
    hipLaunchKernelGGL(cc_rank, lin, dim3(CC_THREADS), 0, s, root, size, partial, parent, pmax, g);
    FORGE_LAUNCH_CHECK("forge_components_label (rank)");
    if (labels != nullptr) {
        hipLaunchKernelGGL(cc_labels, lin, dim3(CC_THREADS), 0, s, root, parent, labels, g);
        FORGE_LAUNCH_CHECK("forge_components_label (labels)");
    }
    return 0;
}

extern "C" int forge_components_stats(const void* workspace, long long workspace_bytes, int n, int D, int H, int W, int max_components, int* sizes,
                                      int* bbox, long long* coord_sum, int* status, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(workspace && status, FORGE_EINVAL, "forge_components_stats: null pointer");
    FORGE_REQUIRE(max_components >= 0, FORGE_EINVAL, "forge_components_stats: max_components=%d must not be negative", max_components);
    FORGE_REQUIRE((sizes && bbox && coord_sum) || max_components == 0, FORGE_EINVAL, "forge_components_stats: null sizes / bbox / coord_sum with max_components=%d",
                  max_components);
    CcGrid g;
    long long off[7];
    int rc = cc_grid(n, D, H, W, g, off, "forge_components_stats");
    if (rc != 0) return rc;
    rc = workspace_ok("forge_components_stats", workspace, workspace_bytes, off[6]);
    if (rc != 0) return rc;
    FORGE_REQUIRE((long long)n * max_components <= 0x7fffffffll, FORGE_ESHAPE, "forge_components_stats: n * max_components beyond 2^31 - 1 rows");
    FORGE_REQUIRE(((unsigned long long)coord_sum & 7ull) == 0, FORGE_EINVAL, "forge_components_stats: coord_sum must be 8-byte aligned");
    const char* ws = (const char*)workspace;
    const int* rank = (const int*)(ws + off[0]);
    const int* root = (const int*)(ws + off[1]);
    const int* size = (const int*)(ws + off[2]);
    const CcVol* vols = (const CcVol*)(ws + off[5]);
    hipStream_t s = (hipStream_t)stream;
    const int kblk = max_components > 0 ? (max_components + CC_THREADS - 1) / CC_THREADS : 1;
    hipLaunchKernelGGL(cc_stats_init, dim3(kblk, n), dim3(CC_THREADS), 0, s, vols, max_components, sizes, bbox, coord_sum, status);
    FORGE_LAUNCH_CHECK("forge_components_stats (init)");
    if (max_components > 0) {
        hipLaunchKernelGGL(cc_stats, dim3(g.nblk, n), dim3(CC_THREADS), 0, s, root, rank, size, max_components, sizes, bbox,
                           (unsigned long long*)coord_sum, g);
        FORGE_LAUNCH_CHECK("forge_components_stats (accumulate)");
    }
    return 0;
}

extern "C" int forge_components_select(const float* density, int n, int D, int H, int W, void* workspace, long long workspace_bytes, int keep_largest,
                                       int min_voxels, double min_fraction, float* out, forge_stream_t stream) {
    using namespace forge;
    FORGE_REQUIRE(density && workspace && out, FORGE_EINVAL, "forge_components_select: null pointer");
    FORGE_REQUIRE(keep_largest == 0 || keep_largest == 1, FORGE_EINVAL, "forge_components_select: keep_largest=%d must be 0 or 1", keep_largest);
    FORGE_REQUIRE(min_voxels >= 1, FORGE_EINVAL, "forge_components_select: min_voxels=%d must be >= 1", min_voxels);
    FORGE_REQUIRE(min_fraction >= 0.0 && min_fraction <= 1.0, FORGE_EINVAL, "forge_components_select: min_fraction=%g must lie in [0, 1]", min_fraction);
    CcGrid g;
    long long off[7];
    int rc = cc_grid(n, D, H, W, g, off, "forge_components_select");
    if (rc != 0) return rc;
    rc = workspace_ok("forge_components_select", workspace, workspace_bytes, off[6]);
    if (rc != 0) return rc;
    char* ws = (char*)workspace;
    const int* root = (const int*)(ws + off[1]);
    const int* size = (const int*)(ws + off[2]);
    const unsigned long long* pmax = (const unsigned long long*)(ws + off[4]);
    CcVol* vols = (CcVol*)(ws + off[5]);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_winner, dim3(n), dim3(CC_SCAN_THREADS), 0, s, pmax, g.nblk, min_fraction, vols);
    FORGE_LAUNCH_CHECK("forge_components_select (winner)");
    hipLaunchKernelGGL(cc_select, dim3(g.nblk, n), dim3(CC_THREADS), 0, s, (const unsigned*)density, root, size, vols, keep_largest, min_voxels,
                       (unsigned*)out, g);
    FORGE_LAUNCH_CHECK("forge_components_select (select)");
    return 0;
}
