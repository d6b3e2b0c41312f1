"""The mesh-extraction contract (include/forge_hip.h section g1) restated in numpy, and the density fields the mesh tests run on.

reference_mesh is fed the same float32 volumes as the kernels and computes in float64 (dtype=np.float32 reruns the same formulas in fp32: that
is how the normals' tolerance is measured). It keeps no case table of its own: `table()` reads the one in csrc/mesh.hip through
forge_mesh_case_table (host only, no device). Used by tests/test_mesh_cpu.py and tests/test_gpu_mesh.py."""
import math

import numpy as np

R0 = math.sqrt(0.08 * math.log(3.0))          # radius of the blob's 0.5 level set: 1.5 exp(-r^2 / 0.08) = 0.5


def table():
    from forge_amd import ops
    return ops.mesh_case_table()


# ------------------------------------------------------------------------------------------------------------------------------ fields
def world_axis(N, volume_size=1.0):
    """Voxel-centre world coordinates of an axis of N samples: (2 i / (N - 1) - 1) e, e = 0.5 (N - 1) volume_size / N."""
    return (np.arange(N, dtype=np.float64) - 0.5 * (N - 1)) * (volume_size / N)


def world_grid(D, H, W, volume_size=1.0):
    return np.meshgrid(world_axis(D, volume_size), world_axis(H, volume_size), world_axis(W, volume_size), indexing="ij")     # Z, Y, X


def blob(D, center=(0.0, 0.0, 0.0)):
    """1.5 exp(-|x - c|^2 / 0.08) on the voxel-centre world grid; center = (x, y, z)."""
    Z, Y, X = world_grid(D, D, D)
    r2 = (X - center[0]) ** 2 + (Y - center[1]) ** 2 + (Z - center[2]) ** 2
    return (1.5 * np.exp(-r2 / 0.08)).astype(np.float32)


ELLIPSOID_RADII = (0.40, 0.30, 0.20)           # along x, y, z


def ellipsoid(D):
    """Level 0.5 at (x / 0.40)^2 + (y / 0.30)^2 + (z / 0.20)^2 = 1: density = 1.5 - q, clamped at 0. Three radii: pins the axis order."""
    Z, Y, X = world_grid(D, D, D)
    q = (X / ELLIPSOID_RADII[0]) ** 2 + (Y / ELLIPSOID_RADII[1]) ** 2 + (Z / ELLIPSOID_RADII[2]) ** 2
    return np.maximum(1.5 - q, 0.0).astype(np.float32)


def torus(D):
    """Level 0.5 on the torus of major radius 0.28 (in the x-y plane) and minor radius 0.12: density = 1.5 exp(-s^2 ln 3 / 0.12^2),
    s the distance to the centre circle."""
    Z, Y, X = world_grid(D, D, D)
    s2 = (np.sqrt(X ** 2 + Y ** 2) - 0.28) ** 2 + Z ** 2
    return (1.5 * np.exp(-s2 * math.log(3.0) / 0.12 ** 2)).astype(np.float32)


def ones(D):
    return np.ones((D, D, D), np.float32)


QUANT_LEVEL = 33.0 / 128.0


def quantised(shape, seed):
    """Multiples of 1/64 in [0, 1) from a seeded generator, for level 33/128: no sample equals the level, every t is exact-ish and ties in
    `d > level` cannot depend on rounding."""
    return (np.random.default_rng(seed).integers(0, 64, size=shape).astype(np.float32) / np.float32(64.0)).astype(np.float32)


def noncubic(seed=7):
    return quantised((6, 5, 7), seed)          # D, H, W all different


def below(D):
    return np.full((D, D, D), 0.25, np.float32)


def random_features(C, shape, seed):
    return np.random.default_rng(seed).standard_normal((C,) + tuple(shape)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------- the restatement
class RefMesh:
    def __init__(self, vertices, normals, faces, features, grad_norm, grad_end_norm, feat_scale):
        self.vertices, self.normals, self.faces, self.features = vertices, normals, faces, features
        self.grad_norm = grad_norm             # |lerp(g_a, g_b, t)| per vertex
        self.grad_end_norm = grad_end_norm     # max(|g_a|, |g_b|) per vertex
        self.feat_scale = feat_scale           # |f_a| + |f_b| per vertex and channel (None without features)


def reference_mesh(density, level=0.5, volume_size=1.0, features=None, dtype=np.float64, tab=None):
    """density [D,H,W] float32, features [C,D,H,W] float32 or None -> RefMesh, in the contract's order."""
    tab = tab or table()
    dens = np.asarray(density)
    assert dens.dtype == np.float32 and dens.ndim == 3
    D, H, W = dens.shape
    lvl32 = np.float32(level)
    F = np.zeros((D + 4, H + 4, W + 4), np.float32)            # index i of the contract sits at i + 2: covers -2 .. N+1
    F[2:D + 2, 2:H + 2, 2:W + 2] = dens
    inside = F > lvl32                                         # strict, an fp32 compare
    Fw = F.astype(dtype)
    lvl = dtype(lvl32)
    Ns = (W, H, D)                                             # per emitted axis x, y, z
    ext = [dtype(0.5) * dtype(N - 1) * dtype(volume_size) / dtype(N) for N in Ns]
    den = [dtype(max(N - 1, 1)) for N in Ns]
    Cf = None
    if features is not None:
        Cf = np.zeros((features.shape[0], D + 4, H + 4, W + 4), dtype)
        Cf[:, 2:D + 2, 2:H + 2, 2:W + 2] = features

    def f(p):                                                  # p = (x, y, z) grid index
        return Fw[p[2] + 2, p[1] + 2, p[0] + 2]

    def ins(p):
        return bool(inside[p[2] + 2, p[1] + 2, p[0] + 2])

    def grad(p):
        g = np.zeros(3, dtype)
        for a in range(3):
            hi, lo = list(p), list(p)
            hi[a] += 1
            lo[a] -= 1
            g[a] = (f(hi) - f(lo)) * dtype(Ns[a])
        return g

    def offs(code):
        return (code & 1, (code >> 1) & 1, (code >> 2) & 1)

    # cells with both inside and outside corners
    c8 = np.zeros((D + 1, H + 1, W + 1), np.int32)
    for code in range(8):
        ox, oy, oz = offs(code)
        c8 += inside[1 + oz:D + 2 + oz, 1 + oy:H + 2 + oy, 1 + ox:W + 2 + ox].astype(np.int32)
    active = np.argwhere((c8 > 0) & (c8 < 8))                  # z-major = ascending linear index

    Hc, Wc = H + 1, W + 1
    vindex, verts, norms, feats, gn, gen, fscale = {}, [], [], [], [], [], []
    for cz, cy, cx in active:
        p0 = (cx - 1, cy - 1, cz - 1)
        lin = (cz * Hc + cy) * Wc + cx
        for k in range(7):
            o = offs(k + 1)
            p1 = (p0[0] + o[0], p0[1] + o[1], p0[2] + o[2])
            if ins(p0) == ins(p1):
                continue
            a, b = (p0, p1) if ins(p0) else (p1, p0)
            t = (lvl - f(a)) / (f(b) - f(a))
            pos = [((dtype(2) * (dtype(a[ax]) + dtype(b[ax] - a[ax]) * t)) / den[ax] - dtype(1)) * ext[ax] for ax in range(3)]
            ga, gb = grad(a), grad(b)
            g = ga + t * (gb - ga)
            ln = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
            vindex[(lin, k)] = len(verts)
            verts.append(pos)
            norms.append(-g / ln if ln > 0 else np.zeros(3, dtype))
            gn.append(float(ln))
            gen.append(float(max(np.sqrt((ga.astype(np.float64) ** 2).sum()), np.sqrt((gb.astype(np.float64) ** 2).sum()))))
            if Cf is not None:
                fa, fb = Cf[:, a[2] + 2, a[1] + 2, a[0] + 2], Cf[:, b[2] + 2, b[1] + 2, b[0] + 2]
                feats.append(fa + t * (fb - fa))
                fscale.append(np.abs(fa) + np.abs(fb))

    faces = []
    for cz, cy, cx in active:
        p0 = (cx - 1, cy - 1, cz - 1)
        for q in range(6):
            corner = tab["tet_corner"][q]
            pts = [tuple(p0[ax] + offs(c)[ax] for ax in range(3)) for c in corner]
            case = sum(1 << i for i in range(4) if ins(pts[i]))
            for tr in range(tab["case_ntri"][case]):
                tri = []
                for e in tab["case_tri"][case][tr]:
                    i, j = tab["tet_edge"][e]
                    oi = offs(corner[i])
                    owner = ((cz + oi[2]) * Hc + cy + oi[1]) * Wc + cx + oi[0]
                    tri.append(vindex[(owner, (corner[j] ^ corner[i]) - 1)])
                if tab["tet_flip"][q]:
                    tri = [tri[0], tri[2], tri[1]]
                faces.append(tri)
    C = 0 if features is None else features.shape[0]
    return RefMesh(np.array(verts, dtype).reshape(-1, 3), np.array(norms, dtype).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3),
                   None if features is None else np.array(feats, dtype).reshape(-1, C), np.array(gn), np.array(gen),
                   None if features is None else np.array(fscale, np.float64).reshape(-1, C))


# -------------------------------------------------------------------------------------------------------------------- mesh properties
def directed_edges_paired(faces):
    """Every directed edge occurs exactly once and its reverse exactly once."""
    f = np.asarray(faces, np.int64)
    if f.size == 0:
        return True
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e[:, 0] * (f.max() + 1) + e[:, 1]
    rev = e[:, 1] * (f.max() + 1) + e[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))


def euler_characteristic(n_vertices, faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return int(n_vertices) - len(np.unique(e, axis=0)) + len(f)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def index_positions(vertices, shape, volume_size=1.0):
    """World positions back to index units per axis (x, y, z) <-> (W, H, D)."""
    D, H, W = shape
    v = np.asarray(vertices, np.float64)
    return np.stack([v[:, a] / (volume_size / N) + 0.5 * (N - 1) for a, N in enumerate((W, H, D))], axis=1)
