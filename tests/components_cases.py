"""The connected-components contract (include/forge_hip.h section g4) restated in plain numpy, and the density fields the component tests run on.

reference_labels is a sequential union-find over the 7 positive directions (offset codes 1..7 of the mesh case table: bit 0 = +x, bit 1 = +y,
bit 2 = +z); everything else - statistics, centroid, the selection rule, the cleaned volume - follows from its labels in integer or float64
arithmetic. No scipy. Used by tests/test_components_cpu.py and tests/test_gpu_components.py; every field is built once and never modified."""
import functools
import itertools
import math

import numpy as np

import mesh_cases as mc

DIRECTIONS = tuple((code & 1, (code >> 1) & 1, code >> 2) for code in range(1, 8))          # (dx, dy, dz) of offset codes 1..7
INT_MAX = 2 ** 31 - 1


def tile():
    """T, the tile edge of the kernels (forge_components_tile, host only)."""
    from forge_amd import ops
    return ops.components_tile()


# ----------------------------------------------------------------------------------------------------------------------- the restatement
def reference_labels(density, level):
    """density [D,H,W] float32 -> labels [D,H,W] int32: 0 outside, 1..K inside, components numbered by their lowest linear index."""
    d = np.asarray(density)
    assert d.dtype == np.float32 and d.ndim == 3
    D, H, W = d.shape
    inside = d > np.float32(level)                                  # strict, fp32; NaN compares false
    flat = inside.ravel()
    idx = np.flatnonzero(flat).tolist()
    parent = {i: i for i in idx}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for lin in idx:
        x, y, z = lin % W, (lin // W) % H, lin // (W * H)
        for dx, dy, dz in DIRECTIONS:
            if x + dx >= W or y + dy >= H or z + dz >= D:
                continue
            nb = lin + dx + dy * W + dz * W * H
            if not flat[nb]:
                continue
            a, b = find(lin), find(nb)
            if a != b:
                parent[max(a, b)] = min(a, b)                       # a root is its component's lowest index
    labels = np.zeros(D * H * W, np.int32)
    number = {}
    for lin in idx:                                                 # ascending: roots come up in label order
        r = find(lin)
        if r not in number:
            assert r == lin
            number[r] = len(number) + 1
        labels[lin] = number[r]
    return labels.reshape(D, H, W)


class Stats:
    def __init__(self, labels):
        K = int(labels.max())
        z, y, x = np.nonzero(labels)
        k = labels[z, y, x].astype(np.int64) - 1
        self.count = K
        self.sizes = np.bincount(k, minlength=K).astype(np.int32)
        self.bbox = np.zeros((K, 6), np.int32)
        self.bbox[:, :3] = INT_MAX
        self.coord_sum = np.zeros((K, 3), np.int64)
        for a, c in enumerate((x, y, z)):
            np.minimum.at(self.bbox[:, a], k, c.astype(np.int32))
            np.maximum.at(self.bbox[:, 3 + a], k, c.astype(np.int32))
            np.add.at(self.coord_sum[:, a], k, c.astype(np.int64))


def reference_centroid(coord_sum, sizes, shape, volume_size=1.0):
    """float64 [K,3] (x, y, z): mesh_cases.world_axis's formula at the mean index, (sum / size - 0.5 (N - 1)) (volume_size / N); rows of size 0: 0."""
    D, H, W = shape
    out = np.zeros(coord_sum.shape, np.float64)
    for a, N in enumerate((W, H, D)):
        nz = sizes > 0
        out[nz, a] = (coord_sum[nz, a].astype(np.float64) / sizes[nz].astype(np.float64) - 0.5 * (N - 1)) * (volume_size / N)
    return out


def kept_components(sizes, keep="largest", min_voxels=1, min_fraction=0.0):
    """0-based component indices the selection keeps."""
    if len(sizes) == 0:
        return []
    L = int(sizes.max())
    thr = math.ceil(float(min_fraction) * float(L))                 # float64: one rounding in the product, ceil exact
    passing = [k for k, s in enumerate(sizes.tolist()) if s >= min_voxels and s >= thr]
    if keep == "all" or not passing:
        return passing
    assert keep == "largest"
    return [max(passing, key=lambda k: (sizes[k], -k))]


def reference_clean(density, level, keep="largest", min_voxels=1, min_fraction=0.0):
    labels = reference(density, level)[0]
    kept = np.array(kept_components(reference(density, level)[1].sizes, keep, min_voxels, min_fraction), np.int64) + 1
    out = np.array(density, np.float32, copy=True)
    out[(labels > 0) & ~np.isin(labels, kept)] = np.float32(0.0)
    return out


_REF = {}


def reference(density, level):
    """(labels, Stats) of a field, computed once per (array, level): the fields of this module are module-level constants."""
    key = (id(density), float(level))
    if key not in _REF:
        labels = reference_labels(density, level)
        _REF[key] = (labels, Stats(labels), density)                # the array is held, so its id stays its own
    return _REF[key][:2]


# ------------------------------------------------------------------------------------------------------------------------------ fields
class Field:
    """name, density [D,H,W] float32, level, K (the known answer, or None) and, where known, the sizes in label order."""

    def __init__(self, name, density, level, K=None, sizes=None):
        self.name, self.density, self.level, self.K, self.sizes = name, np.ascontiguousarray(density, np.float32), float(level), K, sizes
        self.density.setflags(write=False)

    @property
    def shape(self):
        return self.density.shape


def binary(mask):
    return np.where(mask, np.float32(1.0), np.float32(0.0)).astype(np.float32)


def from_mask(mask, seed):
    """Quantised values (mesh_cases.quantised, level QUANT_LEVEL = 16.5 / 64): inside voxels draw from 17/64 .. 63/64, outside ones from 0 .. 16/64."""
    q = np.rint(mc.quantised(mask.shape, seed) * 64.0).astype(np.int64)
    return (np.where(mask, 17 + q % 47, q % 17).astype(np.float32) / np.float32(64.0)).astype(np.float32)


def direction_representatives():
    """The 13 directions (dx, dy, dz) up to sign, the first non-zero component positive."""
    out = []
    for d in itertools.product((-1, 0, 1), repeat=3):
        nz = [c for c in d if c]
        if nz and nz[0] > 0:
            out.append(d)
    assert len(out) == 13
    return out


def same_sign(d):
    return all(c >= 0 for c in d) or all(c <= 0 for c in d)


def two_voxels(d):
    m = np.zeros((3, 3, 3), bool)
    m[1, 1, 1] = True
    m[1 + d[2], 1 + d[1], 1 + d[0]] = True
    return Field("two_voxels%+d%+d%+d" % d, binary(m), 0.5, 1 if same_sign(d) else 2)


def row_wrap():
    m = np.zeros((2, 3, 5), bool)
    m[1, 0, 4] = m[1, 1, 0] = True                                  # linear neighbours, not lattice neighbours
    return Field("row_wrap", binary(m), 0.5, 2, [1, 1])


def batch_wrap():
    """Two volumes of one batch: the last voxel of the first, the first voxel of the second."""
    a, b = np.zeros((2, 3, 4), bool), np.zeros((2, 3, 4), bool)
    a[-1, -1, -1] = b[0, 0, 0] = True
    return [Field("batch_wrap_last", binary(a), 0.5, 1, [1]), Field("batch_wrap_first", binary(b), 0.5, 1, [1])]


def specials():
    """NaN is outside, +inf is inside, -inf is outside; the NaNs carry payloads the cleaned volume must keep."""
    d = np.zeros((3, 3, 3), np.float32)
    d[0, 0, 0] = np.inf
    d[0, 0, 1] = np.nan
    d[0, 0, 2] = 1.0                                                # separated from +inf by the NaN
    d[1, 1, 1] = -np.inf
    d[2, 2, 2] = 0.75
    d[2, 2, 1] = np.inf
    bits = d.view(np.uint32).copy()
    bits[1, 0, 0] = 0x7fc12345                                      # a quiet NaN with a payload
    bits[1, 0, 1] = 0xffc00001                                      # a negative one
    bits[2, 0, 0] = 0x80000000                                      # -0.0
    return Field("specials", bits.view(np.float32), 0.5, 3, [1, 1, 2])


def snake_mask(D, H, W):
    """One component that walks boustrophedon along the even rows of the even planes, joined at alternating ends: diameter ~ D H W / 4."""
    m = np.zeros((D, H, W), bool)
    rows = list(range(0, H, 2))
    side = 0
    for k, z in enumerate(range(0, D, 2)):
        ys = rows if k % 2 == 0 else rows[::-1]
        for j, y in enumerate(ys):
            m[z, y, :] = True
            side = W - 1 - side
            if j + 1 < len(ys):
                m[z, (y + ys[j + 1]) // 2, side] = True
        if z + 2 < D:
            m[z + 1, ys[-1], side] = True
    return m


def snake(D, H, W):
    return Field("snake%dx%dx%d" % (D, H, W), binary(snake_mask(D, H, W)), 0.5, 1)


def twin_snakes(bridge, D=10, H=9, w=7):
    """Two equal snakes in the two x-halves with the empty column pair x = w, w + 1 between them; the bridge fills that pair in the last even row
    of the last even plane - the far end of both walks - so the two halves meet only there. Without it: two components of equal size."""
    s = snake_mask(D, H, w)
    m = np.zeros((D, H, 2 * w + 2), bool)
    m[:, :, :w] = s
    m[:, :, w + 2:] = s
    if bridge:
        z = (D - 1) // 2 * 2
        y = (H - 1) // 2 * 2 if ((D - 1) // 2) % 2 == 0 else 0
        assert m[z, y, w - 1] and m[z, y, w + 2]
        m[z, y, w:w + 2] = True
    n = int(s.sum())
    return Field("twin_snakes_%s" % ("bridged" if bridge else "apart"), binary(m), 0.5, 1 if bridge else 2, [2 * n + 2] if bridge else [n, n])


RANDOM_SHAPE = (20, 17, 23)
RANDOM_KNOWN = {0.05: (268, 9, 9), 0.1: (355, 17, 17), 0.2: (196, 727, 165), 0.3: (55, 2192, 19)}       # p: K, largest, second (scipy, measured)


RANDOM_P = (0.05, 0.1, 0.15, 0.2, 0.3)


def random_mask(shape, p, seed=0):
    return np.random.default_rng(seed).random(shape) < p


def random_fields():
    """ONE default_rng(0), one draw of RANDOM_SHAPE per p in the order of RANDOM_P: the masks the known answers were measured on."""
    rng = np.random.default_rng(0)
    out = []
    for p in RANDOM_P:
        mask = rng.random(RANDOM_SHAPE) < p
        out.append(Field("random_p%g" % p, from_mask(mask, 100 + int(round(p * 100))), mc.QUANT_LEVEL, RANDOM_KNOWN.get(p, (None,))[0]))
    return out


def blob_floaters():
    d = mc.blob(12, (0.05, -0.03, 0.02)).copy()
    for z, y, x in ((1, 1, 1), (10, 10, 1), (10, 9, 1), (1, 10, 10), (2, 11, 11)):
        d[z, y, x] = 1.0
    return Field("blob_floaters", d, 0.5, 4, [1, 2, 190, 2])


def extent_field(shape, seed):
    return Field("extent%dx%dx%d" % shape, from_mask(random_mask(shape, 0.25, seed), seed), mc.QUANT_LEVEL)


def seam_pairs(T):
    """One two-voxel volume of (T + 3)^3 per direction representative d and per non-empty set of d's axes: the pair straddles the tile seam at
    T - 1 | T on exactly those axes and stays inside the first tile on the others. K = 1 for same-sign d, 2 otherwise. Covers the pairs across a
    tile face, edge and corner along (1,1,0), (1,0,1), (0,1,1), (1,1,1) and along every direction that must NOT connect."""
    out = []
    N = T + 3
    for d in direction_representatives():
        support = [a for a in range(3) if d[a]]
        for r in range(1, len(support) + 1):
            for axes in itertools.combinations(support, r):
                a = [2, 2, 2]
                for ax in axes:
                    a[ax] = T - 1 if d[ax] > 0 else T
                m = np.zeros((N, N, N), bool)
                m[a[2], a[1], a[0]] = True
                m[a[2] + d[2], a[1] + d[1], a[0] + d[0]] = True
                out.append(Field("seam%+d%+d%+d_%s" % (d + ("".join("xyz"[ax] for ax in axes),)), binary(m), 0.5, 1 if same_sign(d) else 2))
    assert len(out) == 49
    return out


@functools.lru_cache(maxsize=None)
def fields():
    """Every field, by name."""
    T = tile()
    out = [two_voxels(d) for d in direction_representatives()]
    out += [row_wrap()] + batch_wrap() + [specials()]
    out += [Field("single", binary(np.ones((1, 1, 1), bool)), 0.5, 1, [1]), Field("all_outside", binary(np.zeros((2, 3, 5), bool)), 0.5, 0, []),
            Field("all_inside", binary(np.ones((33, 9, 8), bool)), 0.5, 1, [33 * 9 * 8])]
    out += [snake(16, 16, 16), snake(9, 7, 17), twin_snakes(True), twin_snakes(False)]
    out += random_fields()
    out += [blob_floaters()]
    shapes = [(1, 1, 1), (1, 1, 40), (2, 3, 5), (7, 8, 9), (9, 7, 17), (17, 33, 15),
              (T - 1, T, T + 1), (T + 1, T - 1, T), (T, T + 1, T - 1), (2 * T + 1, T, T - 1), (T + 1, 2 * T + 1, T), (T, T - 1, 2 * T + 1),
              (2 * T + 1, 2 * T + 1, 2 * T + 1)]
    out += [extent_field(s, 7 + k) for k, s in enumerate(dict.fromkeys(shapes))]
    out += seam_pairs(T)
    names = [f.name for f in out]
    assert len(set(names)) == len(names)
    return {f.name: f for f in out}


@functools.lru_cache(maxsize=None)
def batches():
    """Fields of one shape and level, stacked three to a batch (the last batch of a shape may be shorter): [(names, fields)]. The two batch_wrap
    volumes share a batch, in their order."""
    groups = {}
    for f in fields().values():
        groups.setdefault((f.shape, f.level), []).append(f)
    out = []
    for fs in groups.values():
        for i in range(0, len(fs), 3):
            out.append(tuple(fs[i:i + 3]))
    return tuple(out)


def stack(fs):
    return np.stack([f.density for f in fs])[:, None]                # [n,1,D,H,W]


# ----------------------------------------------------------------------------------------------------------------------- sub-mesh property
def submesh_map(v_full, v_sub):
    """v_sub must be an ordered, bitwise subset of v_full: returns map [len(v_full)] int64, -1 for rows that are not in v_sub."""
    a = np.ascontiguousarray(v_full, np.float32).view(np.uint32).reshape(-1, 3)
    b = np.ascontiguousarray(v_sub, np.float32).view(np.uint32).reshape(-1, 3)
    out = np.full(len(a), -1, np.int64)
    j = 0
    for i in range(len(a)):
        if j < len(b) and (a[i] == b[j]).all():
            out[i] = j
            j += 1
    assert j == len(b), "%d of %d vertices of the cleaned mesh are not in the original, in order" % (len(b) - j, len(b))
    return out


def filtered_faces(f_full, vmap):
    """The faces of the original whose three vertices survive, re-indexed, in their order."""
    f = np.asarray(f_full, np.int64).reshape(-1, 3)
    m = vmap[f]
    keep = (m >= 0).all(axis=1)
    assert ((m >= 0).any(axis=1) == keep).all(), "a face of the original joins a kept vertex to a removed one"
    return m[keep].astype(np.int32)
