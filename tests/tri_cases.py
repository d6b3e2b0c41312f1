"""The point-to-triangle contract (include/forge_hip.h section g3b) restated in numpy, and the cases its tests run on.

  closest64    the float64 restatement: per (query, face) the exact distance T_f, the closest point and the Voronoi region that holds the query;
  second64     an independently written second formulation (plane distance if the projection is inside, else the minimum over the three segments);
  closest32    the header's fp32 expression order, fma by fma (an fp32 fma is the float64 product, exact, plus the addend, rounded twice);
  restate      one pair as the kernel sees it: the transforms applied in the fp32 chain, the candidate faces, T [Nq,F], L [Nq,F], s [F];
  case()       the meshes, face counts, query counts, layouts and transforms of tests/test_gpu_tridist.py, built once, never modified;
  measured_k() K_lo and K_hi: the worst case of closest32 against closest64 over those cases, in the form the tests assert.
Used by tests/test_tridist_cpu.py (no GPU) and tests/test_gpu_tridist.py (the kernels against this)."""
import functools
from collections import namedtuple

import numpy as np

import geom_cases as gc
import mesh_cases as mc

U = gc.U
TILE = 256                                     # forge_nn_tile_faces(); test_tridist_cpu.py checks it against the library
VERTEX_A, VERTEX_B, VERTEX_C, EDGE_AB, EDGE_AC, EDGE_BC, INTERIOR = range(7)
KIND = np.array([0, 0, 0, 1, 1, 1, 2])         # region -> vertex / edge / interior


def _dot(u, v):
    return (u * v).sum(axis=-1)


# ------------------------------------------------------------------------------------------------------------------- the restatements
def closest64(q, a, b, c):
    """q, a, b, c [..., 3] (broadcast against each other), float64 -> (distance, closest point, region). Ericson's closest point on a
    triangle, with his branches in his order."""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    ab, ac = b - a, c - a
    ap, bp, cp = q - a, q - b, q - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    region = np.select(conds, [VERTEX_A, VERTEX_B, EDGE_AB, VERTEX_C, EDGE_AC, EDGE_BC], INTERIOR)
    with np.errstate(invalid="ignore", divide="ignore"):
        tab, tac, tbc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
        pts = [a + 0 * q, b + 0 * q, c + 0 * q, a + tab[..., None] * ab, a + tac[..., None] * ac, b + tbc[..., None] * (c - b),
               a + (vb * den)[..., None] * ab + (vc * den)[..., None] * ac]
    p = np.select([(region == k)[..., None] for k in range(6)], pts[:6], pts[6])
    return np.sqrt(_dot(q - p, q - p)), p, region


def _segment64(q, a, b):
    ab = b - a
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.clip(_dot(q - a, ab) / _dot(ab, ab), 0.0, 1.0)
    r = q - (a + t[..., None] * ab)
    return np.sqrt(_dot(r, r))


def second64(q, a, b, c):
    """The same distance from a different construction: project onto the plane; inside (the three edge functions agree in sign with the normal):
    the plane distance; otherwise the nearest of the three segments."""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = _dot(q - a, n) / nn
    p = q - h[..., None] * n
    inside = (_dot(np.cross(b - a, p - a), n) >= 0) & (_dot(np.cross(c - b, p - b), n) >= 0) & (_dot(np.cross(a - c, p - c), n) >= 0)
    seg = np.minimum(np.minimum(_segment64(q, a, b), _segment64(q, b, c)), _segment64(q, c, a))
    return np.where(inside, np.abs(h) * np.sqrt(nn), seg)


def fma32(a, b, c):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def xf32(p, xf):
    """The fp32 fma chain of section g3 applied to p [..., 3] float32: x' = fma(m02, z, fma(m01, y, fma(m00, x, t0)))."""
    p = np.asarray(p, np.float32)
    if xf is None:
        return p
    m = np.asarray(xf, np.float32).reshape(3, 4)
    return np.stack([fma32(m[r, 2], p[..., 2], fma32(m[r, 1], p[..., 1], fma32(m[r, 0], p[..., 0], m[r, 3]))) for r in range(3)], axis=-1)


def _dot32(u, v):
    return fma32(u[..., 2], v[..., 2], fma32(u[..., 1], v[..., 1], u[..., 0] * v[..., 0]))


def closest32(q, a, b, c):
    """The header's order in fp32 (numpy float32 arithmetic rounds every operation to nearest, as the device does; the reciprocal is a true
    division here) -> (d2 float32, P float32 relative to the query, region)."""
    q, a, b, c = (np.asarray(x, np.float32) for x in (q, a, b, c))
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A, B, C = a - q, b - q, c - q
        ab, ac = B - A, C - A
        n1, n2, n3, n4, n5, n6 = _dot32(ab, A), _dot32(ac, A), _dot32(ab, B), _dot32(ac, B), _dot32(ab, C), _dot32(ac, C)
        vc, vb, va = fma32(n1, n4, -(n3 * n2)), fma32(n5, n2, -(n1 * n6)), fma32(n3, n6, -(n5 * n4))
        t34, t65 = n3 - n4, n6 - n5
        conds = [(n1 >= 0) & (n2 >= 0), (n3 <= 0) & (n4 >= n3), (vc <= 0) & (n1 <= 0) & (n3 >= 0), (n6 <= 0) & (n5 >= n6),
                 (vb <= 0) & (n2 <= 0) & (n6 >= 0), (va <= 0) & (t34 >= 0) & (t65 >= 0)]
        region = np.select(conds, [VERTEX_A, VERTEX_B, EDGE_AB, VERTEX_C, EDGE_AC, EDGE_BC], INTERIOR)
        z, o = zero * n1, zero * n1 + one
        vn = np.select(conds, [z, o, n1, z, z, t65], vb)
        wn = np.select(conds, [z, z, z, o, n2, t34], vc)
        den = np.select(conds, [o, o, n1 - n3, o, n2 - n6, t34 + t65], (va + vb) + vc)
        r = one / den
        v, w = (vn * r)[..., None], (wn * r)[..., None]
        P = fma32(w, ac, fma32(v, ab, A))
        d2 = fma32(P[..., 2], P[..., 2], fma32(P[..., 1], P[..., 1], P[..., 0] * P[..., 0]))
    return d2, P, region


Restated = namedtuple("Restated", "q a b c cand T region L s")


def min_angle_sine(a, b, c):
    """sine of the smallest angle of each face (float64); 0 for a face without area."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    la, lb, lc = np.linalg.norm(c - b, axis=-1), np.linalg.norm(a - c, axis=-1), np.linalg.norm(b - a, axis=-1)      # sides opposite a, b, c
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=-1)
    lo = np.minimum(np.minimum(la, lb), lc)
    with np.errstate(invalid="ignore", divide="ignore"):
        # the smallest angle is opposite the shortest side; sin = 2 A / (product of the two other sides)
        s = area2 * lo / (la * lb * lc)
    return np.where(area2 > 0, s, 0.0)


def restate(q, v, f, nf=None, xf_q=None, xf_mesh=None):
    """One pair as the kernel scores it: q [Nq,3], v [V,3] float32, f [F,3] int -> Restated. q', a, b, c carry the fp32 transforms (float64
    arrays of fp32 values); cand [F] marks the candidate faces (indices in range and float64 area of the UNtransformed corners not 0);
    T [Nq,F] the exact distance to each face (inf for a face that is no candidate), region [Nq,F], L [Nq,F] the largest corner distance from
    the query, s [F] the sine of the smallest angle."""
    v = np.asarray(v, np.float32)
    f = np.asarray(f, np.int64)[:len(f) if nf is None else nf]
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    cand = ok & (gc.face_areas(v, f) != 0.0)
    fs = np.where(ok[:, None], f, 0)
    vt = xf32(v, xf_mesh).astype(np.float64)
    a, b, c = vt[fs[:, 0]], vt[fs[:, 1]], vt[fs[:, 2]]
    q64 = xf32(q, xf_q).astype(np.float64)
    T, _, region = closest64(q64[:, None, :], a[None], b[None], c[None])
    T = np.where(cand[None, :], T, np.inf)
    L = np.maximum(np.maximum(np.linalg.norm(a[None] - q64[:, None], axis=2), np.linalg.norm(b[None] - q64[:, None], axis=2)),
                   np.linalg.norm(c[None] - q64[:, None], axis=2))
    return Restated(q64, a, b, c, cand, T, region, L, min_angle_sine(a, b, c))


def scored32(r):
    """closest32 over a Restated pair -> d [Nq,F] float64 = sqrt(d2_f), NaN where the face is no candidate (it never wins)."""
    d2, _, _ = closest32(r.q[:, None, :], r.a[None], r.b[None], r.c[None])
    with np.errstate(invalid="ignore"):
        return np.where(r.cand[None, :], np.sqrt(d2.astype(np.float64)), np.nan)


def winner(d):
    """The kernel's rule on a [Nq,F] matrix of distances: the first minimum among the values that are not NaN -> (value, face), (inf, -1)
    without one."""
    if d.shape[1] == 0:
        return np.full(len(d), np.inf), np.full(len(d), -1)
    clean = np.where(np.isnan(d), np.inf, d)
    face = clean.argmin(axis=1)
    val = clean[np.arange(len(d)), face]
    return val, np.where(np.isfinite(val), face, -1)


def bounds(r, k_lo, k_hi):
    """The two-sided contract of one pair -> (lower [Nq], upper [Nq], per-face slack [Nq,F] = k_hi u L / s^2). Queries without a candidate:
    lower = upper = inf."""
    Nq, F = r.T.shape
    if F == 0 or not r.cand.any():
        return np.full(Nq, np.inf), np.full(Nq, np.inf), np.zeros((Nq, F))
    with np.errstate(divide="ignore", invalid="ignore"):
        slack = np.where(r.cand[None, :], k_hi * U * r.L / (r.s ** 2)[None, :], np.inf)
    fstar = r.T.argmin(axis=1)
    rows = np.arange(Nq)
    return r.T[rows, fstar] - k_lo * U * r.L[rows, fstar], (r.T + slack).min(axis=1), slack


# ----------------------------------------------------------------------------------------------------------------------------- meshes
def right_triangle():
    """Small-integer corners: a = (0,0,0), b = (4,0,0), c = (0,2,0); |ab x ac|^2 = 64."""
    return np.array([[0, 0, 0], [4, 0, 0], [0, 2, 0]], np.float32), np.array([[0, 1, 2]], np.int32)


def soup(n=40, seed=5):
    """Independent random triangles in the half-unit cube: a third well shaped with edges about 0.3, a third small (0.016), a third slivers (the
    third corner within 1e-3 of the length of the line through the other two), and face 11 exactly degenerate (three collinear corners whose
    cross product is exactly zero in any precision)."""
    g = np.random.default_rng(seed)
    ctr = g.uniform(-0.35, 0.35, (n, 1, 3))
    edge = np.where(np.arange(n) % 3 == 1, 0.016, 0.3)[:, None, None]
    tri = ctr + g.normal(0.0, 1.0, (n, 3, 3)) * edge * 0.5
    sl = np.arange(n) % 3 == 2
    t = g.uniform(0.1, 0.9, (n, 1))
    ln = np.linalg.norm(tri[:, 1] - tri[:, 0], axis=1, keepdims=True)
    tri[sl, 2] = (tri[:, 0] + t * (tri[:, 1] - tri[:, 0]) + g.normal(0.0, 1.0, (n, 3)) * ln * 1e-3)[sl]
    tri[11] = np.array([[0.0, 0.0, 0.0], [0.25, 0.125, 0.0], [0.5, 0.25, 0.0]])
    v = tri.reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


@functools.lru_cache(maxsize=None)
def base_mesh(kind):
    """(vertices float32, faces int32): never modified."""
    if kind == "octahedron":
        return gc.octahedron()
    if kind == "bad_faces":
        v, f, _ = gc.with_bad_faces(*gc.octahedron())
        return v, f
    if kind in ("blob8", "blob12"):
        m = mc.reference_mesh(mc.blob(int(kind[4:])), 0.5)
        return m.vertices.astype(np.float32), m.faces.astype(np.int32)
    if kind == "soup":
        return soup()
    raise KeyError(kind)


MESHES = ("octahedron", "bad_faces", "blob8", "blob12", "soup")
FACES = (1, 7, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
QUERIES = (1, 255, 257, 700)
OFFSETS = (0.0, 1e-3, 0.3)
XF = np.array([[0.99, -0.33, 0.22, 0.25, 0.363, 0.946, -0.11, -0.5, -0.187, 0.187, 1.045, 0.125],       # about 1.1 x a rotation, and a shift
               [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0],
               [0.5, 0, 0, 0.1, 0, 0, -0.5, 0, 0, 0.5, 0, -0.2]], np.float32)
XF_MESH = np.array([[0, -1, 0, 0.05, 1, 0, 0, -0.02, 0, 0, 1, 0.01],                                      # a quarter turn and a shift
                    [0.9, 0, 0, 0, 0, 0.9, 0, 0, 0, 0, 0.9, 0],
                    [0.8, 0.6, 0, 0, -0.6, 0.8, 0, 0, 0, 0, 1, 0.25]], np.float32)


def fit_faces(f, F, roll=0):
    """The face list cut or padded (cyclically repeated) to F faces, starting at face `roll`."""
    f = np.roll(np.asarray(f, np.int32), -roll, axis=0)
    return np.ascontiguousarray(np.resize(f, (F, 3)))


def queries_for(v, f, Nq, seed):
    """Nq queries: a quarter on the surface (the contract's own samples of the valid faces), a quarter 1e-3 and half of them 0.3 away from such
    a sample, in a random direction of the outward half space of its face (the far ones are those that land in vertex and edge regions)."""
    s = gc.sample_surface(v, f, Nq)
    g = np.random.default_rng(seed)
    if s["status"] != 0:
        return gc.uniform_points((Nq, 3), seed)
    d = g.standard_normal((Nq, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where(_dot(d, s["normals"]) < 0, -1.0, 1.0)[:, None]
    off = np.asarray(OFFSETS + OFFSETS[-1:])[g.permutation(Nq) % 4]
    return (s["points"] + off[:, None] * d).astype(np.float32)


Case = namedtuple("Case", "name mesh F Nq packed xf q vertices faces counts q_count xf_q xf_mesh")


@functools.lru_cache(maxsize=None)
def case(im, iF):
    """One case of the distance tests: B = 3 pairs of mesh MESHES[im] cut or padded to FACES[iF] faces (each pair starts its face list elsewhere
    and keeps fewer of them), Nq, the layout and the transforms taken in turn so that every value of each meets every mesh and every F over
    the grid. q [3][Nq][3], vertices / faces: a list per pair (the test lays them out padded or packed), counts [3][2], q_count [3] or None."""
    kind, F = MESHES[im], FACES[iF]
    k = im + iF
    Nq = QUERIES[k % 4]
    packed, xf = bool((k // 2) % 2), bool(((k + im) // 3) % 2)
    v, f = base_mesh(kind)
    nfs = [F, (F + 1) // 2, max(F - 3, 0)]
    faces = [fit_faces(f, F, roll=b * 3) for b in range(3)]
    q = []
    for b in range(3):                                        # queries are laid out around the mesh AS IT IS SCORED (after xf_mesh) ...
        qb = queries_for(xf32(v, XF_MESH[b]) if xf else v, faces[b][:max(nfs[b], 1)], Nq, 1000 * im + 10 * iF + b)
        if xf:                                                # ... and handed over in the frame that xf_q brings back there (up to rounding)
            m = XF[b].astype(np.float64).reshape(3, 4)
            qb = ((qb.astype(np.float64) - m[:, 3]) @ np.linalg.inv(m[:, :3]).T).astype(np.float32)
        q.append(qb)
    counts = np.array([[len(v), nfs[b]] for b in range(3)], np.int32)
    q_count = np.array([Nq, (Nq + 1) // 2, max(Nq - 1, 0)], np.int32) if k % 3 != 1 else None
    return Case("%s-F%d" % (kind, F), kind, F, Nq, packed, xf, np.stack(q), [v, v, v], faces, counts, q_count, XF if xf else None,
                XF_MESH if xf else None)


def restate_case(c, b):
    nq = c.Nq if c.q_count is None else int(c.q_count[b])
    return restate(c.q[b, :nq], c.vertices[b], c.faces[b], int(c.counts[b, 1]), None if c.xf_q is None else c.xf_q[b],
                   None if c.xf_mesh is None else c.xf_mesh[b])


_RESTATED = {}


def restated(im, iF, b):
    """restate_case, kept: the GPU tests and the measurement of K share it."""
    if (im, iF, b) not in _RESTATED:
        _RESTATED[(im, iF, b)] = restate_case(case(im, iF), b)
    return _RESTATED[(im, iF, b)]


def k_of_winner(r, val, face):
    """(k_lo, k_hi) that the winners (val [Nq] distances, face [Nq]) of a Restated pair need, in the form the contract is asserted:
      lower   val >= T_f* - k_lo u L_f*                      -> k_lo = (T_f* - val) / (u L_f*)
      upper   val <= T_f + k_hi u L_f / s_f^2 for EVERY f    -> k_hi = (val - T_f) s_f^2 / (u L_f), its largest
      named   |val - T_face| <= k_hi u L / s^2 of the face that won (no winner although there are candidates: no k is enough)."""
    if r.T.shape[1] == 0 or not r.cand.any() or r.T.shape[0] == 0:
        return 0.0, 0.0
    rows = np.arange(len(val))
    fstar = r.T.argmin(axis=1)
    k_lo = float(((r.T[rows, fstar] - val) / (U * r.L[rows, fstar])).max())
    with np.errstate(invalid="ignore"):
        need = np.where(r.cand[None, :], (val[:, None] - r.T) * (r.s ** 2)[None, :] / (U * r.L), -np.inf)
    fw = np.maximum(face, 0)
    with np.errstate(invalid="ignore"):
        named = np.where(face >= 0, np.abs(val - r.T[rows, fw]) * r.s[fw] ** 2 / (U * r.L[rows, fw]), np.inf)
    return max(k_lo, 0.0), max(float(need.max()), float(named.max()), 0.0)


def k_of_pair(r, d):
    """k_of_winner of the scores d [Nq,F] (NaN: never wins) under the kernel's rule."""
    return k_of_winner(r, *winner(d))


@functools.lru_cache(maxsize=None)
def measured_k():
    """(K_lo, K_hi) of closest32 over every pair of every case: what the fp32 expression order itself costs. The device is allowed 4 times
    that (fma contraction it does not have, v_rcp_f32 against the true division used here)."""
    k_lo = k_hi = 0.0
    for im in range(len(MESHES)):
        for iF in range(len(FACES)):
            for b in range(3):
                r = restated(im, iF, b)
                lo, hi = k_of_pair(r, scored32(r))
                k_lo, k_hi = max(k_lo, lo), max(k_hi, hi)
    return k_lo, k_hi
