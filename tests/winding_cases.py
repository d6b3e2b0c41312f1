"""The winding-number contract (include/forge_hip.h section g3c) restated in numpy, and the cases its tests run on.

  theta64      the float64 restatement: per (query, face) Van Oosterom and Strackee's half angle theta_f and kappa_f = la lb lc / hypot(num, den);
  second64     an independently written second formulation: the solid angle as the sum of the three dihedral angles minus pi, halved;
  atan2_32, theta32   the header's fp32 expression order, fma by fma (tri_cases.fma32), the reciprocal a true division;
  restate      one pair as the kernel sees it: the transforms in the fp32 chain, the candidate faces, theta [Nq,F], w [Nq], scale [Nq];
  w32          the header's sum on theta32: groups of 8 faces in fp32 from 0, group totals in float64;
  case()       the meshes, face counts, query counts, layouts and transforms of tests/test_gpu_winding.py, built once, never modified;
  measured_k() the worst |w32 - w| / (u scale) over those cases: what the fp32 order itself costs.
The error model: |w_dev - w| <= K u scale, scale = (1 / 2 pi) sum_f (kappa_f + |theta_f|), u = 2^-24. num and den carry rounding of about
u la lb lc each, which moves atan2 by u la lb lc / hypot(num, den) = u kappa_f; the polynomial and the sums are relative to |theta_f|.
Used by tests/test_winding_cpu.py (no GPU) and tests/test_gpu_winding.py (the kernels against this)."""
import functools
from collections import namedtuple

import numpy as np

import geom_cases as gc
import mesh_cases as mc  # noqa: F401  (the blobs of tri_cases.base_mesh are its fields)
import tri_cases as tc

U = gc.U
TILE = tc.TILE
GROUP = 8                                      # faces per fp32 group sum (section g3c)
INV_2PI = 0.15915494309189535
MESHES, FACES, QUERIES = tc.MESHES, tc.FACES, tc.QUERIES
CLOSED = ("blob8", "blob12")                   # extracted meshes: closed when whole
OFFSETS = (0.3, 1e-2, 1e-3)
ATAN_P = (2.920691855e-03, -1.636792719e-02, 4.321185872e-02, -7.552213967e-02, 1.066600457e-01, -1.421105564e-01, 1.999377310e-01,
          -3.333315253e-01)


def _dot(u, v):
    return (u * v).sum(axis=-1)


# ------------------------------------------------------------------------------------------------------------------- the restatements
def theta64(q, a, b, c):
    """q, a, b, c [..., 3] (broadcast), float64 -> (theta, kappa). theta = atan2(A . (B x C), la lb lc + (A.B) lc + (B.C) la + (C.A) lb)."""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    A, B, C = a - q, b - q, c - q
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    num = _dot(A, np.cross(B, C))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.arctan2(num, den), la * lb * lc / np.hypot(num, den)


def _angle(u, v):
    return np.arctan2(np.linalg.norm(np.cross(u, v), axis=-1), _dot(u, v))


def second64(q, a, b, c):
    """The same half angle from spherical geometry: the area of the spherical triangle of the three unit directions is the sum of its dihedral
    angles minus pi (Girard); its sign is that of the triple product. The dihedral angle at A is the angle between A x B and A x C."""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    A, B, C = a - q, b - q, c - q
    ab, bc, ca = np.cross(A, B), np.cross(B, C), np.cross(C, A)
    omega = _angle(ab, -ca) + _angle(bc, -ab) + _angle(ca, -bc) - np.pi
    return 0.5 * np.sign(_dot(A, bc)) * omega


fma32 = tc.fma32


def _dot32(u, v):
    return fma32(u[..., 2], v[..., 2], fma32(u[..., 1], v[..., 1], u[..., 0] * v[..., 0]))


def atan2_32(y, x):
    """The header's atan2 in numpy float32 (every operation rounds to nearest; 1 / mx is a true division here)."""
    y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
        t = mn * (np.float32(1) / mx)
        s = t * t
        p = np.float32(ATAN_P[0]) + np.float32(0) * s
        for c in ATAN_P[1:]:
            p = fma32(p, s, np.float32(c))
        r = fma32(p * s, t, t)
        r = np.where(ay > ax, np.float32(1.57079637) - r, r)
        r = np.where(x < 0, np.float32(3.14159274) - r, r)
        return np.copysign(r, y).astype(np.float32)


def theta32(q, a, b, c):
    """The header's order in fp32 -> theta_f float32 (NaN where the header's is)."""
    q, a, b, c = (np.asarray(x, np.float32) for x in (q, a, b, c))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A, B, C = a - q, b - q, c - q
        la, lb, lc = np.sqrt(_dot32(A, A)), np.sqrt(_dot32(B, B)), np.sqrt(_dot32(C, C))
        n = np.stack([fma32(B[..., 1], C[..., 2], -(B[..., 2] * C[..., 1])), fma32(B[..., 2], C[..., 0], -(B[..., 0] * C[..., 2])),
                      fma32(B[..., 0], C[..., 1], -(B[..., 1] * C[..., 0]))], axis=-1)
        num = _dot32(A, n)
        ab, bc, ca = _dot32(A, B), _dot32(B, C), _dot32(C, A)
        den = fma32(ca, lb, fma32(bc, la, fma32(ab, lc, (la * lb) * lc)))
        return atan2_32(num, den)


Restated = namedtuple("Restated", "q a b c cand theta kappa w scale")


def restate(q, v, f, nf=None, xf_q=None, xf_mesh=None):
    """One pair as the kernel sums it: q [Nq,3], v [V,3] float32, f [F,3] int -> Restated. q', a, b, c carry the fp32 transforms; cand [F] marks
    the candidates (tri_cases.restate's rule); theta, kappa [Nq,F] in float64 (0 for a face that is no candidate, and where theta is NaN: a
    query on a vertex); w [Nq] = sum theta / 2 pi; scale [Nq] = sum (kappa + |theta|) / 2 pi."""
    v = np.asarray(v, np.float32)
    f = np.asarray(f, np.int64)[:len(f) if nf is None else nf]
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    cand = ok & (gc.face_areas(v, f) != 0.0)
    fs = np.where(ok[:, None], f, 0)
    vt = tc.xf32(v, xf_mesh).astype(np.float64)
    a, b, c = vt[fs[:, 0]], vt[fs[:, 1]], vt[fs[:, 2]]
    q64 = tc.xf32(q, xf_q).astype(np.float64)
    th, kp = theta64(q64[:, None, :], a[None], b[None], c[None])
    keep = cand[None, :] & ~np.isnan(th) & ~np.isnan(kp)           # numpy's atan2(0, 0) is 0, but kappa there is 0 / 0
    th, kp = np.where(keep, th, 0.0), np.where(keep, kp, 0.0)
    return Restated(q64, a, b, c, cand, th, kp, th.sum(axis=1) * INV_2PI, (kp + np.abs(th)).sum(axis=1) * INV_2PI)


def w32(r):
    """The header's sum over a Restated pair -> w [Nq] float32: theta32 per face (0 where NaN or no candidate), the terms of each group of 8
    consecutive faces added in fp32 from 0 in order, the group totals in float64 in order, times 1 / 2 pi in float64, rounded once."""
    Nq, F = r.theta.shape
    if F == 0 or Nq == 0:
        return np.zeros(Nq, np.float32)
    th = theta32(r.q[:, None, :], r.a[None], r.b[None], r.c[None])
    th = np.where(r.cand[None, :] & ~np.isnan(th), th, np.float32(0)).astype(np.float32)
    pad = (-F) % GROUP
    th = np.concatenate([th, np.zeros((Nq, pad), np.float32)], axis=1).reshape(Nq, -1, GROUP)
    gs = np.zeros(th.shape[:2], np.float32)
    for e in range(GROUP):
        gs = (gs + th[:, :, e]).astype(np.float32)
    total = np.zeros(Nq, np.float64)
    for g in range(gs.shape[1]):
        total = total + gs[:, g].astype(np.float64)
    return (total * INV_2PI).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------- cases
def queries_for(v, f, Nq, seed):
    """Nq queries: a quarter each 0.3, 1e-2 and 1e-3 away from a sample of the valid faces (gc.sample_surface) in a random direction, on either
    side of the surface, and a quarter uniform in the unit cube around the origin. None lies on the surface."""
    s = gc.sample_surface(v, f, Nq)
    uni = gc.uniform_points((Nq, 3), seed)
    if s["status"] != 0:
        return uni
    g = np.random.default_rng(seed)
    d = g.standard_normal((Nq, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kind = g.permutation(Nq) % 4
    off = np.asarray(OFFSETS + (0.0,))[kind]
    return np.where((kind == 3)[:, None], uni, (s["points"] + off[:, None] * d).astype(np.float32)).astype(np.float32)


Case = tc.Case


@functools.lru_cache(maxsize=None)
def case(im, iF):
    """One case: B = 3 pairs of mesh MESHES[im] cut or padded (cyclically repeated) to FACES[iF] faces, each pair starting its face list elsewhere
    and keeping fewer of them (a cut mesh is open; the last pair of the one-face cases has no face at all); Nq, the layout, the transforms and
    q_count taken in turn as tri_cases.case takes them, so that every value of each meets every mesh over the grid."""
    kind, F = MESHES[im], FACES[iF]
    k = im + iF
    Nq = QUERIES[k % 4]
    packed, xf = bool((k // 2) % 2), bool(((k + im) // 3) % 2)
    v, f = tc.base_mesh(kind)
    nfs = [F, (F + 1) // 2, max(F - 3, 0)]
    faces = [tc.fit_faces(f, F, roll=b * 3) for b in range(3)]
    q = []
    for b in range(3):                                        # queries are laid out around the mesh AS IT IS SUMMED (after xf_mesh) ...
        qb = queries_for(tc.xf32(v, tc.XF_MESH[b]) if xf else v, faces[b][:max(nfs[b], 1)], Nq, 2000 * im + 10 * iF + b)
        if xf:                                                # ... and handed over in the frame that xf_q brings back there (up to rounding)
            m = tc.XF[b].astype(np.float64).reshape(3, 4)
            qb = ((qb.astype(np.float64) - m[:, 3]) @ np.linalg.inv(m[:, :3]).T).astype(np.float32)
        q.append(qb)
    counts = np.array([[len(v), nfs[b]] for b in range(3)], np.int32)
    q_count = np.array([Nq, (Nq + 1) // 2, max(Nq - 1, 0)], np.int32) if k % 3 != 1 else None
    return Case("%s-F%d" % (kind, F), kind, F, Nq, packed, xf, np.stack(q), [v, v, v], faces, counts, q_count, tc.XF if xf else None,
                tc.XF_MESH if xf else None)


_RESTATED = {}


def restated(im, iF, b):
    """restate of pair b of case (im, iF) on its valid rows, kept: the GPU tests and the measurement of K share it."""
    if (im, iF, b) not in _RESTATED:
        c = case(im, iF)
        nq = c.Nq if c.q_count is None else int(c.q_count[b])
        _RESTATED[(im, iF, b)] = restate(c.q[b, :nq], c.vertices[b], c.faces[b], int(c.counts[b, 1]), None if c.xf_q is None else c.xf_q[b],
                                         None if c.xf_mesh is None else c.xf_mesh[b])
    return _RESTATED[(im, iF, b)]


def k_of(r, w):
    """The K that the values w [Nq] of a Restated pair need: the largest |w - r.w| / (u scale); 0 without a candidate (w must then be 0)."""
    if not len(r.q) or not (r.scale > 0).any():
        return 0.0
    ok = r.scale > 0
    return float((np.abs(np.asarray(w, np.float64) - r.w)[ok] / (U * r.scale[ok])).max())


GRID = [(im, iF) for im in range(len(MESHES)) for iF in range(len(FACES))]


@functools.lru_cache(maxsize=None)
def measured_k():
    """K of w32 over every pair of every case: what the fp32 expression order and the grouped sum cost. The device is allowed 4 times that
    (v_sqrt_f32 and v_rcp_f32 against numpy's correctly rounded ones), as tests/test_gpu_tridist.py allows its kernel."""
    return max(k_of(restated(im, iF, b), w32(restated(im, iF, b))) for im, iF in GRID for b in range(3))


def whole_closed(kind, Nq=700, seed=7):
    """A whole extracted mesh (closed) and Nq queries around it -> (v, f, q, Restated)."""
    v, f = tc.base_mesh(kind)
    q = queries_for(v, f, Nq, seed)
    return v, f, q, restate(q, v, f)
