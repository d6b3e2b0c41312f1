"""The surface-metric contract (include/forge_hip.h section g3) restated in float64 numpy, and the cases its tests run on: surface sampling,
nearest neighbours between point sets, and the reduction to accuracy / completeness / Chamfer / Hausdorff / F-score / normal consistency.
Used by tests/test_geometry_metrics_cpu.py (known answers, no GPU) and tests/test_gpu_geometry_metrics.py (the kernels against this)."""
import math

import numpy as np

U = 2.0 ** -24                                 # fp32 unit roundoff
EMPTY = 1                                      # FORGE_GEOM_EMPTY
SCAN_THREADS = 256                             # forge_geom_scan_threads(): the chunking of the cumulative-area scan
OUT = {"accuracy": 0, "completeness": 1, "chamfer_l1": 2, "chamfer_l2": 3, "hausdorff": 4, "normal_consistency": 5, "precision": 6, "recall": 10,
       "fscore": 14}
OUT_DOUBLES = 18


# -------------------------------------------------------------------------------------------------------------------------------- cases
def sphere_points(n, r=1.0, seed=0):
    """n points on the sphere of radius r (float32) and their radial unit normals: normalised gaussian draws of a seeded generator."""
    g = np.random.default_rng(seed).standard_normal((n, 3))
    nrm = g / np.linalg.norm(g, axis=1, keepdims=True)
    return (nrm * r).astype(np.float32), nrm.astype(np.float32)


def octahedron(r=0.4):
    """8 outward-wound faces of different areas (the axes are scaled 1, 0.75, 0.5)."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 0.75, 0], [0, -0.75, 0], [0, 0, 0.5], [0, 0, -0.5]], np.float32) * np.float32(r)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def with_bad_faces(v, f):
    """The mesh with three faces that must never be chosen inserted among the real ones: a zero-area face (a repeated corner), one with an index
    past the vertex count and one with a negative index."""
    bad = np.array([[0, 0, 1], [0, 1, len(v)], [-1, 0, 1]], np.int32)
    return v, np.concatenate([f[:3], bad[:1], f[3:5], bad[1:], f[5:]]), [3, 6, 7]


def uniform_points(shape, seed):
    return (np.random.default_rng(seed).random(shape, dtype=np.float64) - 0.5).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------- surface sampling
def face_areas(v, f):
    """A_f in float64 from the fp32 corners; 0 for a face with an index outside 0 .. len(v) - 1."""
    v = np.asarray(v, np.float32).astype(np.float64)
    f = np.asarray(f, np.int64)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    fs = np.where(ok[:, None], f, 0)
    a, b, c = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
    return np.where(ok, 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1), 0.0)


def cumulative_areas(areas):
    """The inclusive scan in the contract's order: chunk = ceil(F / 256); the sum of the chunks before (chunk sums added in increasing index) plus
    the running sum within the chunk."""
    F = len(areas)
    cum = np.zeros(F, np.float64)
    chunk = -(-F // SCAN_THREADS) if F else 0
    run = 0.0
    for t in range(SCAN_THREADS if F else 0):
        lo, hi = min(t * chunk, F), min(t * chunk + chunk, F)
        s = 0.0
        for k in range(lo, hi):
            s += float(areas[k])
            cum[k] = run + s
        run += s
    return cum


def barycentrics(n):
    """(r1, r2) of samples 0 .. n-1: integers only, exact in fp32."""
    i = np.arange(n, dtype=np.uint64)
    k1 = ((i * 3242174889) & 0xFFFFFFFF) >> 8
    k2 = ((i * 2447445414) & 0xFFFFFFFF) >> 8
    flip = k1 + k2 > (1 << 24)
    k1 = np.where(flip, (1 << 24) - k1, k1)
    k2 = np.where(flip, (1 << 24) - k2, k2)
    return (k1.astype(np.float64) * 2.0 ** -24).astype(np.float32), (k2.astype(np.float64) * 2.0 ** -24).astype(np.float32)


def sample_points(v, f, face, r1, r2):
    """a + r1 (b - a) + r2 (c - a) in float64 from faces and barycentrics."""
    v = np.asarray(v, np.float32).astype(np.float64)
    fs = np.asarray(f, np.int64)[face]
    a, b, c = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
    return a + r1.astype(np.float64)[:, None] * (b - a) + r2.astype(np.float64)[:, None] * (c - a)


def sample_surface(v, f, n):
    """-> dict(face [n] int, r1, r2 [n] float32, points [n,3] float64, normals [n,3] float64, areas [F], status)."""
    areas = face_areas(v, f)
    cum = cumulative_areas(areas)
    total = cum[-1] if len(cum) else 0.0
    r1, r2 = barycentrics(n)
    if not (total > 0.0 and math.isfinite(total)):
        return dict(face=np.full(n, -1), r1=r1, r2=r2, points=np.zeros((n, 3)), normals=np.zeros((n, 3)), areas=areas, status=EMPTY)
    u = (np.arange(n, dtype=np.float64) + 0.5) / float(n) * total
    face = np.minimum(np.searchsorted(cum, u, side="right"), len(cum) - 1)          # the first f with cum[f] > u
    vv = np.asarray(v, np.float32).astype(np.float64)
    fs = np.asarray(f, np.int64)[face]
    cr = np.cross(vv[fs[:, 1]] - vv[fs[:, 0]], vv[fs[:, 2]] - vv[fs[:, 0]])
    ln = np.linalg.norm(cr, axis=1, keepdims=True)
    return dict(face=face, r1=r1, r2=r2, points=sample_points(v, f, face, r1, r2), normals=np.where(ln > 0, cr / np.maximum(ln, 1e-300), 0.0),
                areas=areas, status=0)


def check_systematic(face, areas, n):
    """The properties of systematic sampling on a face list; returns the largest |k_f - n A_f / A|."""
    face = np.asarray(face, np.int64)
    assert (np.diff(face) >= 0).all(), "face indices must be non-decreasing"
    k = np.bincount(face, minlength=len(areas)).astype(np.float64)
    dev = np.abs(k - n * areas / areas.sum())
    assert (dev < 1.0 + 1e-6 * n).all(), dev.max()
    assert (k[areas == 0.0] == 0).all(), "a face without area was chosen"
    return float(dev.max())


# -------------------------------------------------------------------------------------------------------------------- nearest neighbours
def transform_points(q, xf):
    """q [N,3] float32, xf [12] float32 (row-major 3x4) -> q' in float64 (exact products and sums of the fp32 operands, rounded once in float64)."""
    m = np.asarray(xf, np.float32).astype(np.float64).reshape(3, 4)
    return np.asarray(q, np.float32).astype(np.float64) @ m[:, :3].T + m[:, 3]


def nn(q, p, nq=None, np_=None, xf=None):
    """One pair in float64: -> dict(d2 [Nq], idx [Nq], runner_up [Nq] (the second smallest d2, inf without one), dist(i, j) -> d2 of a pair).
    Rows at or past nq: d2 = 0, idx = -1; np_ = 0: d2 = inf, idx = -1."""
    q64 = np.asarray(q, np.float64) if xf is None else transform_points(q, xf)      # fp32 inputs widen exactly
    p64 = np.asarray(p, np.float64)
    Nq = len(q64)
    nq = Nq if nq is None else int(nq)
    np_ = len(p64) if np_ is None else int(np_)
    d2, idx, second = np.zeros(Nq), np.full(Nq, -1, np.int64), np.full(Nq, np.inf)
    if np_ == 0:
        d2[:nq] = np.inf
    else:
        for lo in range(0, nq, 256):                                                # 256 queries at a time: the distance matrix stays small
            hi = min(lo + 256, nq)
            full = ((q64[lo:hi, None, :] - p64[None, :np_, :]) ** 2).sum(axis=2)
            idx[lo:hi] = full.argmin(axis=1)                                        # numpy's argmin returns the first minimum
            d2[lo:hi] = full[np.arange(hi - lo), idx[lo:hi]]
            if np_ > 1:
                second[lo:hi] = np.partition(full, 1, axis=1)[:, 1]
    return dict(d2=d2, idx=idx, runner_up=second, q=q64, p=p64)


# --------------------------------------------------------------------------------------------------------------------------- the metrics
def metrics(d2_ab, idx_ab, d2_ba, idx_ba, normals_a=None, normals_b=None, na=None, nb=None, thresholds=()):
    """One pair: the reduction of section g3 in float64 -> (out [18], status)."""
    def direction(d2, idx, n, nf, nt):
        d2 = np.asarray(d2, np.float64)[:n]
        d = np.sqrt(d2)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_d, mean_d2 = d.sum() / n if n else np.nan, d2.sum() / n if n else np.nan
            frac = [float((d < t).sum()) / n if n else np.nan for t in thresholds]
            nc = np.nan
            if nf is not None:
                j = np.asarray(idx, np.int64)[:n]
                ok = j >= 0
                dots = (np.asarray(nf, np.float32).astype(np.float64)[:n][ok] * np.asarray(nt, np.float32).astype(np.float64)[j[ok]]).sum(axis=1)
                nc = np.abs(dots).sum() / n if n else np.nan
        return mean_d, mean_d2, (d.max() if n else np.nan), frac, nc
    na = len(d2_ab) if na is None else int(na)
    nb = len(d2_ba) if nb is None else int(nb)
    A = direction(d2_ab, idx_ab, na, normals_a, normals_b)
    B = direction(d2_ba, idx_ba, nb, normals_b, normals_a)
    out = np.full(OUT_DOUBLES, np.nan)
    out[0], out[1], out[2], out[3] = A[0], B[0], 0.5 * (A[0] + B[0]), A[1] + B[1]
    out[4] = np.nan if (np.isnan(A[2]) or np.isnan(B[2])) else max(A[2], B[2])
    out[5] = 0.5 * (A[4] + B[4])
    for k in range(len(thresholds)):
        P, R = A[3][k], B[3][k]
        out[6 + k], out[10 + k] = P, R
        out[14 + k] = 0.0 if P + R == 0.0 else 2.0 * P * R / (P + R)
    return out, (EMPTY if na == 0 or nb == 0 else 0)


def point_metrics(a, b, normals_a=None, normals_b=None, thresholds=(), na=None, nb=None, xf=None):
    """nn both ways + metrics, all float64: the known-answer path of the CPU tests. Returns (out [18], status, nn a -> b, nn b -> a)."""
    ab = nn(a, b, na, nb, xf)
    ba = nn(b, ab["q"], nb, na)                    # against a in the frame of b, kept in float64
    out, status = metrics(ab["d2"], ab["idx"], ba["d2"], ba["idx"], normals_a, normals_b, na, nb, thresholds)
    return out, status, ab, ba
