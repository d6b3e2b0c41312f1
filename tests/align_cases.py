"""The alignment contract (include/forge_hip.h section g5) restated in float64 numpy, and the cases its tests run on: the moments of a step, the
solve (numpy.linalg.svd with the determinant fix), rejection, the freeze, the selection among starts and the ICP loop (the search is geom_cases.nn
under the fp32 xf). Used by tests/test_align_cpu.py (known answers, no GPU) and tests/test_gpu_align.py (the kernels against this).

How exact the restatement itself is: `self_error` runs one step in float64 and again in numpy.longdouble (64-bit mantissa here; its SVD is a
one-sided Jacobi written below, since numpy.linalg has none for longdouble) and returns the largest |difference| / max(1, |value|) over T, SCALE,
RMSE and SV. Over the cases of tests/test_gpu_align.py (N in {1, 2, 3, 255, 257, 1000} x 3 pairs x with / without scale, idx and d2 from the
device's own search) the measured maximum is MEASURED_SELF_ERROR below; the device, which contracts fmas and sums in another order, is allowed 16
times the maximum the test measures on its own cases."""
import math

import numpy as np

import geom_cases as gc

MEASURED_SELF_ERROR = 3.8e-15                  # tests/test_gpu_align.py prints it: `align step: restatement float64 vs longdouble`
U = gc.U
EMPTY, RANK, NONFINITE, CONVERGED = 1, 2, 4, 8
T, SCALE, RMSE, N_IN, N_VALID, CUT2, DELTA, ITERATIONS, SV, SCORE, CQ, CP, STATE = 0, 12, 13, 14, 15, 16, 17, 18, 19, 22, 23, 26, 29
PARTIAL = 21                                   # n_in | n_valid | sum q | sum p | sum p_r q_c (9) | sum |q|^2 | sum d2 | sum min(d2, clamp2) | skipped rows
RANK_TOL = 1e-6


# -------------------------------------------------------------------------------------------------------------------------------- cases
def shape(n, seed):
    """n points (float32) of an asymmetric shape: an ellipsoid with semi-axes (0.40, 0.25, 0.15) whose first n // 3 points lie on a sphere of radius
    0.10 centred at (0.30, 0.15, 0.05) - no rotation maps it onto itself, so an alignment has one answer."""
    g = np.random.default_rng(seed).standard_normal((n, 3))
    u = g / np.linalg.norm(g, axis=1, keepdims=True)
    pts = u * np.array([0.40, 0.25, 0.15])
    k = n // 3
    pts[:k] = u[:k] * 0.10 + np.array([0.30, 0.15, 0.05])
    return pts.astype(np.float32)


def similarity(angle_deg, axis, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """[4,4] float64: scale x the rotation by angle_deg about axis (Rodrigues), then the shift."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = math.radians(angle_deg)
    M = np.eye(4)
    M[:3, :3] = scale * (np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K))
    M[:3, 3] = shift
    return M


def apply(M, pts):
    """M [4,4] float64 applied to pts [N,3] in float64, rounded once to float32."""
    return (np.asarray(pts, np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


SHIFT = (0.05, -0.03, 0.02)
ICP_CASES = [("rigid 15", similarity(15, (1, 2, 3), 1.0, SHIFT), False),              # (name, the transform b is made with, with_scale)
             ("similarity 15", similarity(15, (1, 2, 3), 1.1, SHIFT), True),
             ("rigid 25", similarity(25, (3, -1, 2), 1.0, (0.02, 0.04, -0.05)), False)]
FAR = similarity(100, (2, -1, 3), 1.0, (0.03, 0.02, -0.04))                          # beyond what ICP reaches from the identity: needs starts
N_FLOATERS = 51


def floaters():
    """N_FLOATERS points uniform in (-0.5, 0.5)^3: what replaces the last rows of a in the rejection cases."""
    return (np.random.default_rng(99).random((N_FLOATERS, 3)) - 0.5).astype(np.float32)


def new_state(init=None, dt=np.float64):
    st = np.zeros(STATE, dt)
    M = np.eye(4) if init is None else np.asarray(init, np.float64)
    st[T:T + 12] = M[:3, :4].reshape(12)
    st[SCALE] = math.sqrt(float((M[0, :3] ** 2).sum()))
    st[CUT2] = st[DELTA] = np.inf
    st[RMSE] = st[SCORE] = np.nan
    return st


# ------------------------------------------------------------------------------------------------------------------------- the moments
def row_terms(q, p, idx=None, d2=None, nq=None, np_=None, cut2=np.inf, clamp2=np.inf, dt=np.float64):
    """[rows, PARTIAL]: what each looked-at row adds to the 21 sums of launch 1 (zeros for a skipped row). Products of two widened fp32 values are
    exact in float64, and (qx qx + qy qy) + qz qz rounds where fma(qz, qz, fma(qy, qy, qx qx)) does: the terms are the device's, bit for bit."""
    q, p = np.asarray(q, np.float32).astype(dt), np.asarray(p, np.float32).astype(dt)
    nq = len(q) if nq is None else min(max(int(nq), 0), len(q))
    np_ = len(p) if np_ is None else min(max(int(np_), 0), len(p))
    rows = nq if idx is not None else min(nq, np_)
    j = np.asarray(idx, np.int64)[:rows] if idx is not None else np.arange(rows)
    matched = (j >= 0) & (j < np_)
    qi, pj = q[:rows], p[np.where(matched, j, 0)] if len(p) else np.zeros((rows, 3), dt)
    d = np.asarray(d2, np.float32)[:rows].astype(dt) if d2 is not None else np.zeros(rows, dt)
    finite = np.isfinite(qi).all(axis=1) & np.isfinite(pj).all(axis=1) & ~np.isnan(d)
    valid = matched & finite
    with np.errstate(invalid="ignore"):
        inl = valid & ~(d > cut2)
    t = np.zeros((rows, PARTIAL), dt)
    z = lambda mask, v: np.where(mask if np.ndim(v) == 1 else mask[:, None], v, 0)       # noqa: E731  (a skipped row adds 0, never NaN x 0)
    qz_, pz_, dz_ = z(inl, qi), z(inl, pj), z(inl, d)
    t[:, 0], t[:, 1] = inl, valid
    t[:, 2:5], t[:, 5:8] = qz_, pz_
    t[:, 8:17] = (pz_[:, :, None] * qz_[:, None, :]).reshape(rows, 9)
    t[:, 17] = (qz_[:, 0] * qz_[:, 0] + qz_[:, 1] * qz_[:, 1]) + qz_[:, 2] * qz_[:, 2]
    t[:, 18] = dz_
    t[:, 19] = z(valid, np.minimum(np.where(valid, d, 0), clamp2))
    t[:, 20] = matched & ~finite
    return t


def exact_moments(terms):
    """(math.fsum of every column, the sum of |term| of every column): what the moment bound n 2^-53 sum |term| is taken against."""
    cols = np.asarray(terms, np.float64).T
    return np.array([math.fsum(c) for c in cols]), np.array([math.fsum(np.abs(c)) for c in cols])


# --------------------------------------------------------------------------------------------------------------------------- the solve
def _jacobi_svd(H, dt):
    """One-sided Jacobi (Hestenes) in dtype dt: (a: the rotated columns, s: their norms descending, v)."""
    a, v = np.array(H, dt), np.eye(3, dtype=dt)
    for _ in range(40):
        for pq in ((0, 1), (0, 2), (1, 2)):
            i, k = pq
            alpha, beta, gamma = a[:, i] @ a[:, i], a[:, k] @ a[:, k], a[:, i] @ a[:, k]
            if not abs(gamma) > dt(1e-22) * np.sqrt(alpha * beta):
                continue
            zeta = (beta - alpha) / (2 * gamma)
            t = np.copysign(dt(1), zeta) / (abs(zeta) + np.sqrt(zeta * zeta + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = c * t
            for m in (a, v):
                x, y = m[:, i].copy(), m[:, k].copy()
                m[:, i], m[:, k] = c * x - s * y, s * x + c * y
    s = np.sqrt((a * a).sum(axis=0))
    order = np.argsort(-s, kind="stable")
    return a[:, order], s[order], v[:, order]


def project_so3(H, dt=np.float64):
    """(R = U diag(1, 1, det(U V^T)) V^T, the singular values descending). float64: numpy.linalg.svd; any other dtype: the Jacobi above, with R in
    the form u0 v0^T + u1 v1^T + (u0 x u1)(v0 x v1)^T, which is the same matrix and needs no u2."""
    if dt is np.float64:
        Um, S, Vt = np.linalg.svd(np.asarray(H, np.float64))
        D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Um @ Vt) >= 0 else -1.0])
        return Um @ D @ Vt, S
    a, s, v = _jacobi_svd(H, dt)
    u0 = a[:, 0] / s[0]
    u1 = a[:, 1] / s[1]
    u1 = u1 - (u0 @ u1) * u0
    u1 = u1 / np.sqrt(u1 @ u1)
    return np.outer(u0, v[:, 0]) + np.outer(u1, v[:, 1]) + np.outer(np.cross(u0, u1), np.cross(v[:, 0], v[:, 1])), s


def solve(m, st, status, with_scale=False, update=True, reject=0.0, reject_floor=0.0, tol=0.0, rank_tol=RANK_TOL, dt=np.float64):
    """Launch 2 on the summed moments m [PARTIAL]: -> (state, status). The caller has dealt with a frozen pair."""
    st = np.array(st, dt)
    n, nv = m[0], m[1]
    bits = (EMPTY if n < 3 else 0) | (NONFINITE if m[20] > 0 else 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_d2 = m[18] / n
        st[RMSE], st[N_IN], st[N_VALID], st[SCORE] = np.sqrt(mean_d2), n, nv, m[19] / nv
        qm, pm = m[2:5] / n, m[5:8] / n
    st[CQ:CQ + 3], st[CP:CP + 3] = qm, pm
    if not update:
        return st, (status & (RANK | CONVERGED)) | bits
    st[ITERATIONS] += 1
    if bits & EMPTY:
        st[DELTA] = 0
        return st, bits
    H = m[8:17].reshape(3, 3) - np.outer(m[5:8], m[2:5]) / n
    vq = m[17] - (m[2:5] @ m[2:5]) / n
    R, sv = project_so3(H, dt)
    if not sv[0] > 0 or not sv[1] / sv[0] >= rank_tol:
        bits |= RANK
    s = (R * H).sum() / vq if (with_scale and vq > 0) else dt(1)
    Tn = np.zeros((3, 4), dt)
    Tn[:, :3] = s * R
    Tn[:, 3] = pm - Tn[:, :3] @ qm
    diff = np.abs(Tn.reshape(12) - st[T:T + 12])
    st[DELTA] = np.nan if np.isnan(diff).any() else diff.max()
    st[T:T + 12], st[SCALE], st[SV:SV + 3] = Tn.reshape(12), s, sv
    st[CUT2] = max(reject * reject * mean_d2, reject_floor * reject_floor) if reject > 0 else np.inf
    if st[DELTA] <= tol:
        bits |= CONVERGED
    return st, bits


def step(q, p, st, status, idx=None, d2=None, nq=None, np_=None, clamp2=np.inf, dt=np.float64, **opts):
    """forge_align_step for one pair: -> (state, status, xf [12] float32)."""
    st = np.array(st, dt)
    if not status & CONVERGED:
        terms = row_terms(q, p, idx, d2, nq, np_, st[CUT2], clamp2, dt)
        st, status = solve(terms.sum(axis=0) if len(terms) else np.zeros(PARTIAL, dt), st, status, dt=dt, **opts)
    return st, status, st[T:T + 12].astype(np.float32)


def self_error(q, p, st, status, **kw):
    """The largest |float64 - longdouble| / max(1, |longdouble|) over T, SCALE, RMSE and SV of one step (0 where the step leaves them alone or the
    fit is undetermined: EMPTY, RANK)."""
    assert np.finfo(np.longdouble).eps < 2e-19, "numpy.longdouble is no wider than float64 here"
    a, sa, _ = step(q, p, st, status, dt=np.float64, **kw)
    b, sb, _ = step(q, p, st, status, dt=np.longdouble, **kw)
    if sa != sb or sa & (EMPTY | RANK):
        return 0.0
    cols = list(range(T, T + 12)) + [SCALE, RMSE] + list(range(SV, SV + 3))
    return float(max(abs(np.longdouble(a[c]) - b[c]) / max(np.longdouble(1), abs(b[c])) for c in cols if not np.isnan(b[c])))


# ----------------------------------------------------------------------------------------------------------------------- the selection
def select(states, statuses):
    """forge_align_select for one pair: -> (best, state, status); strict `<` from +inf in increasing k, EMPTY never wins, none: (-1, start 0)."""
    best, score = -1, np.inf
    for k, (st, bits) in enumerate(zip(states, statuses)):
        if not bits & EMPTY and st[SCORE] < score:
            best, score = k, st[SCORE]
    k = max(best, 0)
    return best, np.array(states[k]), statuses[k]


# ------------------------------------------------------------------------------------------------------------------------- the ICP loop
def icp(a, b, iterations=32, init=None, na=None, nb=None, **opts):
    """geometry.align_points for one pair and one start: every iteration searches a under the fp32 xf in b (geom_cases.nn: the difference form,
    d2 rounded to fp32 as the kernel returns it) and steps; a last search and a statistics-only step measure. -> (state, status)."""
    st, status = new_state(init), 0
    xf = st[T:T + 12].astype(np.float32)
    na = len(a) if na is None else int(na)
    for it in range(iterations + 1):
        if status & CONVERGED:
            break                                   # frozen: every further step leaves it as it is
        r = gc.nn(a, b, na, nb, xf)
        st, status, xf = step(a, b, st, status, idx=r["idx"], d2=r["d2"].astype(np.float32), nq=na, np_=nb, update=it < iterations, **opts)
    return st, status


def matrix(st):
    M = np.eye(4)
    M[:3] = np.asarray(st[T:T + 12], np.float64).reshape(3, 4)
    return M


def fit_bound(a, b, M):
    """The length a point of a may miss its own image in b by when M is the transform b was made with: the fp32 rounding of xf and of the fma chain
    that applies it (geom_cases-style: 4 u (1 + 4 u) S per row with S = |t| + |m| |x|, four roundings instead of the chain's three for the
    rounding of xf itself), plus the rounding of b to fp32 (sqrt(3) u max |b|). rmse under the recovered transform, and the recovered transform's
    distance from M, are asserted against the largest value over the points."""
    m = np.abs(np.asarray(M, np.float64)[:3])
    S = np.abs(np.asarray(a, np.float64)) @ m[:, :3].T + m[:, 3]
    return float((4 * U * (1 + 4 * U) * np.linalg.norm(S, axis=1)).max() + math.sqrt(3) * U * np.abs(np.asarray(b, np.float64)).max())
