"""Exact point-to-triangle distances on the MI355X (forge_amd.ops.nn_triangles / geom_metrics_hits, forge_amd.geometry.point_mesh_distance /
mesh_metrics(surface="triangles") -> csrc/tridist.hip, csrc/geomdist.hip) against the float64 restatement of tests/tri_cases.py (include/forge_hip.h
section g3b). The contract is two-sided and per query, u = 2^-24, T_f the exact distance to face f, L_f the largest corner distance from the query,
s_f the sine of the face's smallest angle:
    lower   d >= min_f T_f - K_lo u L_f*  at the minimising face f*;
    upper   d <= min_f (T_f + K_hi u L_f / s_f^2);
    named   |d - T_face| <= K_hi u L / s^2 of the face the device names.
K_lo, K_hi = 4 x what the header's fp32 expression order costs in numpy float32 over these same cases (tri_cases.measured_k; the factor covers
v_rcp_f32 against a true division). Face indices are never compared with the restatement's: on a closed mesh neighbouring faces tie exactly."""
import numpy as np
import pytest
import torch

import geom_cases as gc
import mesh_cases as mc
import tri_cases as tc

pytestmark = pytest.mark.gpu

U = tc.U
_CACHE = {}


def dev(a, dt=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)


def K():
    lo, hi = tc.measured_k()
    return 4.0 * lo, 4.0 * hi


def lay_out(vertices, faces, counts, packed, spare=2):
    """The meshes of a batch as device rows. Padded: every mesh owns max rows, the rows past its count hold a face that WOULD be a candidate
    (0, 1, 2) - reading them shows. Packed: the meshes one after the other with `spare` such rows between them and offsets that skip them."""
    mv, mf = max(len(v) for v in vertices) + spare, max(len(f) for f in faces) + spare
    filler_v, filler_f = np.zeros((1, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    if not packed:
        V = np.concatenate([np.concatenate([v, np.repeat(filler_v, mv - len(v), 0)])[None] for v in vertices])
        Fm = np.concatenate([np.concatenate([f, np.repeat(filler_f, mf - len(f), 0)])[None] for f in faces])
        return dev(V), dev(Fm), dev(counts), None
    vs, fs, off = [], [], []
    nv = nf = 0
    for v, f in zip(vertices, faces):
        off.append([nv, nf])
        vs += [v, np.repeat(filler_v, spare, 0)]
        fs += [f, np.repeat(filler_f, spare, 0)]
        nv, nf = nv + len(v) + spare, nf + len(f) + spare
    return dev(np.concatenate(vs)), dev(np.concatenate(fs)), dev(counts), dev(np.array(off, np.int32))


def run_case(im, iF):
    key = ("case", im, iF)
    if key not in _CACHE:
        from forge_amd import ops
        c = tc.case(im, iF)
        V, Fm, counts, offsets = lay_out(c.vertices, c.faces, c.counts, c.packed)
        out = ops.nn_triangles(dev(c.q), V, Fm, counts, offsets=offsets, q_count=dev(c.q_count), xf_q=dev(c.xf_q), xf_mesh=dev(c.xf_mesh),
                               want_closest=True, want_normal=True)
        _CACHE[key] = [t.cpu().numpy() for t in out]
    return _CACHE[key]


def check_pair(r, d2, face, closest, normal, k_lo, k_hi):
    """The contract on one pair's valid rows -> the share of (k_lo, k_hi) that was used."""
    Nq = len(r.q)
    if Nq == 0:
        return 0.0, 0.0
    if not r.cand.any():
        assert np.isposinf(d2).all() and (face == -1).all() and (closest == 0).all() and (normal == 0).all()
        return 0.0, 0.0
    rows = np.arange(Nq)
    d = np.sqrt(d2.astype(np.float64))
    lower, upper, slack = tc.bounds(r, k_lo, k_hi)
    assert (face >= 0).all() and (face < len(r.cand)).all() and r.cand[face].all()
    assert (d >= lower).all(), float((lower - d).max())
    assert (d <= upper).all(), float((d - upper).max())
    assert (np.abs(d - r.T[rows, face]) <= slack[rows, face]).all()
    # closest = q' + P lies on the named face: its barycentrics are in [0, 1] up to delta / (the face's smallest height), delta = the slack of that
    # face plus the rounding of the sum q' + P (half an ulp per component)
    a, b, c = r.a[face], r.b[face], r.c[face]
    cl = closest.astype(np.float64)
    ab, ac, ap = b - a, c - a, cl - a
    g11, g12, g22 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    det = g11 * g22 - g12 * g12
    v = (g22 * (ab * ap).sum(1) - g12 * (ac * ap).sum(1)) / det
    w = (g11 * (ac * ap).sum(1) - g12 * (ab * ap).sum(1)) / det
    delta = slack[rows, face] + 2 * U * np.abs(cl).max(axis=1)
    height = np.sqrt(det) / np.sqrt(np.maximum(np.maximum(g11, g22), ((c - b) ** 2).sum(1)))
    tol = delta / height
    assert (v >= -tol).all() and (w >= -tol).all() and (v + w <= 1 + tol).all()
    assert (np.linalg.norm(ap - v[:, None] * ab - w[:, None] * ac, axis=1) <= delta).all()                  # and in its plane
    # |q' - closest| is d: the sum q' + P rounds each component by at most half an ulp of it, asserted as 4 ulp (8 u) of the largest
    assert (np.abs(np.linalg.norm(cl - r.q, axis=1) - d) <= 8 * U * np.abs(cl).max(axis=1) + 4 * U * d).all()
    n64 = np.cross(ab, ac)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    assert (np.abs(normal - n64).max(axis=1) <= 16 * U / r.s[face]).all()        # a cross product of fp32 edges: relative u per term, over the sine
    lo, hi = tc.k_of_winner(r, d, face)
    return lo / k_lo, hi / k_hi


@pytest.mark.parametrize("iF", range(len(tc.FACES)), ids=["F%d" % F for F in tc.FACES])
@pytest.mark.parametrize("im", range(len(tc.MESHES)), ids=tc.MESHES)
def test_nn_triangles_distances(im, iF):
    c = tc.case(im, iF)
    d2, face, closest, normal = run_case(im, iF)
    k_lo, k_hi = K()
    used = [0.0, 0.0]
    for b in range(3):
        nq = c.Nq if c.q_count is None else int(c.q_count[b])
        assert (d2[b, nq:] == 0).all() and (face[b, nq:] == -1).all() and (closest[b, nq:] == 0).all() and (normal[b, nq:] == 0).all()
        lo, hi = check_pair(tc.restated(im, iF, b), d2[b, :nq], face[b, :nq], closest[b, :nq], normal[b, :nq], k_lo, k_hi)
        used = [max(used[0], lo), max(used[1], hi)]
    print("tridist %-16s Nq %3d %s %s: measured K_lo %.3f K_hi %.3f, allowed x4, the device used %.3f and %.3f of that"
          % (c.name, c.Nq, "packed" if c.packed else "padded", "xf" if c.xf else "plain", k_lo / 4, k_hi / 4, used[0], used[1]))


# ------------------------------------------------------------------------------------------------------------------------- properties
def blob8_rows():
    if "blob8" not in _CACHE:
        v, f = tc.base_mesh("blob8")
        q = np.stack([tc.queries_for(v, f, 263, 71), tc.queries_for(v, f, 263, 72)])
        _CACHE["blob8"] = (v, f, q)
    return _CACHE["blob8"]


def test_ties_go_to_the_lower_copy_and_runs_are_identical():
    from forge_amd import ops
    v, f, q = blob8_rows()
    F = len(f)
    counts = lambda n: dev(np.array([[len(v), n]] * 2, np.int32))       # noqa: E731
    V = dev(np.stack([v, v]))
    base = ops.nn_triangles(dev(q), V, dev(np.stack([f, f])), counts(F), want_closest=True, want_normal=True)
    for name, ff, expect in (("appended", np.concatenate([f, f]), base[1]), ("interleaved", np.repeat(f, 2, axis=0), 2 * base[1])):
        out = ops.nn_triangles(dev(q), V, dev(np.stack([ff, ff])), counts(2 * F), want_closest=True, want_normal=True)
        assert torch.equal(out[0], base[0]) and torch.equal(out[1], expect) and torch.equal(out[2], base[2]) and torch.equal(out[3], base[3]), name
        again = ops.nn_triangles(dev(q), V, dev(np.stack([ff, ff])), counts(2 * F), want_closest=True, want_normal=True)
        assert all(torch.equal(x, y) for x, y in zip(out, again)), name
    alone = ops.nn_triangles(dev(q[1:]), V[1:].contiguous(), dev(f[None]), counts(F)[1:].contiguous(), want_closest=True, want_normal=True)
    assert all(torch.equal(x[1:], y) for x, y in zip(base, alone))


def own_samples():
    """[octahedron with faces that must not be chosen, blob8]: n samples of each, scored against their own triangles (the list path: packed rows)."""
    if "own" not in _CACHE:
        from forge_amd.geometry import Mesh, point_mesh_distance, sample_surface
        v0, f0, _ = gc.with_bad_faces(*gc.octahedron())
        v1, f1 = tc.base_mesh("blob8")
        meshes = [Mesh(dev(v), torch.zeros(len(v), 3, device="cuda"), dev(f)) for v, f in ((v0, f0), (v1, f1))]
        pts, nrm, sface, _, status = sample_surface(meshes, 600)
        hit = point_mesh_distance(pts, meshes)
        _CACHE["own"] = ([(v0, f0), (v1, f1)], [t.cpu().numpy() for t in (pts, nrm, sface, status)], [t.cpu().numpy() for t in hit])
    return _CACHE["own"]


def test_own_samples_lie_on_the_surface_and_hit_normals_are_the_samples():
    """A sample is fma(r2, c - a, fma(r1, b - a, a)) in fp32: it lies on its face up to that rounding, which T (float64, from the fp32 sample)
    carries; the device's distance is within the upper tolerance of T at the sample's OWN face, whichever face it names. Where it names that
    face the hit normal is the sample's normal bit for bit: one expression, the same operands."""
    meshes, (pts, nrm, sface, status), (dist, face, closest, normal) = own_samples()
    _, k_hi = K()
    for b, (v, f) in enumerate(meshes):
        r = tc.restate(pts[b], v, f)
        rows = np.arange(len(pts[b]))
        slack = tc.bounds(r, 0.0, k_hi)[2]
        assert status[b] == 0 and (dist[b] <= r.T[rows, sface[b]] + slack[rows, sface[b]]).all()
        assert (r.T[rows, sface[b]] <= 8 * U * np.abs(v).max()).all()                          # the premise: two fmas, each within u of a coordinate
        same = face[b] == sface[b]
        assert same.mean() > 0.5 and np.array_equal(normal[b][same].view(np.uint32), nrm[b][same].view(np.uint32))
        print("own samples mesh %d: largest distance %.3g, %d of %d name the sample's face" % (b, dist[b].max(), same.sum(), len(same)))


def test_a_triangle_is_never_farther_than_a_point_on_it():
    """d_tri <= d_nn to the mesh's samples. nn_points' distance is within 8 u (relative) of |q - p_j|; p_j lies within 8 u L of its face f_j (the
    premise above: 8 u max |v|); the device's d_tri is at most T_fj + slack_fj: d_tri <= d_nn (1 + 8 u) + 8 u max |v| + slack at face f_j."""
    from forge_amd import ops
    from forge_amd.geometry import Mesh, point_mesh_distance
    meshes, (pts, _, sface, _), _ = own_samples()
    v, f = meshes[1]
    q = tc.queries_for(v, f, 300, 81)
    d2, idx = ops.nn_points(dev(q[None]), dev(pts[1][None]))
    hit = point_mesh_distance(dev(q), Mesh(dev(v), torch.zeros(len(v), 3, device="cuda"), dev(f)))
    r = tc.restate(q, v, f)
    rows = np.arange(len(q))
    fj = sface[1][idx[0].cpu().numpy()]
    slack = tc.bounds(r, 0.0, K()[1])[2][rows, fj]
    d_nn, d_tri = np.sqrt(d2[0].cpu().numpy().astype(np.float64)), hit.distance[0].cpu().numpy().astype(np.float64)
    assert (d_tri <= d_nn * (1 + 8 * U) + 8 * U * np.abs(v).max() + slack).all()
    assert (d_tri < d_nn).mean() > 0.5                                                          # and it matters: most are strictly nearer


def test_nan_never_wins_and_empty_sides():
    from forge_amd import ops
    v, f, q = blob8_rows()
    F = len(f)
    V, Fm, cnt = dev(v[None]), dev(f[None]), dev(np.array([[len(v), F]], np.int32))
    vn = v.copy()
    only = np.setdiff1d(np.unique(f[:40]), np.unique(f[40:]))          # vertices of the first 40 faces alone: NaN there spoils only those faces
    vn[only, 1] = np.nan
    spoiled = np.isin(f, only).any(axis=1)
    keep = ops.nn_triangles(dev(q[:1]), dev(v[None]), dev(f[None][:, ~spoiled]), dev(np.array([[len(v), int((~spoiled).sum())]], np.int32)))
    d2, face, _, _ = ops.nn_triangles(dev(q[:1]), dev(vn[None]), Fm, cnt)
    assert spoiled.any() and torch.equal(d2, keep[0]) and torch.equal(face, dev(np.flatnonzero(~spoiled).astype(np.int32))[keep[1].long()])
    qn = q[:1].copy()
    qn[0, ::3, 2] = np.nan
    d2, face, closest, normal = ops.nn_triangles(dev(qn), V, Fm, cnt, want_closest=True, want_normal=True)
    assert torch.isposinf(d2[0, ::3]).all() and (face[0, ::3] == -1).all() and (closest[0, ::3] == 0).all() and (normal[0, ::3] == 0).all()
    assert torch.isfinite(d2[0, 1::3]).all() and (face[0, 1::3] >= 0).all()
    bad = np.array([[0, 0, 1], [0, 1, len(v)], [-1, 0, 1], [5, 5, 5]], np.int32)
    d2, face, _, _ = ops.nn_triangles(dev(q[:1]), V, dev(bad[None]), dev(np.array([[len(v), 4]], np.int32)))
    assert torch.isposinf(d2).all() and (face == -1).all()
    d2, face, _, _ = ops.nn_triangles(dev(q[:1]), V, Fm, dev(np.array([[len(v), 0]], np.int32)), q_count=dev(np.array([100], np.int32)))
    assert torch.isposinf(d2[0, :100]).all() and (d2[0, 100:] == 0).all() and (face == -1).all()


# ----------------------------------------------------------------------------------------------------------------------- the reduction
def test_geom_metrics_hits_matches_the_float64_reduction():
    """Row-aligned normals: everything but the normal term is forge_geom_metrics' own arithmetic (bit-equal to it, and within the 1e-12 of
    its test against geom_cases.metrics); the normal term against a float64 sum of |n_from[i] . hit[i]| over the valid rows. Fed hit = the
    other side's normals gathered through idx, the two entries agree in every bit."""
    from forge_amd import ops
    Na, Nb = 265, 515
    a, b = gc.uniform_points((3, Na, 3), 51), gc.uniform_points((3, Nb, 3), 52)
    na_, nb_ = gc.sphere_points(3 * Na, seed=53)[1].reshape(3, Na, 3), gc.sphere_points(3 * Nb, seed=54)[1].reshape(3, Nb, 3)
    ha, hb = gc.sphere_points(3 * Na, seed=55)[1].reshape(3, Na, 3).copy(), gc.sphere_points(3 * Nb, seed=56)[1].reshape(3, Nb, 3).copy()
    ha[:, ::7] = 0                                                                      # queries without a hit: they add 0
    ca, cb = np.array([Na, 0, Na // 2], np.int32), np.array([Nb // 3, Nb, 0], np.int32)
    taus = (0.05, 0.1, 0.2, 0.4)
    for counts in (False, True):
        qa, qb = (dev(ca), dev(cb)) if counts else (None, None)
        d2ab, iab = ops.nn_points(dev(a), dev(b), qa, qb)
        d2ba, iba = ops.nn_points(dev(b), dev(a), qb, qa)
        plain, pstatus = ops.geom_metrics(d2ab, iab, d2ba, iba, dev(na_), dev(nb_), qa, qb, taus)
        out, status = ops.geom_metrics_hits(d2ab, dev(ha), d2ba, dev(hb), dev(na_), dev(nb_), qa, qb, taus)
        nc = gc.OUT["normal_consistency"]
        others = [k for k in range(gc.OUT_DOUBLES) if k != nc]
        assert torch.equal(status, pstatus) and torch.equal(torch.nan_to_num(out[:, others], nan=-1.0), torch.nan_to_num(plain[:, others], nan=-1.0))
        out = out.cpu().numpy()
        for k in range(3):
            ref, st = gc.metrics(d2ab[k].cpu().numpy(), iab[k].cpu().numpy(), d2ba[k].cpu().numpy(), iba[k].cpu().numpy(), None, None,
                                 ca[k] if counts else None, cb[k] if counts else None, taus)
            n1, n2 = (int(ca[k]), int(cb[k])) if counts else (Na, Nb)
            with np.errstate(invalid="ignore"):
                ref[nc] = 0.5 * (np.abs((na_[k, :n1].astype(np.float64) * ha[k, :n1]).sum(1)).sum() / np.float64(n1)
                                 + np.abs((nb_[k, :n2].astype(np.float64) * hb[k, :n2]).sum(1)).sum() / np.float64(n2))
            assert status[k] == st
            np.testing.assert_allclose(out[k], ref, rtol=1e-12, atol=0, equal_nan=True)
        none, _ = ops.geom_metrics_hits(d2ab, None, d2ba, None, None, None, qa, qb, taus)
        assert torch.isnan(none[:, nc]).all() and torch.equal(torch.nan_to_num(none[:, others], nan=-1.0), torch.nan_to_num(plain[:, others], nan=-1.0))
    gathered = lambda n, i: torch.where(i[..., None] >= 0, torch.gather(dev(n), 1, i.clamp_min(0).long()[..., None].expand(-1, -1, 3)),      # noqa: E731
                                        torch.zeros((), device="cuda")).contiguous()
    d2ab, iab = ops.nn_points(dev(a), dev(b))
    d2ba, iba = ops.nn_points(dev(b), dev(a))
    one, _ = ops.geom_metrics(d2ab, iab, d2ba, iba, dev(na_), dev(nb_), thresholds=taus)
    two, _ = ops.geom_metrics_hits(d2ab, gathered(nb_, iab), d2ba, gathered(na_, iba), dev(na_), dev(nb_), thresholds=taus)
    assert torch.equal(one, two)


# -------------------------------------------------------------------------------------------------------------------------- end to end
def blobs16():
    if "blobs16" not in _CACHE:
        from forge_amd.geometry import extract_mesh
        dens = torch.from_numpy(np.stack([mc.blob(16), mc.blob(16, (0.05, 0.0, 0.0))])[:, None]).cuda()
        _CACHE["blobs16"] = extract_mesh(dens)
    return _CACHE["blobs16"]


def _np_mesh(m):
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy()


def test_mesh_metrics_triangles_end_to_end():
    """The blob against the blob shifted by 0.05, n samples a side, against the restatement fed the device's own samples: every distance lies
    between its lower and its upper bound, so accuracy / completeness / chamfer_l1 lie between the means of the bounds and hausdorff between
    their maxima (float64 sums: 1e-12). Normal consistency against the float64 normals of the named faces."""
    from forge_amd.geometry import mesh_metrics, point_metrics, sample_surface
    m0, m1 = blobs16()
    n = 1500
    res = mesh_metrics(m0, m1, n=n, surface="triangles")
    k_lo, k_hi = K()
    means, maxima = [], []
    for src, dst in ((m0, m1), (m1, m0)):
        pts = sample_surface(src, n)[0][0].cpu().numpy()
        lower, upper, _ = tc.bounds(tc.restate(pts, *_np_mesh(dst)), k_lo, k_hi)
        means.append((lower.mean(), upper.mean()))
        maxima.append((lower.max(), upper.max()))
    for key, (lo, hi) in (("accuracy", means[0]), ("completeness", means[1]),
                          ("chamfer_l1", (0.5 * (means[0][0] + means[1][0]), 0.5 * (means[0][1] + means[1][1]))),
                          ("hausdorff", (max(maxima[0][0], maxima[1][0]), max(maxima[0][1], maxima[1][1])))):
        assert lo * (1 - 1e-12) <= float(res[key][0]) <= hi * (1 + 1e-12), (key, lo, float(res[key][0]), hi)
    assert int(res["status"][0]) == 0 and float(res["normal_consistency"][0]) > 0.9
    assert 0 <= float(res["fscore@0.01"][0]) <= float(res["fscore@0.02"][0]) <= float(res["fscore@0.05"][0]) <= 1.0
    # a mesh against itself: 0 up to the tolerance with triangles, at any n; the sampling floor with samples of two different n
    same = mesh_metrics(m0, m0, n=n, surface="triangles")
    pts = sample_surface(m0, n)[0][0].cpu().numpy()
    r = tc.restate(pts, *_np_mesh(m0))
    tol = float(tc.bounds(r, k_lo, k_hi)[1].mean())
    pa, pb = sample_surface(m0, n)[0], sample_surface(m0, n + 37)[0]
    floor = float(point_metrics(pa, pb)["chamfer_l1"][0])
    spacing = float(np.sqrt(float(m0.area()) / n))
    print("triangles: self chamfer_l1 %.3g (tolerance %.3g); samples of n and n + 37: %.3g (spacing %.3g); m0 vs m1 %.6f, samples mode %.6f"
          % (float(same["chamfer_l1"][0]), tol, floor, spacing, float(res["chamfer_l1"][0]), float(mesh_metrics(m0, m1, n=n)["chamfer_l1"][0])))
    assert float(same["chamfer_l1"][0]) <= tol < 1e-6 and float(same["fscore@0.01"][0]) == 1.0 and float(same["normal_consistency"][0]) > 0.999
    assert floor > 0.1 * spacing > 100 * tol
    # a point cloud as ground truth: nearest points one way, triangles the other, no normal consistency
    cloud = mesh_metrics(m0, sample_surface(m1, n)[0], n=n, surface="triangles")
    assert float(cloud["completeness"][0]) == float(res["completeness"][0]) and torch.isnan(cloud["normal_consistency"]).all()
    assert float(cloud["accuracy"][0]) >= float(res["accuracy"][0])
    with pytest.raises(ValueError, match="surface"):
        mesh_metrics(m0, m1, n=n, surface="faces")


def test_mesh_metrics_triangles_transform_undoes_a_known_shift():
    """The prediction is m0 moved by t = (0.0625, -0.03125, 0.125) (each vertex rounds once: within u |v| of the exact shift); transform = the
    inverse shift. Under it every sample is within 2 u |v| sqrt(3) of m0's surface, plus the tolerance of the search: chamfer_l1 and hausdorff
    are at most that, against about |t| without the transform."""
    from forge_amd.geometry import Mesh, mesh_metrics, sample_surface
    m0, _ = blobs16()
    n = 1000
    t = torch.tensor([0.0625, -0.03125, 0.125], device="cuda")
    moved = Mesh(m0.vertices + t, m0.normals, m0.faces)
    T = torch.eye(4, device="cuda")
    T[:3, 3] = -t
    res = mesh_metrics(moved, m0, n=n, surface="triangles", transform=T)
    off = mesh_metrics(moved, m0, n=n, surface="triangles")
    k_lo, k_hi = K()
    pts = sample_surface(m0, n)[0][0].cpu().numpy()
    tol = float(tc.bounds(tc.restate(pts, *_np_mesh(m0)), k_lo, k_hi)[1].max()) + 4 * np.sqrt(3) * U * float(moved.vertices.abs().max())
    print("shift: chamfer_l1 %.3g hausdorff %.3g under the transform (tolerance %.3g), %.4f without" % (
        float(res["chamfer_l1"][0]), float(res["hausdorff"][0]), tol, float(off["chamfer_l1"][0])))
    assert float(res["hausdorff"][0]) <= tol and float(res["chamfer_l1"][0]) <= tol and float(res["normal_consistency"][0]) > 0.999
    assert float(off["chamfer_l1"][0]) > 0.02
    batch = mesh_metrics([moved, moved], [m0, m0], n=n, surface="triangles", transform=torch.stack([T, torch.eye(4, device="cuda")]))
    assert float(batch["chamfer_l1"][0]) == float(res["chamfer_l1"][0]) and float(batch["chamfer_l1"][1]) == float(off["chamfer_l1"][0])


# ------------------------------------------------------------------------------------------------------------------------- integration
def test_samples_mode_is_what_it_was():
    from forge_amd.geometry import mesh_metrics
    m0, m1 = blobs16()
    a, b = mesh_metrics(m0, m1, n=2048), mesh_metrics(m0, m1, n=2048, surface="samples")
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_the_triangles_chain_runs_in_a_captured_graph():
    """extract_mesh with capacities -> mesh_metrics(surface="triangles") on the MeshBatches: no host synchronisation anywhere (a synchronising
    call inside the capture raises). Captured once, replayed twice: identical to the eager call."""
    from forge_amd.geometry import extract_mesh, mesh_metrics
    dens = torch.from_numpy(np.stack([mc.blob(8), mc.blob(8, (0.05, -0.03, 0.02)), mc.below(8)])[:, None]).cuda()
    other = torch.from_numpy(np.stack([mc.blob(8, (0.0, 0.04, 0.0)), mc.blob(8), mc.blob(8)])[:, None]).cuda()
    T = torch.eye(4, device="cuda")
    T[1, 3] = 0.01

    def chain():
        a = extract_mesh(dens, max_vertices=600, max_faces=1100)
        b = extract_mesh(other, max_vertices=600, max_faces=1100)
        return mesh_metrics(a, b, n=500, surface="triangles", transform=T)

    eager = {k: v.clone() for k, v in chain().items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = chain()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, v in eager.items():
            assert torch.equal(torch.nan_to_num(res[k].double(), nan=-1.0), torch.nan_to_num(v.double(), nan=-1.0)), k      # NaN == NaN here
    assert eager["status"].cpu().tolist() == [0, 0, 1] and torch.isnan(eager["chamfer_l1"][2]) and float(eager["chamfer_l1"][0]) > 0


def test_ops_refuse_before_any_launch():
    import ctypes
    from forge_amd import _lib, ops
    q = torch.zeros(2, 8, 3, device="cuda")
    v, f, c = torch.zeros(2, 4, 3, device="cuda"), torch.zeros(2, 5, 3, dtype=torch.int32, device="cuda"), torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        ops.nn_triangles(q.double(), v, f, c)
    with pytest.raises(TypeError):
        ops.nn_triangles(q, v, f.long(), c)
    with pytest.raises(ValueError, match="contiguous"):
        ops.nn_triangles(torch.zeros(2, 8, 6, device="cuda")[..., ::2], v, f, c)
    with pytest.raises(ValueError):
        ops.nn_triangles(q, v, f, c, xf_mesh=torch.zeros(2, 16, device="cuda"))
    with pytest.raises(ValueError):
        ops.nn_triangles(q, v[0], f[0], c)                                     # packed rows without offsets
    with pytest.raises(RuntimeError, match="HIP|cuda|device"):
        ops.nn_triangles(q, v.cpu(), f, c)
    need = _lib.size_query("forge_nn_triangles_workspace_bytes", 2, 5, 0)
    assert need == 2 * 5 * 48 + 16
    with pytest.raises(ValueError, match="workspace"):
        ops.nn_triangles(q, v, f, c, workspace=torch.zeros(need - 1, dtype=torch.uint8, device="cuda"))
    d2, face = torch.zeros(2, 8, device="cuda"), torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    P, L = _lib.ptr, _lib.lib()
    call = lambda w, nbytes: L.forge_nn_triangles(P(q), None, None, P(v), P(f), P(c), None, None, 2, 8, 4, 5, w, nbytes, P(d2), P(face), None, None, None)      # noqa: E731
    assert call(None, need) != 0 and "null" in L.forge_last_error().decode()
    assert call(P(ws), need - 1) != 0 and "workspace" in L.forge_last_error().decode()
    assert call(ctypes.c_void_p(ws.data_ptr() + 4), need) != 0 and "aligned" in L.forge_last_error().decode()
    assert call(P(ws), need) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="all|none"):
        ops.geom_metrics_hits(d2, torch.zeros(2, 8, 3, device="cuda"), d2, None)
    with pytest.raises(TypeError):
        ops.geom_metrics_hits(d2, q.double(), d2, q, q, q)
    with pytest.raises(ValueError, match="thresholds"):
        ops.geom_metrics_hits(d2, None, d2, None, thresholds=(0.1,) * 5)
