"""Surface metrics on the MI355X (forge_amd.geometry -> csrc/geomdist.hip) against the float64 numpy restatement of their contract
(tests/geom_cases.py, include/forge_hip.h section g3). Every bound is derived from the fp32 expression order the contract states; u = 2^-24."""
import numpy as np
import pytest
import torch

import geom_cases as gc
import mesh_cases as mc

pytestmark = pytest.mark.gpu

U = gc.U
_CACHE = {}


def consts():
    from forge_amd import ops
    return ops.nn_constants()            # Q queries per workgroup, T references per tile


def shapes():
    Q, T = consts()
    return [(1, 1), (1, 2 * T + 3), (Q - 1, T), (Q + 1, T + 1), (3 * Q + 5, 5)]


XF = np.array([[0.99, -0.33, 0.22, 0.25, 0.363, 0.946, -0.11, -0.5, -0.187, 0.187, 1.045, 0.125],      # about 1.1 x a rotation, and a shift
               [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0],
               [0.5, 0, 0, 1.0, 0, 0, -0.5, 0, 0, 0.5, 0, -1.0]], np.float32)


def nn_case(k, counts, transform):
    """(q, p, q_count, p_count, xf as numpy or None; restatement per pair; kernel d2, idx as numpy): built once per case, never modified."""
    key = (k, counts, transform)
    if key not in _CACHE:
        from forge_amd import ops
        Nq, Np = shapes()[k]
        q, p = gc.uniform_points((3, Nq, 3), 100 + k), gc.uniform_points((3, Np, 3), 200 + k)
        qc = np.array([Nq, 0, (Nq + 1) // 2], np.int32) if counts else None
        pc = np.array([(Np + 1) // 2, Np, 0], np.int32) if counts else None
        xf = XF if transform else None
        dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)       # noqa: E731
        d2, idx = ops.nn_points(dev(q, torch.float32), dev(p, torch.float32), dev(qc, torch.int32), dev(pc, torch.int32), dev(xf, torch.float32))
        refs = [gc.nn(q[b], p[b], None if qc is None else qc[b], None if pc is None else pc[b], None if xf is None else xf[b]) for b in range(3)]
        _CACHE[key] = (q, p, qc, pc, xf, refs, d2.cpu().numpy(), idx.cpu().numpy())
    return _CACHE[key]


def _transform_slack(q, xf):
    """e per query: the distance the fp32 fma chain x' = fma(m02, z, fma(m01, y, fma(m00, x, t0))) can move q' away from its float64 value. Three
    roundings per row, each at most u times the magnitude of its result, and every partial result is at most S (1 + u)^2 with
    S = |t0| + |m00 x| + |m01 y| + |m02 z|: |dx'| <= 3 u (1 + 4 u) S per row; e is the 2-norm over the three rows."""
    if xf is None:
        return np.zeros(len(q))
    m = np.abs(xf.astype(np.float64).reshape(3, 4))
    S = np.abs(q.astype(np.float64)) @ m[:, :3].T + m[:, 3]
    return 3 * U * (1 + 4 * U) * np.linalg.norm(S, axis=1)


@pytest.mark.parametrize("transform", [False, True], ids=["plain", "transform"])
@pytest.mark.parametrize("counts", [False, True], ids=["full", "counts"])
@pytest.mark.parametrize("k", range(5))
def test_nn_points(k, counts, transform):
    """d2 = fma(dz, dz, fma(dy, dy, dx dx)) on fp32 differences. Each difference is correctly rounded (relative u), so each square carries 2 u; the
    product and the two fma roundings add 3 u: 5 u in all, asserted as 8 u. This holds even where the winner differs from the float64 one, because
    the minimum of perturbed values is a perturbed minimum. With D the float64 minimum and R the float64 runner-up:
      |d2 - D| <= 8 u D;   idx = argmin wherever R (1 - 16 u) > D (1 + 16 u), i.e. the runner-up is more than 32 u (relative) away;
      always sqrt(d2_64(q, p[idx])) <= sqrt(D) (1 + 8 u), i.e. d2_64(q, p[idx]) <= D (1 + 16 u).
    With a transform the queries the kernel scores lie within e of the float64 q' (e: _transform_slack), so every distance moves by at most e:
      |d2 - D| <= 8 u D + (2 sqrt(D) e + e^2) (1 + 8 u);   idx = argmin wherever (sqrt(R) - e)^2 (1 - 16 u) > (sqrt(D) + e)^2 (1 + 16 u);
      always sqrt(d2_64(q', p[idx])) <= (sqrt(D) + e) (1 + 8 u) + e.
    e = 0 gives back the three bounds without a transform."""
    q, p, qc, pc, xf, refs, d2, idx = nn_case(k, counts, transform)
    Nq, Np = shapes()[k]
    worst = 0.0
    for b in range(3):
        r = refs[b]
        nq = Nq if qc is None else int(qc[b])
        npb = Np if pc is None else int(pc[b])
        assert (d2[b, nq:] == 0).all() and (idx[b, nq:] == -1).all()
        if npb == 0:
            assert np.isinf(d2[b, :nq]).all() and (d2[b, :nq] > 0).all() and (idx[b, :nq] == -1).all()
            continue
        if nq == 0:
            continue
        D, R, got, gi = r["d2"][:nq], r["runner_up"][:nq], d2[b, :nq].astype(np.float64), idx[b, :nq]
        e = _transform_slack(q[b, :nq], None if xf is None else xf[b])
        assert (gi >= 0).all() and (gi < npb).all()
        bound = 8 * U * D + (2 * np.sqrt(D) * e + e * e) * (1 + 8 * U)
        worst = max(worst, float((np.abs(got - D) / np.maximum(bound, 1e-300)).max()))
        assert (np.abs(got - D) <= bound).all()
        clear = np.maximum(np.sqrt(R) - e, 0.0) ** 2 * (1 - 16 * U) > (np.sqrt(D) + e) ** 2 * (1 + 16 * U)
        assert np.array_equal(gi[clear], r["idx"][:nq][clear])
        chosen = ((r["q"][:nq] - r["p"][gi]) ** 2).sum(axis=1)
        assert (np.sqrt(chosen) <= (np.sqrt(D) + e) * (1 + 8 * U) + e).all()
    print("nn_points (Nq, Np) = %s counts=%s transform=%s: error / bound = %.3f" % (shapes()[k], counts, transform, worst))


def test_nn_ties_go_to_the_lowest_index_and_runs_are_identical():
    from forge_amd import ops
    Q, T = consts()
    q = torch.from_numpy(gc.uniform_points((2, Q + 7, 3), 31)).cuda()
    p0 = torch.from_numpy(gc.uniform_points((2, T + 3, 3), 32)).cuda()
    d2, idx = ops.nn_points(q, p0)
    for name, p, expect in (("appended", torch.cat([p0, p0], dim=1).contiguous(), idx),                     # the copy of j sits at j + Np
                            ("interleaved", p0.repeat_interleave(2, dim=1).contiguous(), 2 * idx)):       # the copy of j sits at 2 j + 1
        d2d, idxd = ops.nn_points(q, p)
        assert torch.equal(d2d, d2) and torch.equal(idxd, expect), name
        again = ops.nn_points(q, p)
        assert torch.equal(again[0], d2d) and torch.equal(again[1], idxd), name
    same = ops.nn_points(p0, p0)
    assert (same[0] == 0).all() and torch.equal(same[1], torch.arange(T + 3, dtype=torch.int32, device="cuda").expand(2, -1))


def test_nn_nan_never_wins():
    from forge_amd import ops
    q = torch.from_numpy(gc.uniform_points((1, 9, 3), 41)).cuda()
    p = torch.from_numpy(gc.uniform_points((1, 20, 3), 42)).cuda()
    clean = ops.nn_points(q, p[:, 5:].contiguous())
    p[0, :5, 1] = float("nan")
    d2, idx = ops.nn_points(q, p)
    assert torch.equal(d2, clean[0]) and torch.equal(idx, clean[1] + 5)
    d2, idx = ops.nn_points(q, torch.full_like(p, float("nan")))
    assert torch.isinf(d2).all() and (idx == -1).all()


# --------------------------------------------------------------------------------------------------------------------- surface sampling
def _device_mesh(v, f):
    from forge_amd.geometry import Mesh
    return Mesh(torch.from_numpy(v).cuda(), torch.zeros(len(v), 3, device="cuda"), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda())


def sampled(n):
    """The list path on [octahedron with faces that must not be chosen, the blob's reference mesh]: (meshes as numpy, the five outputs as numpy)."""
    if ("sampled", n) not in _CACHE:
        from forge_amd.geometry import sample_surface
        v0, f0, bad = gc.with_bad_faces(*gc.octahedron())
        m = mc.reference_mesh(mc.blob(8), 0.5)
        meshes = [(v0, f0, bad), (m.vertices.astype(np.float32), m.faces, [])]
        out = sample_surface([_device_mesh(v, f) for v, f, _ in meshes], n)
        _CACHE[("sampled", n)] = (meshes, [t.cpu().numpy() for t in out])
    return _CACHE[("sampled", n)]


@pytest.mark.parametrize("n", [7, 1000, 4099])
def test_sample_surface_properties(n):
    """points = fma(r2, c - a, fma(r1, b - a, a)) per axis: two correctly rounded differences (u |b - a|, u |c - a|, each at most 2 u max|coordinate|
    and scaled by r1, r2 with r1 + r2 <= 1) and two fma roundings (each u times a value inside the triangle's bounding box): within
    4 u max|coordinate| of the float64 value from the returned face and bary."""
    meshes, (points, normals, face, bary, status) = sampled(n)
    r1, r2 = gc.barycentrics(n)
    for k, (v, f, bad) in enumerate(meshes):
        assert status[k] == 0 and points.shape == (2, n, 3) and face.dtype == np.int32
        areas = gc.face_areas(v, f)
        dev = gc.check_systematic(face[k], areas, n)
        assert not np.isin(face[k], bad).any()
        assert np.array_equal(bary[k, :, 0], r1) and np.array_equal(bary[k, :, 1], r2)                      # the integer formula, exactly
        ref = gc.sample_points(v, f, face[k], bary[k, :, 0], bary[k, :, 1])
        err = np.abs(points[k].astype(np.float64) - ref).max()
        print("sample_surface mesh %d n=%d: max |k_f - n A_f / A| = %.3f, point error %.2f u max|coordinate|" % (k, n, dev, err / (U * np.abs(v).max())))
        assert err <= 4 * U * np.abs(v).max()
        vv = v.astype(np.float64)
        fs = f[face[k]]
        cr = np.cross(vv[fs[:, 1]] - vv[fs[:, 0]], vv[fs[:, 2]] - vv[fs[:, 0]])
        cr /= np.linalg.norm(cr, axis=1, keepdims=True)
        assert np.abs(normals[k].astype(np.float64) - cr).max() <= 1e-5                                     # the face normal along the winding


def test_sample_surface_padded_and_list_paths_agree_and_empty_volume():
    from forge_amd import ops
    from forge_amd.geometry import extract_mesh, sample_surface
    dens = torch.from_numpy(np.stack([mc.blob(8), mc.below(8), mc.blob(8, (0.05, -0.03, 0.02))])[:, None]).cuda()
    meshes = extract_mesh(dens)
    batch = extract_mesh(dens, max_vertices=600, max_faces=1100)
    assert batch.status.cpu().tolist() == [0, 0, 0]
    a, b = sample_surface(meshes, 777), sample_surface(batch, 777)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    points, normals, face, bary, status = b
    assert status.cpu().tolist() == [0, ops.GEOM_EMPTY, 0]
    assert (points[1] == 0).all() and (normals[1] == 0).all() and (face[1] == -1).all()
    assert (face[0] >= 0).all() and int(face[0].max()) < meshes[0].faces.shape[0]
    r = points[0].double().norm(dim=1)
    assert float((r - mc.R0).abs().max()) <= 2 * (1.0 / 8) ** 2 + 1e-6                                      # on the extracted sphere (test_mesh_cpu's radius bound)
    assert float((normals[0] * points[0]).sum(dim=1).min()) > 0                                             # outward


# ----------------------------------------------------------------------------------------------------------------------- the reduction
def test_geom_metrics_matches_the_float64_reduction():
    """Fed the kernel's own d2 / idx, so independent of the nearest-neighbour tolerance: float64 sums of at most a few thousand terms in a different
    order differ by far less than 1e-12 relative."""
    from forge_amd import ops
    Q, T = consts()
    Na, Nb = Q + 9, 2 * T + 3
    a, b = gc.uniform_points((3, Na, 3), 51), gc.uniform_points((3, Nb, 3), 52)
    na_, nb_ = gc.sphere_points(3 * Na, seed=53)[1].reshape(3, Na, 3), gc.sphere_points(3 * Nb, seed=54)[1].reshape(3, Nb, 3)
    ca, cb = np.array([Na, 0, Na // 2], np.int32), np.array([Nb // 3, Nb, 0], np.int32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()       # noqa: E731
    taus = (0.05, 0.1, 0.2, 0.4)
    for counts in (False, True):
        qa, qb = (dev(ca), dev(cb)) if counts else (None, None)
        d2ab, iab = ops.nn_points(dev(a), dev(b), qa, qb)
        d2ba, iba = ops.nn_points(dev(b), dev(a), qb, qa)
        for normals, nt in ((True, 4), (False, 2), (True, 0)):
            out, status = ops.geom_metrics(d2ab, iab, d2ba, iba, dev(na_) if normals else None, dev(nb_) if normals else None, qa, qb, taus[:nt])
            out, status = out.cpu().numpy(), status.cpu().numpy()
            for k in range(3):
                ref, st = gc.metrics(d2ab[k].cpu().numpy(), iab[k].cpu().numpy(), d2ba[k].cpu().numpy(), iba[k].cpu().numpy(),
                                     na_[k] if normals else None, nb_[k] if normals else None, ca[k] if counts else None, cb[k] if counts else None,
                                     taus[:nt])
                assert status[k] == st
                np.testing.assert_allclose(out[k], ref, rtol=1e-12, atol=0, equal_nan=True)


# -------------------------------------------------------------------------------------------------------------------------- end to end
def blobs16():
    if "blobs16" not in _CACHE:
        from forge_amd.geometry import extract_mesh
        dens = torch.from_numpy(np.stack([mc.blob(16), mc.blob(16, (0.05, 0.0, 0.0))])[:, None]).cuda()
        _CACHE["blobs16"] = extract_mesh(dens)
    return _CACHE["blobs16"]


def test_mesh_metrics_end_to_end():
    """The blob and the blob shifted by 0.05: every point of one sphere is within 0.05 of the other, so chamfer_l1 is in (0, 0.05]. Against the
    float64 restatement fed the same samples: d2 is within 8 u relative, so each distance within 4 u relative (sqrt), and so are the means."""
    from forge_amd.geometry import mesh_metrics, sample_surface
    m0, m1 = blobs16()
    n = 4096
    res = mesh_metrics(m0, m1, n=n, thresholds=(0.01, 0.02, 0.05))
    cd = float(res["chamfer_l1"][0])
    assert 0 < cd <= 0.05 and int(res["status"][0]) == 0
    assert 0 <= float(res["fscore@0.01"][0]) <= float(res["fscore@0.02"][0]) <= float(res["fscore@0.05"][0]) <= 1.0
    assert float(res["normal_consistency"][0]) > 0.9
    pa, na = (t[0].cpu().numpy() for t in sample_surface(m0, n)[:2])
    pb, nb = (t[0].cpu().numpy() for t in sample_surface(m1, n)[:2])
    ref, _, _, _ = gc.point_metrics(pa, pb, na, nb, thresholds=(0.01, 0.02, 0.05))
    print("end to end: chamfer_l1 %.6f (float64 %.6f), hausdorff %.6f, fscore@0.02 %.4f" % (cd, ref[gc.OUT["chamfer_l1"]], float(res["hausdorff"][0]),
                                                                                        float(res["fscore@0.02"][0])))
    for k in ("accuracy", "completeness", "chamfer_l1", "hausdorff"):
        assert float(res[k][0]) >= ref[gc.OUT[k]] * (1 - 4 * U) and float(res[k][0]) <= ref[gc.OUT[k]] * (1 + 4 * U), k
    assert float(res["chamfer_l2"][0]) == pytest.approx(ref[gc.OUT["chamfer_l2"]], rel=8 * U)
    # a mesh against itself: the same samples on both sides
    same = mesh_metrics(m0, m0, n=n)
    spacing = float(np.sqrt(float(m0.area()) / n))
    assert float(same["accuracy"][0]) <= spacing and float(same["chamfer_l1"][0]) == 0.0 and float(same["fscore@0.01"][0]) == 1.0
    # a point cloud as ground truth: no normals, the same distances
    cloud = mesh_metrics(m0, torch.from_numpy(pb).cuda(), n=n)
    assert float(cloud["chamfer_l1"][0]) == cd and torch.isnan(cloud["normal_consistency"]).all()


def test_mesh_metrics_transform_undoes_the_shift():
    """transform = the inverse shift maps the shifted blob's samples back: what is measured then is the two extractions' discretisation only. Against
    the float64 restatement with the same transform on the same samples: every distance moves by at most e (_transform_slack) on top of the 4 u
    relative of the nearest-neighbour search, and so does every mean and the maximum."""
    from forge_amd.geometry import mesh_metrics, sample_surface
    m0, m1 = blobs16()
    n = 4096
    T = torch.eye(4)
    T[0, 3] = -0.05
    res = mesh_metrics(m1, m0, n=n, transform=T.cuda())
    plain = mesh_metrics(m1, m0, n=n)
    assert float(res["chamfer_l1"][0]) < 0.5 * float(plain["chamfer_l1"][0])
    pa, na = (t[0].cpu().numpy() for t in sample_surface(m1, n)[:2])
    pb, nb = (t[0].cpu().numpy() for t in sample_surface(m0, n)[:2])
    xf = T[:3].reshape(12).numpy()
    ref, _, _, _ = gc.point_metrics(pa, pb, na, nb, thresholds=(0.01, 0.02, 0.05), xf=xf)
    e = float(_transform_slack(pa, xf).max())
    print("transform: chamfer_l1 %.6f (float64 %.6f, untransformed %.6f), e = %.2e" % (float(res["chamfer_l1"][0]), ref[gc.OUT["chamfer_l1"]],
                                                                                     float(plain["chamfer_l1"][0]), e))
    for k in ("accuracy", "completeness", "chamfer_l1", "hausdorff"):
        assert abs(float(res[k][0]) - ref[gc.OUT[k]]) <= 4 * U * ref[gc.OUT[k]] + e * (1 + 4 * U), k
    assert float(res["normal_consistency"][0]) == pytest.approx(ref[gc.OUT["normal_consistency"]], abs=1e-3)
    batch = mesh_metrics([m1, m1], [m0, m0], n=n, transform=torch.stack([T, torch.eye(4)]).cuda())        # one transform per pair
    assert float(batch["chamfer_l1"][0]) == float(res["chamfer_l1"][0]) and float(batch["chamfer_l1"][1]) == float(plain["chamfer_l1"][0])


def test_the_chain_runs_in_a_captured_graph():
    """extract_mesh with capacities -> sample_surface -> point_metrics: no host synchronisation anywhere (a synchronising call inside the capture
    raises). Captured once, replayed twice: identical to the eager call."""
    from forge_amd.geometry import extract_mesh, point_metrics, sample_surface
    dens = torch.from_numpy(np.stack([mc.blob(8), mc.blob(8, (0.05, -0.03, 0.02)), mc.below(8)])[:, None]).cuda()
    other = torch.from_numpy(np.stack([mc.blob(8, (0.0, 0.04, 0.0)), mc.blob(8), mc.blob(8)])[:, None]).cuda()

    def chain():
        a = extract_mesh(dens, max_vertices=600, max_faces=1100)
        b = extract_mesh(other, max_vertices=600, max_faces=1100)
        pa, na, _, _, sa = sample_surface(a, 500)
        pb, nb, _, _, sb = sample_surface(b, 500)
        ca = torch.where(sa != 0, torch.zeros_like(sa), torch.full_like(sa, 500))
        return point_metrics(pa, pb, na, nb, counts_a=ca)

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


def test_ops_check_dtype_and_strides():
    from forge_amd import ops
    q = torch.zeros(1, 8, 3, device="cuda")
    with pytest.raises(TypeError):
        ops.nn_points(q.double(), q)
    with pytest.raises(ValueError, match="contiguous"):
        ops.nn_points(torch.zeros(1, 8, 6, device="cuda")[..., ::2], q)
    with pytest.raises(TypeError):
        ops.nn_points(q, q, q_count=torch.zeros(1, device="cuda"))
    with pytest.raises(ValueError):
        ops.nn_points(q, q, xf=torch.zeros(1, 16, device="cuda"))
    with pytest.raises(ValueError, match="thresholds"):
        ops.geom_metrics(q[..., 0], q[..., 0].int(), q[..., 0], q[..., 0].int(), thresholds=(0.1,) * 5)
    with pytest.raises(ValueError, match="thresholds"):
        ops.geom_metrics(q[..., 0], q[..., 0].int(), q[..., 0], q[..., 0].int(), thresholds=(float("nan"),))
