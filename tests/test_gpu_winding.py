"""Generalized winding numbers on the MI355X (forge_amd.ops.winding_number, forge_amd.geometry.winding_number / contains / signed_distance /
voxelize / volume_iou, evaluation.evaluate_geometry(iou=...) -> csrc/winding.hip) against the float64 restatement of tests/winding_cases.py
(include/forge_hip.h section g3c). The contract is per query, u = 2^-24:
    |w_dev - w| <= K u (1 / 2 pi) sum_f (kappa_f + |theta_f|),   kappa_f = la lb lc / hypot(num, den), theta_f and kappa_f in float64,
K = 4 x what the header's fp32 order and grouped sum cost in numpy float32 over these same cases (winding_cases.measured_k; the factor covers
v_sqrt_f32 and v_rcp_f32 against numpy's correctly rounded ones, as in tests/test_gpu_tridist.py). Inside / outside is compared wherever the
exact w is farther from the threshold than that tolerance."""
import numpy as np
import pytest
import torch

import geom_cases as gc
import mesh_cases as mc
import winding_cases as wc

pytestmark = pytest.mark.gpu

U = wc.U
_CACHE = {}


def dev(a, dt=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)


def K():
    return 4.0 * wc.measured_k()


def lay_out(vertices, faces, counts, packed, spare=2):
    """The meshes of a batch as device rows, as tests/test_gpu_tridist.py lays them out. Padded: every mesh owns max rows, the rows past its
    count hold a face that WOULD be a candidate (0, 1, 2) - reading them shows. Packed: the meshes one after the other with `spare` such rows
    between them and offsets that skip them."""
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


def mesh_of(v, f):
    from forge_amd.geometry import Mesh
    return Mesh(dev(v), torch.zeros(len(v), 3, device="cuda"), dev(f))


# ------------------------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("iF", range(len(wc.FACES)), ids=["F%d" % F for F in wc.FACES])
@pytest.mark.parametrize("im", range(len(wc.MESHES)), ids=wc.MESHES)
def test_winding_number_within_its_bound_and_classifies(im, iF):
    from forge_amd import ops
    c = wc.case(im, iF)
    V, Fm, counts, offsets = lay_out(c.vertices, c.faces, c.counts, c.packed)
    w = ops.winding_number(dev(c.q), V, Fm, counts, offsets=offsets, q_count=dev(c.q_count), xf_q=dev(c.xf_q), xf_mesh=dev(c.xf_mesh))
    inside = (w > 0.5).cpu().numpy()               # contains' compare: strict, fp32, on the float32 output
    w = w.cpu().numpy()
    k, used, excluded, total = K(), 0.0, 0, 0
    for b in range(3):
        nq = c.Nq if c.q_count is None else int(c.q_count[b])
        r = wc.restated(im, iF, b)
        assert (w[b, nq:] == 0).all()
        tol = k * U * r.scale
        err = np.abs(w[b, :nq].astype(np.float64) - r.w)
        assert (err <= tol).all(), (b, float((err - tol).max()))
        assert (w[b, :nq][r.scale == 0] == 0).all()                  # no candidate: exactly 0
        used = max(used, wc.k_of(r, w[b, :nq]) / k)
        clear = np.abs(r.w - 0.5) > tol
        assert np.array_equal(inside[b, :nq][clear], (r.w > 0.5)[clear])
        excluded, total = excluded + int((~clear).sum()), total + nq
    assert excluded <= 0.01 * total
    print("winding %-16s Nq %3d %s %s: measured K %.3f, allowed x4, the device used %.3f of that; %d of %d queries within their tolerance of 0.5"
          % (c.name, c.Nq, "packed" if c.packed else "padded", "xf" if c.xf else "plain", k / 4, used, excluded, total))


def closed_meshes():
    """[blob8, blob12] whole (closed), 700 queries each, through the geometry surface: a list of Mesh (packed rows)."""
    if "closed" not in _CACHE:
        from forge_amd.geometry import contains, winding_number
        parts = [wc.whole_closed(kind) for kind in wc.CLOSED]
        meshes = [mesh_of(v, f) for v, f, _, _ in parts]
        q = dev(np.stack([p[2] for p in parts]))
        _CACHE["closed"] = (parts, meshes, q, winding_number(q, meshes), contains(q, meshes))
    return _CACHE["closed"]


def test_closed_meshes_give_integers_and_contains_is_exact():
    """On a closed mesh w is 0 or 1 up to the tolerance, no query lies within it of 0.5 (tests/test_winding_cpu.py), so contains equals the
    restatement's on EVERY query. An inward-wound copy gives -1 inside: contains only with absolute=True. counts and transform as documented."""
    from forge_amd.geometry import Mesh, contains, winding_number
    parts, meshes, q, w, inside = closed_meshes()
    k = K()
    for b, (v, f, _, r) in enumerate(parts):
        assert (np.abs(w[b].cpu().numpy().astype(np.float64) - r.w) <= k * U * r.scale).all()
        assert np.array_equal(inside[b].cpu().numpy(), r.w > 0.5) and 0.1 < (r.w > 0.5).mean() < 0.9
    flipped = [Mesh(m.vertices, m.normals, m.faces.flip(1).contiguous()) for m in meshes]
    assert not contains(q, flipped).any() and torch.equal(contains(q, flipped, absolute=True), inside)
    assert torch.equal(contains(q, meshes, threshold=-1.0), torch.ones_like(inside)) and not contains(q, meshes, threshold=1.5).any()
    counts = dev(np.array([100, 0], np.int32))
    cut = winding_number(q, meshes, counts=counts)
    assert torch.equal(cut[0, :100], w[0, :100]) and (cut[0, 100:] == 0).all() and (cut[1] == 0).all()
    assert not contains(q, meshes, counts=counts)[1].any()
    t = torch.tensor([0.0625, -0.03125, 0.125], device="cuda")           # the queries moved by -t, brought back by the transform: exact sums
    T = torch.eye(4, device="cuda")
    T[:3, 3] = t
    moved = winding_number(q - t, meshes, transform=T)
    r_moved = [wc.restate((q[b] - t).cpu().numpy(), parts[b][0], parts[b][1], xf_q=T[:3].reshape(12).cpu().numpy()) for b in range(2)]
    for b in range(2):
        assert (np.abs(moved[b].cpu().numpy().astype(np.float64) - r_moved[b].w) <= k * U * r_moved[b].scale).all()
    one = winding_number(q[0], meshes[0])                                 # [N,3] against one Mesh
    assert one.shape == (1, q.shape[1]) and torch.equal(one[0], w[0])
    with pytest.raises(ValueError, match="point sets"):
        winding_number(q, meshes[:1])


# ------------------------------------------------------------------------------------------------------------------------ special rows
def test_faces_that_are_no_candidates_add_exactly_nothing_and_nan_drops():
    from forge_amd import ops
    v, f = gc.octahedron()                                                # 8 faces: one whole group
    q = wc.queries_for(v, f, 300, 11)
    bad = np.array([[0, 0, 1], [0, 1, len(v)], [-1, 0, 1], [5, 5, 5]], np.int32)
    cnt = lambda n: dev(np.array([[len(v), n]], np.int32))               # noqa: E731
    base = ops.winding_number(dev(q[None]), dev(v[None]), dev(f[None]), cnt(8))
    more = ops.winding_number(dev(q[None]), dev(v[None]), dev(np.concatenate([f, bad])[None]), cnt(12))      # a second group of zeros
    assert torch.equal(base, more) and base.abs().max() > 0.9
    only_bad = ops.winding_number(dev(q[None]), dev(v[None]), dev(bad[None]), cnt(4))
    none = ops.winding_number(dev(q[None]), dev(v[None]), dev(f[None]), cnt(0), q_count=dev(np.array([100], np.int32)))
    assert (only_bad == 0).all() and (none == 0).all()
    empty = ops.winding_number(dev(q[None]), torch.zeros(1, 0, 3, device="cuda"), torch.zeros(1, 0, 3, dtype=torch.int32, device="cuda"),
                               dev(np.zeros((1, 2), np.int32)))
    assert (empty == 0).all()
    qn = q.copy()
    qn[::3, 2] = np.nan                                                   # a NaN query: every term is NaN and drops
    wn = ops.winding_number(dev(qn[None]), dev(v[None]), dev(f[None]), cnt(8))
    assert (wn[0, ::3] == 0).all() and torch.equal(wn[0, 1::3], base[0, 1::3])
    on = ops.winding_number(dev(v[None]), dev(v[None]), dev(f[None]), cnt(8))          # queries ON the vertices: the four faces around drop
    r = wc.restate(v, v, f)
    assert torch.isfinite(on).all() and (np.abs(on[0].cpu().numpy() - r.w) <= K() * U * r.scale).all()
    vn = v.copy()
    vn[4, 1] = np.nan                                                     # a NaN corner spoils the four faces around vertex 4, and only them
    keep = ~np.isin(f, 4).any(axis=1)
    spoiled = ops.winding_number(dev(q[None]), dev(vn[None]), dev(f[None]), cnt(8))
    rk = wc.restate(q, v, f[keep])
    assert (np.abs(spoiled[0].cpu().numpy() - rk.w) <= K() * U * rk.scale).all()


# ---------------------------------------------------------------------------------------------------------------------------- the bits
def test_bits_do_not_depend_on_the_run_the_position_or_the_layout():
    from forge_amd import ops
    c = wc.case(3, 4)                                                     # blob12, 257 faces: two tiles, 700 queries, with transforms
    assert c.F == wc.TILE + 1 and c.Nq == 700 and c.xf
    def run(order, packed):
        order = np.asarray(order)
        V, Fm, counts, offsets = lay_out([c.vertices[b] for b in order], [c.faces[b] for b in order], c.counts[order], packed)
        return ops.winding_number(dev(c.q[order]), V, Fm, counts, offsets=offsets, q_count=dev(None if c.q_count is None else c.q_count[order]),
                                  xf_q=dev(c.xf_q[order]), xf_mesh=dev(c.xf_mesh[order]))
    ident = np.arange(3)
    base = run(ident, False)
    assert torch.equal(base, run(ident, False))
    assert torch.equal(base, run(ident, True))
    order = np.array([2, 0, 1])
    for packed in (False, True):
        assert torch.equal(base[order], run(order, packed))
    alone = run(np.array([1]), True)
    assert torch.equal(alone[0], base[1])


def test_one_replay_of_a_captured_graph_is_the_eager_call():
    from forge_amd import ops
    c = wc.case(2, 5)                                                     # blob8, 513 faces
    V, Fm, counts, offsets = lay_out(c.vertices, c.faces, c.counts, c.packed)
    q, qc, xq, xm = dev(c.q), dev(c.q_count), dev(c.xf_q), dev(c.xf_mesh)
    nbytes = 3 * (c.F + 2) * 48 + 16
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    call = lambda: ops.winding_number(q, V, Fm, counts, offsets=offsets, q_count=qc, xf_q=xq, xf_mesh=xm, workspace=ws)      # noqa: E731
    eager = call().clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and eager.abs().max() > 0


# ------------------------------------------------------------------------------------------------------------------------ round trips
def _volumes(*fields):
    return torch.from_numpy(np.stack(fields)[:, None]).cuda()


@pytest.mark.parametrize("name", ["blob8", "torus12", "noncubic", "quantised8", "batch"])
def test_voxelize_of_an_extraction_is_the_occupancy(name):
    """voxelize(extract_mesh(d, level), d.shape) == (d > level) at EVERY lattice point: the grid points lie off the surface (a vertex sits
    strictly between two of them), the meshes are closed, and w is 0 or 1 there up to rounding."""
    from forge_amd.geometry import extract_mesh, voxelize
    dens, level = {"blob8": (_volumes(mc.blob(8)), 0.5), "torus12": (_volumes(mc.torus(12)), 0.5), "noncubic": (_volumes(mc.noncubic()), mc.QUANT_LEVEL),
                   "quantised8": (_volumes(mc.quantised((8, 8, 8), 5)), mc.QUANT_LEVEL),
                   "batch": (_volumes(mc.blob(8, (0.05, -0.03, 0.02)), mc.quantised((8, 8, 8), 6)), mc.QUANT_LEVEL)}[name]
    shape = tuple(dens.shape[2:])
    occ = voxelize(extract_mesh(dens, level), shape)
    assert occ.dtype == torch.bool and tuple(occ.shape) == (dens.shape[0],) + shape
    assert torch.equal(occ, dens[:, 0] > level) and occ.any() and not occ.all()
    if name == "batch":                                                   # the padded rows of a MeshBatch: the same answer, nothing read back
        batch = extract_mesh(dens, level, max_vertices=8000, max_faces=16000)
        assert int(batch.status.max()) == 0 and torch.equal(voxelize(batch, shape), occ)


def test_voxelize_sees_what_keep_components_kept():
    from forge_amd.geometry import extract_mesh, keep_components, voxelize
    # a blob (radius 0.18 at level 1) and a floater (0.85 of a blob: radius 0.14) 0.55 away from it, and a random field for good measure
    dens = _volumes(np.maximum(mc.blob(16, (-0.2, 0.0, 0.0)), np.float32(0.85) * mc.blob(16, (0.3, 0.2, 0.1))))
    kept = keep_components(dens, 1.0, keep="largest")
    occ = voxelize(extract_mesh(dens, 1.0, components="largest"), (16, 16, 16))
    assert torch.equal(occ, kept[:, 0] > 1.0)
    assert 0 < int(occ.sum()) < int((dens > 1.0).sum())                   # and something was dropped: the two occupancies differ
    assert torch.equal(voxelize(extract_mesh(dens, 1.0), (16, 16, 16)), dens[:, 0] > 1.0)
    rnd = _volumes(mc.quantised((8, 8, 8), 5))
    assert torch.equal(voxelize(extract_mesh(rnd, mc.QUANT_LEVEL, components="largest"), (8, 8, 8)),
                       keep_components(rnd, mc.QUANT_LEVEL, keep="largest")[:, 0] > mc.QUANT_LEVEL)
    half = voxelize(extract_mesh(_volumes(mc.blob(8)), 0.5, volume_size=0.5), (8, 8, 8), volume_size=0.5)
    assert torch.equal(half, _volumes(mc.blob(8))[:, 0] > 0.5)            # the lattice follows volume_size


def test_signed_distance_is_the_distance_with_the_sign_of_contains():
    from forge_amd.geometry import point_mesh_distance, signed_distance
    parts, meshes, q, w, inside = closed_meshes()
    sd, hit = signed_distance(q, meshes), point_mesh_distance(q, meshes)
    assert torch.equal(torch.signbit(sd.distance), inside) and inside.any() and not inside.all()
    assert torch.equal(sd.distance.abs(), hit.distance) and torch.equal(sd.w, w)
    assert torch.equal(sd.face, hit.face) and torch.equal(sd.closest, hit.closest) and torch.equal(sd.normal, hit.normal)
    assert (hit.distance > 0).all()                                       # no query lies on the surface: every sign is a strict one


# ------------------------------------------------------------------------------------------------------------------------- volume IoU
def test_volume_iou():
    from forge_amd import ops
    from forge_amd.geometry import extract_mesh, volume_iou
    n = 20_000
    a, b = mc.blob(32), mc.blob(32, (0.1, -0.05, 0.0))
    m = extract_mesh(_volumes(a, b))
    same = volume_iou(m, m, n=n)
    assert same["iou"].dtype == torch.float64 and same["iou"].tolist() == [1.0, 1.0] and same["status"].tolist() == [0, 0]
    assert torch.equal(same["volume_pred"], same["volume_gt"])
    exact = torch.stack([x.volume() for x in m])
    assert ((same["volume_gt"] - exact).abs() <= 3 / n ** 0.5 * exact).all()
    # the blob against the shifted blob: the lattice IoU of the two occupancies at 32^3
    lattice = float(((a > 0.5) & (b > 0.5)).sum()) / float(((a > 0.5) | (b > 0.5)).sum())
    res = volume_iou(m[:1], m[1:], n=n)
    print("volume_iou: %.5f against the lattice's %.5f at 32^3 (allowed 3 / sqrt(n) = %.5f); volumes %.6f and %.6f against the meshes' %.6f and %.6f"
          % (float(res["iou"][0]), lattice, 3 / n ** 0.5, float(res["volume_pred"][0]), float(res["volume_gt"][0]), float(exact[0]), float(exact[1])))
    assert abs(float(res["iou"][0]) - lattice) <= 3 / n ** 0.5
    # ... and the same pair with the shift undone by the transform: one
    T = torch.eye(4, device="cuda")
    T[:3, 3] = torch.tensor([0.1, -0.05, 0.0], device="cuda")
    undone = float(volume_iou(m[:1], m[1:], n=n, transform=T)["iou"][0])      # what is left: two discretisations of one blob, a tenth of a voxel
    print("volume_iou: %.5f with the shift undone" % undone)                   # (0.003) on a radius of 0.296, three times that in volume
    assert undone > 0.97
    # two disjoint blobs (level 1.2: radius 0.134 around (-0.25, 0, 0) and (0.25, 0, 0))
    two = extract_mesh(_volumes(mc.blob(16, (-0.25, 0.0, 0.0)), mc.blob(16, (0.25, 0.0, 0.0))), 1.2)
    apart = volume_iou(two[:1], two[1:], n=n)
    assert float(apart["iou"][0]) == 0.0 and float(apart["volume_pred"][0]) > 0 and float(apart["volume_gt"][0]) > 0
    # an empty side, in a batch with a full pair, as a list and as a MeshBatch (no read-back)
    dens = _volumes(mc.blob(8), mc.below(8))
    full = _volumes(mc.blob(8), mc.blob(8))
    for pred, gt in ((extract_mesh(dens), extract_mesh(full)), (extract_mesh(dens, max_vertices=600, max_faces=1100), extract_mesh(full, max_vertices=600, max_faces=1100))):
        res = volume_iou(pred, gt, n=2000)
        assert res["status"].tolist() == [0, ops.GEOM_EMPTY] and float(res["iou"][0]) == 1.0 and torch.isnan(res["iou"][1])
        res = volume_iou(gt, pred, n=2000)
        assert res["status"].tolist() == [0, ops.GEOM_EMPTY] and torch.isnan(res["iou"][1])
    alone = volume_iou(extract_mesh(dens[1:]), extract_mesh(dens[1:]), n=100)
    assert alone["status"].tolist() == [ops.GEOM_EMPTY] and torch.isnan(alone["iou"][0])


def test_evaluate_geometry_adds_the_iou_and_keeps_its_default():
    from forge_amd.evaluation import evaluate_geometry
    from forge_amd.geometry import extract_mesh, mesh_metrics, volume_iou
    m = extract_mesh(_volumes(mc.blob(16), mc.blob(16, (0.05, 0.0, 0.0))))
    pred, gt = m[:1], m[1:]
    T = torch.eye(4, device="cuda")
    T[0, 3] = 0.05
    plain, parent = evaluate_geometry(pred, gt, transform=T, n=2000), mesh_metrics(pred, gt, transform=T, n=2000)
    assert list(plain) == list(parent) and all(torch.equal(plain[k], parent[k]) for k in parent)
    res = evaluate_geometry(pred, gt, transform=T, n=2000, iou=True)
    vol = volume_iou(pred, gt, transform=T)
    assert list(res) == list(parent) + ["iou", "volume_pred", "volume_gt", "iou_status"]
    assert all(torch.equal(res[k], parent[k]) for k in parent)
    assert all(torch.equal(res[k], vol[k]) for k in ("iou", "volume_pred", "volume_gt")) and torch.equal(res["iou_status"], vol["status"])
    assert float(res["iou"][0]) > 0.9 > float(volume_iou(pred, gt)["iou"][0])      # a shift of 0.05 on a radius of 0.296: about 0.78 left in place
    few = evaluate_geometry(pred, gt, transform=T, n=2000, iou={"n": 5000})
    assert torch.equal(few["iou"], volume_iou(pred, gt, n=5000, transform=T)["iou"])
    aligned = evaluate_geometry(pred, gt, n=2000, align={"n": 2000, "iterations": 20}, iou={"n": 5000})
    found = aligned["alignment"].transform.to(torch.float32)
    assert torch.equal(aligned["iou"], volume_iou(pred, gt, n=5000, transform=found)["iou"]) and float(aligned["iou"][0]) > 0.9
    with pytest.raises(ValueError, match="iou"):
        evaluate_geometry(pred, gt, n=2000, iou="yes")
