"""Mesh extraction on the MI355X (forge_amd.geometry.extract_mesh -> csrc/mesh.hip) against the float64 numpy restatement of its contract
(tests/mesh_cases.py): faces and counts integer for integer, vertices / features / normals within bounds derived from the fp32 expression order."""
import numpy as np
import pytest
import torch

import mesh_cases as mc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff

# name -> (list of density volumes, level, volume_size, feature channels or 0)
CASES = {
    "blob4": ([mc.blob(4)], 0.5, 1.0, 0),
    "blob8_features": ([mc.blob(8)], 0.5, 1.0, 8),
    "blob16_off_centre": ([mc.blob(16, (0.05, -0.03, 0.02))], 0.5, 1.0, 0),
    "noncubic_6x5x7_features": ([mc.noncubic()], mc.QUANT_LEVEL, 1.5, 4),
    "quantised8": ([mc.quantised((8, 8, 8), 3)], mc.QUANT_LEVEL, 1.0, 0),
    "two_blobs8_features": ([mc.blob(8, (0.06, -0.04, 0.02)), mc.blob(8, (-0.05, 0.03, -0.07))], 0.5, 1.0, 4),
}
_CACHE = {}


def case(name):
    """(density [n,1,D,H,W] cuda, features cuda or None, list of RefMesh, level, volume_size): built once, never modified."""
    if name not in _CACHE:
        vols, level, vs, C = CASES[name]
        feats = [mc.random_features(C, v.shape, 11 + i) for i, v in enumerate(vols)] if C else [None] * len(vols)
        refs = [mc.reference_mesh(v, level, vs, f) for v, f in zip(vols, feats)]
        dens = torch.from_numpy(np.stack(vols)[:, None]).cuda()
        fdev = torch.from_numpy(np.stack(feats)).cuda().contiguous(memory_format=torch.channels_last_3d) if C else None
        _CACHE[name] = (dens, fdev, refs, level, vs)
    return _CACHE[name]


def extract(name, **kw):
    from forge_amd.geometry import extract_mesh
    dens, feats, refs, level, vs = case(name)
    return extract_mesh(dens, level=level, volume_size=vs, features=feats, **kw), refs


@pytest.mark.parametrize("name", list(CASES))
def test_faces_and_counts_are_exact(name):
    meshes, refs = extract(name)
    assert len(meshes) == len(refs)
    for m, r in zip(meshes, refs):
        assert m.faces.dtype == torch.int32 and m.vertices.dtype == torch.float32 and m.normals.dtype == torch.float32
        assert tuple(m.vertices.shape) == r.vertices.shape and tuple(m.normals.shape) == r.normals.shape
        assert len(r.faces) > 0
        assert np.array_equal(m.faces.cpu().numpy(), r.faces)           # indices are per volume, in the contract's order


@pytest.mark.parametrize("name", list(CASES))
def test_vertices(name):
    """Per coordinate, in units of u volume_size (u = 2^-24), following the kernel's expression order for an axis of N samples:
      t = (level - d_a) / (d_b - d_a): two correctly rounded differences and a quotient, |dt| <= 3 u t <= 3 u index units   -> 3 / N
      idx = a + t (b - a): the product is exact, one rounding <= u |idx|, |idx| <= N                                          -> 1
      q = (2 idx) / (N - 1): one rounding <= u |q|, |q| <= 2 N / (N - 1), times e = 0.5 (N - 1) volume_size / N               -> 1
      q - 1: one rounding <= u (N + 1) / (N - 1), times e                                                                     -> 0.5 (N + 1) / N
      (q - 1) e: one rounding <= u |result| <= u (N + 1) / (2 N) volume_size                                                  -> 0.5 (N + 1) / N
      e rounded to fp32 once: <= u |result|                                                                                   -> 0.5 (N + 1) / N
    Sum at the smallest N used here (4): 0.75 + 1 + 1 + 3 x 0.625 = 4.6 < 6, the bound the contract states; smaller for larger N."""
    meshes, refs = extract(name)
    vs = case(name)[4]
    for m, r in zip(meshes, refs):
        err = np.abs(m.vertices.cpu().numpy().astype(np.float64) - r.vertices).max()
        print("%s: vertex error %.2f u volume_size" % (name, err / (U * vs)))
        assert err <= 6 * U * vs


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][3]])
def test_vertex_features(name):
    """f_a + t (f_b - f_a) as fmaf(t, f_b - f_a, f_a): |dt| <= 3 u on a factor |f_b - f_a|, the difference's rounding u |f_b - f_a|, the fma's
    rounding u max(|f_a|, |f_b|): at most 5 u (|f_a| + |f_b|) to first order; 6 u with room for the second-order terms."""
    meshes, refs = extract(name)
    for m, r in zip(meshes, refs):
        assert tuple(m.features.shape) == r.features.shape
        err = np.abs(m.features.cpu().numpy().astype(np.float64) - r.features)
        print("%s: feature error %.2f u (|f_a| + |f_b|)" % (name, (err / (U * r.feat_scale + 1e-300)).max()))
        assert (err <= 6 * U * r.feat_scale).all()


@pytest.mark.parametrize("name", list(CASES))
def test_normals(name):
    """Compared where the float64 lerped gradient is at least 1e-3 of the larger endpoint gradient norm. The error of the lerped gradient is
    relative to the ENDPOINT gradients, so the angle error grows with ratio = max(|g_a|, |g_b|) / |lerp|. Measured on the CPU, restatement in fp32
    against restatement in float64 over blobs at D = 4, 8, 16, the ellipsoid, the torus, all-ones and both random fields:
    max |n32 - n64| / (u ratio) = 2.03 (the quantised 8^3 field; 1.4 - 1.6 on the smooth fields). Allowed: 4 x that."""
    meshes, refs = extract(name)
    for m, r in zip(meshes, refs):
        keep = r.grad_norm >= 1e-3 * r.grad_end_norm
        excluded = 1.0 - keep.mean()
        assert excluded <= 0.01
        if name.startswith("blob") or name.startswith("two_blobs"):
            assert excluded == 0.0
        got = m.normals.cpu().numpy().astype(np.float64)
        chord = np.linalg.norm(got - r.normals, axis=1)[keep]
        ratio = (r.grad_end_norm / r.grad_norm)[keep]
        print("%s: normal error %.2f u ratio" % (name, (chord / (U * ratio)).max()))
        assert (chord <= 4 * 2.03 * U * ratio).all()
        assert np.abs(np.linalg.norm(got[keep], axis=1) - 1.0).max() <= 4 * U


def test_border_case_is_closed():
    from forge_amd.geometry import extract_mesh
    (m,) = extract_mesh(torch.ones(1, 1, 4, 4, 4, device="cuda"))
    r = mc.reference_mesh(mc.ones(4))
    f = m.faces.cpu().numpy()
    assert np.array_equal(f, r.faces)
    assert mc.directed_edges_paired(f) and mc.euler_characteristic(m.vertices.shape[0], f) == 2
    assert float(m.volume()) == pytest.approx(61.25 / 64, rel=1e-5)
    assert float(m.area()) > 0


def test_empty_case():
    from forge_amd.geometry import extract_mesh
    dens = torch.from_numpy(np.stack([mc.below(4), mc.blob(4)])[:, None]).cuda()
    feats = torch.zeros(2, 4, 4, 4, 4, device="cuda").contiguous(memory_format=torch.channels_last_3d)
    empty, full = extract_mesh(dens, features=feats)
    assert tuple(empty.vertices.shape) == (0, 3) and tuple(empty.normals.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3)
    assert tuple(empty.features.shape) == (0, 4)
    assert full.faces.shape[0] > 0
    assert float(empty.volume()) == 0.0 and float(empty.area()) == 0.0
    (alone,) = extract_mesh(dens[:1])
    assert alone.vertices.shape[0] == 0 and alone.faces.shape[0] == 0


def test_frame_axis_order():
    from forge_amd.geometry import extract_mesh
    (m,) = extract_mesh(torch.from_numpy(mc.ellipsoid(16)[None, None]).cuda())
    v = m.vertices.cpu().numpy()
    for a in range(3):                                              # (x, y, z) <-> (W, H, D): radii 0.40, 0.30, 0.20, to within h = 1/16
        assert abs(v[:, a].max() - mc.ELLIPSOID_RADII[a]) <= 1.0 / 16
        assert abs(v[:, a].min() + mc.ELLIPSOID_RADII[a]) <= 1.0 / 16


def test_determinism():
    a, _ = extract("two_blobs8_features")
    b, _ = extract("two_blobs8_features")
    for x, y in zip(a, b):
        for s, t in ((x.vertices, y.vertices), (x.normals, y.normals), (x.faces, y.faces), (x.features, y.features)):
            assert torch.equal(s.view(torch.int32), t.view(torch.int32))


# --------------------------------------------------------------------------------------------------------------------- capacity mode
CANARY_F, CANARY_I = -7.25, -77


def _emit_with_canaries(dens, mv, mf):
    """ops.mesh_emit into views of larger buffers filled with a canary value; returns the outputs and the buffers."""
    from forge_amd import ops
    n = dens.shape[0]
    counts, ws = ops.mesh_count(dens, 0.5)
    vb = torch.full((n * mv * 3 + 96,), CANARY_F, device="cuda")
    nb = torch.full((n * mv * 3 + 96,), CANARY_F, device="cuda")
    fb = torch.full((n * mf * 3 + 96,), CANARY_I, dtype=torch.int32, device="cuda")
    out = (vb[:n * mv * 3].view(n, mv, 3), nb[:n * mv * 3].view(n, mv, 3), fb[:n * mf * 3].view(n, mf, 3), None)
    v, nr, f, _, status = ops.mesh_emit(dens, ws, counts, mv, mf, 0.5, 1.0, out=out)
    return v, nr, f, counts, status, (vb, nb, fb)


@pytest.mark.parametrize("mv,mf", [(100, 250), (400, 250), (100, 700), (302, 600), (400, 700)])
def test_capacity_mode_prefix_overflow_and_canary(mv, mf):
    from forge_amd import ops
    from forge_amd.geometry import extract_mesh
    dens = torch.from_numpy(np.stack([mc.blob(8), mc.below(8)])[:, None]).cuda()
    full = extract_mesh(dens)[0]
    nv, nf = full.vertices.shape[0], full.faces.shape[0]
    assert (nv, nf) == (302, 600)                                  # the restatement's counts for this blob
    v, nr, f, counts, status, bufs = _emit_with_canaries(dens, mv, mf)
    assert counts.cpu().tolist() == [[nv, nf], [0, 0]]             # the full need, whatever the capacity
    assert status.cpu().tolist() == [ops.MESH_OVERFLOW if (mv < nv or mf < nf) else 0, 0]
    kv, kf = min(mv, nv), min(mf, nf)
    assert torch.equal(v[0, :kv], full.vertices[:kv]) and torch.equal(nr[0, :kv], full.normals[:kv]) and torch.equal(f[0, :kf], full.faces[:kf])
    # nothing else was written: the rest of volume 0's rows, all of the empty volume 1's rows, and the region behind the capacity
    assert (v[0, kv:] == CANARY_F).all() and (nr[0, kv:] == CANARY_F).all() and (f[0, kf:] == CANARY_I).all()
    assert (v[1] == CANARY_F).all() and (nr[1] == CANARY_F).all() and (f[1] == CANARY_I).all()
    vb, nb, fb = bufs
    assert (vb[-96:] == CANARY_F).all() and (nb[-96:] == CANARY_F).all() and (fb[-96:] == CANARY_I).all()


def test_capacity_mode_features_prefix():
    from forge_amd import ops
    from forge_amd.geometry import extract_mesh
    dens, feats, _, level, vs = case("two_blobs8_features")
    full = extract_mesh(dens, level=level, volume_size=vs, features=feats)
    batch = extract_mesh(dens, level=level, volume_size=vs, features=feats, max_vertices=128, max_faces=1024)
    assert batch.status.cpu().tolist() == [ops.MESH_OVERFLOW, ops.MESH_OVERFLOW]
    for i, m in enumerate(full):
        assert batch.counts[i].cpu().tolist() == [m.vertices.shape[0], m.faces.shape[0]]
        assert torch.equal(batch.features[i], m.features[:128]) and torch.equal(batch.vertices[i], m.vertices[:128])
        nf = m.faces.shape[0]
        assert torch.equal(batch.faces[i, :nf], m.faces) and (batch.faces[i, nf:] == 0).all()


def test_capacity_mode_runs_in_a_captured_graph():
    """No host synchronisation: a synchronising call inside torch.cuda.graph capture raises. Captured once, replayed once."""
    from forge_amd.geometry import extract_mesh
    dens, feats, _, level, vs = case("two_blobs8_features")
    full = extract_mesh(dens, level=level, volume_size=vs, features=feats)
    static = dens.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch = extract_mesh(static, level=level, volume_size=vs, features=feats, max_vertices=512, max_faces=1024)
    g.replay()
    torch.cuda.synchronize()
    assert batch.status.cpu().tolist() == [0, 0]
    for i, m in enumerate(full):
        nv, nf = m.vertices.shape[0], m.faces.shape[0]
        assert batch.counts[i].cpu().tolist() == [nv, nf]
        assert torch.equal(batch.vertices[i, :nv], m.vertices) and torch.equal(batch.normals[i, :nv], m.normals)
        assert torch.equal(batch.faces[i, :nf], m.faces) and torch.equal(batch.features[i, :nv], m.features)
        assert (batch.vertices[i, nv:] == 0).all() and (batch.faces[i, nf:] == 0).all()


def test_ops_check_dtype_and_strides():
    from forge_amd import ops
    d = torch.zeros(1, 1, 4, 4, 4, device="cuda")
    with pytest.raises(TypeError):
        ops.mesh_count(d.double())
    with pytest.raises(ValueError, match="contiguous"):
        ops.mesh_count(torch.zeros(1, 1, 4, 4, 8, device="cuda")[..., ::2])
    with pytest.raises(ValueError, match="level"):
        ops.mesh_count(d, level=0.0)
    counts, ws = ops.mesh_count(d)
    with pytest.raises(ValueError, match="channels-last"):
        ops.mesh_emit(d, ws, counts, 4, 4, features=torch.zeros(1, 8, 4, 4, 4, device="cuda"))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.mesh_emit(d, ws, counts, 4, 4, features=torch.zeros(1, 6, 4, 4, 4, device="cuda"))
