"""Connected components on the MI355X (forge_amd.geometry.label_components / keep_components -> csrc/components.hip) against the numpy
restatement of include/forge_hip.h section g4 (tests/components_cases.py). Everything is integer arithmetic or a copy of bits, so every
comparison is exact: labels, counts, sizes, boxes, coordinate sums integer for integer, the centroid against the same float64 formula, the
cleaned density as int32 views (NaN payloads, -0.0 and the +0.0 of removed voxels are pinned). Fields are stacked three to a batch, so
per-volume offsets are exercised everywhere; none is larger than 33^3-class."""
import numpy as np
import pytest
import torch

import components_cases as cc
import mesh_cases as mc

pytestmark = pytest.mark.gpu

_DEV = {}
SELECTIONS = (("largest", 1, 0.0), ("all", 1, 0.0), ("all", 2, 0.0), ("all", 10, 0.0), ("all", 1, 0.01), ("all", 1, 1.0), ("largest", 2, 0.01))


def on_device(fs):
    """The batch [n,1,D,H,W] of a tuple of fields on the device, uploaded once and never modified."""
    key = tuple(f.name for f in fs)
    if key not in _DEV:
        _DEV[key] = torch.from_numpy(cc.stack(fs)).cuda()
    return _DEV[key]


def batch_of(name):
    (fs,) = [fs for fs in cc.batches() if any(f.name == name for f in fs)]
    return fs


def padded(rows, kmax, width, dtype):
    """Per-volume statistics rows -> [n,kmax(,width)] with zero rows past each count and the rows past kmax dropped."""
    out = np.zeros((len(rows), kmax) + ((width,) if width else ()), dtype)
    for v, r in enumerate(rows):
        k = min(len(r), kmax)
        out[v, :k] = r[:k]
    return out


def check_statistics(fs, kmax, sizes, bbox, coord_sum, status, centroid=None, volume_size=1.0):
    refs = [cc.reference(f.density, f.level)[1] for f in fs]
    assert sizes.dtype == torch.int32 and bbox.dtype == torch.int32 and coord_sum.dtype == torch.int64 and status.dtype == torch.int32
    assert np.array_equal(sizes.cpu().numpy(), padded([r.sizes for r in refs], kmax, 0, np.int32))
    assert np.array_equal(bbox.cpu().numpy(), padded([r.bbox for r in refs], kmax, 6, np.int32))
    assert np.array_equal(coord_sum.cpu().numpy(), padded([r.coord_sum for r in refs], kmax, 3, np.int64))
    assert status.cpu().tolist() == [1 if r.count > kmax else 0 for r in refs]
    if centroid is not None:
        want = padded([cc.reference_centroid(r.coord_sum, r.sizes, fs[0].shape, volume_size) for r in refs], kmax, 3, np.float64)
        assert centroid.dtype == torch.float64 and np.array_equal(centroid.cpu().numpy(), want)


def test_labels_and_statistics_equal_the_restatement():
    from forge_amd import geometry, ops
    assert ops.COMPONENTS_OVERFLOW == 1
    shapes, mixed = set(), 0
    for fs in cc.batches():
        d = on_device(fs)
        comp = geometry.label_components(d, fs[0].level)
        refs = [cc.reference(f.density, f.level) for f in fs]
        names = [f.name for f in fs]
        assert comp.labels.dtype == torch.int32 and tuple(comp.labels.shape) == (len(fs),) + fs[0].shape
        assert np.array_equal(comp.labels.cpu().numpy(), np.stack([r[0] for r in refs])), names
        counts = [r[1].count for r in refs]
        assert comp.counts.cpu().tolist() == counts, names
        for f, k in zip(fs, counts):
            assert f.K is None or f.K == k, f.name
        kmax = max(counts)
        assert comp.sizes.shape[1] == kmax                                              # the exact allocation of the read-back mode
        _, _, ws = ops.components_label(d, fs[0].level, want_labels=False)
        sizes, bbox, coord_sum, status = ops.components_stats(d, ws, kmax)
        check_statistics(fs, kmax, sizes, bbox, coord_sum, status)
        check_statistics(fs, kmax, comp.sizes, comp.bbox, coord_sum, comp.status, comp.centroid)
        shapes.add(fs[0].shape)
        mixed += len(fs) == 3
    T = cc.tile()
    assert {(1, 1, 1), (1, 1, 40), (2, 3, 5), (7, 8, 9), (9, 7, 17), (17, 33, 15), (33, 9, 8), (T - 1, T, T + 1), (2 * T + 1, T, T - 1),
            (2 * T + 1,) * 3, (T + 3,) * 3} <= shapes and mixed >= 20


def test_centroid_follows_the_volume_size():
    from forge_amd import geometry
    fs = batch_of("random_p0.2")
    comp = geometry.label_components(on_device(fs), fs[0].level, volume_size=1.5)
    refs = [cc.reference(f.density, f.level)[1] for f in fs]
    kmax = max(r.count for r in refs)
    want = padded([cc.reference_centroid(r.coord_sum, r.sizes, fs[0].shape, 1.5) for r in refs], kmax, 3, np.float64)
    assert np.array_equal(comp.centroid.cpu().numpy(), want)
    x = mc.world_axis(fs[0].shape[2], 1.5)
    assert x[0] <= want[0, :refs[0].count, 0].min() and want[0, :refs[0].count, 0].max() <= x[-1]


def test_cleaned_density_equals_the_restatement_bit_for_bit():
    from forge_amd import geometry
    removed = kept = 0
    for fs in cc.batches():
        d = on_device(fs)
        for keep, min_voxels, min_fraction in SELECTIONS:
            out = geometry.keep_components(d, fs[0].level, keep=keep, min_voxels=min_voxels, min_fraction=min_fraction)
            assert out.shape == d.shape and out.dtype == torch.float32 and out.device == d.device
            want = np.stack([cc.reference_clean(f.density, f.level, keep, min_voxels, min_fraction) for f in fs])[:, None]
            got = out.cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), ([f.name for f in fs], keep, min_voxels, min_fraction)
            src = cc.stack(fs).view(np.int32)
            removed += int((got.view(np.int32) != src).sum())
            kept += int(((got.view(np.int32) == src) & (cc.stack(fs) > np.float32(fs[0].level))).sum())
    assert removed > 0 and kept > 0
    apart = cc.fields()["twin_snakes_apart"]                                             # the tie: the lower label wins
    fs = batch_of("twin_snakes_apart")
    v = [f.name for f in fs].index("twin_snakes_apart")
    got = geometry.keep_components(on_device(fs), 0.5)[v, 0].cpu().numpy()
    w = apart.shape[2] // 2 - 1
    assert np.array_equal(got[:, :, :w], apart.density[:, :, :w]) and not got[:, :, w:].any() and apart.density[:, :, w + 2:].any()


@pytest.mark.parametrize("which", ["K", "K-1", "1", "0"])
def test_capacity_mode(which):
    from forge_amd import geometry, ops
    fs = batch_of("random_p0.05")
    assert len(fs) == 3
    d = on_device(fs)
    counts = [cc.reference(f.density, f.level)[1].count for f in fs]
    kmax = {"K": max(counts), "K-1": max(counts) - 1, "1": 1, "0": 0}[which]
    comp = geometry.label_components(d, fs[0].level, max_components=kmax)
    assert comp.counts.cpu().tolist() == counts and tuple(comp.sizes.shape) == (3, kmax)
    assert comp.status.cpu().tolist() == [ops.COMPONENTS_OVERFLOW if k > kmax else 0 for k in counts]
    assert np.array_equal(comp.labels.cpu().numpy(), np.stack([cc.reference(f.density, f.level)[0] for f in fs]))      # labels need no capacity
    _, _, ws = ops.components_label(d, fs[0].level, want_labels=False)
    sizes, bbox, coord_sum, status = ops.components_stats(d, ws, kmax)
    check_statistics(fs, kmax, sizes, bbox, coord_sum, status)
    check_statistics(fs, kmax, comp.sizes, comp.bbox, coord_sum, comp.status, comp.centroid)
    if which == "K":
        low = counts.index(min(counts))
        assert not comp.sizes[low, counts[low]:].any() and not comp.bbox[low, counts[low]:].any() and not comp.centroid[low, counts[low]:].any()


@pytest.mark.parametrize("name", ["random_p0.2", "snake16x16x16"])
def test_determinism(name):
    from forge_amd import geometry, ops
    fs = batch_of(name)
    d = on_device(fs)
    runs = []
    for _ in range(2):
        labels, counts, ws = ops.components_label(d, fs[0].level)
        stats = ops.components_stats(d, ws, 400)
        clean = geometry.keep_components(d, fs[0].level, keep="all", min_voxels=3)
        runs.append((labels, counts) + tuple(stats) + (clean.view(torch.int32),))
    for a, b in zip(*runs):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_keep_components_and_extraction_in_one_captured_graph():
    """keep_components and capacity-mode extract_mesh never synchronise: captured once on one stream (no parallel branches), replayed twice,
    both replays bitwise the eager result."""
    from forge_amd.geometry import extract_mesh, keep_components
    f = cc.fields()["blob_floaters"]
    d = on_device((f,))
    eager_clean = keep_components(d, 0.5)
    eager = extract_mesh(eager_clean, max_vertices=800, max_faces=1600)
    assert eager.counts.cpu().tolist() == [[706, 1408]] and eager.status.cpu().tolist() == [0]
    static = d.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        clean = keep_components(static, 0.5)
        batch = extract_mesh(clean, max_vertices=800, max_faces=1600)
    for _ in range(2):
        clean.zero_()
        batch.vertices.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(clean.view(torch.int32), eager_clean.view(torch.int32))
        assert torch.equal(batch.counts, eager.counts) and torch.equal(batch.faces, eager.faces)
        assert torch.equal(batch.vertices.view(torch.int32), eager.vertices.view(torch.int32))
        assert torch.equal(batch.normals.view(torch.int32), eager.normals.view(torch.int32))


def test_label_components_with_a_capacity_runs_in_a_captured_graph():
    """label_components(max_components=K) makes no host synchronisation and no host-to-device copy: captured once on one stream (no parallel
    branches), replayed twice after its outputs were overwritten, every field bitwise the eager result."""
    from forge_amd.geometry import label_components
    fs = batch_of("random_p0.05")
    d = on_device(fs)
    K = max(cc.reference(f.density, f.level)[1].count for f in fs) - 1                  # one volume overflows: the status bit is replayed too
    eager = label_components(d, fs[0].level, max_components=K, volume_size=1.5)
    assert sorted(eager.status.cpu().tolist()) == [0, 0, 1]
    static = d.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        comp = label_components(static, fs[0].level, max_components=K, volume_size=1.5)
    for _ in range(2):
        for t in comp:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(comp._fields, comp, eager):
            assert a.dtype == b.dtype and a.shape == b.shape, name
            if a.dtype == torch.float64:
                a, b = a.view(torch.int64), b.view(torch.int64)
            assert torch.equal(a, b), name


@pytest.mark.parametrize("components", ["largest", {"keep": "largest", "level": 0.2}, {"keep": "all", "min_voxels": 3}])
def test_submesh_property_on_the_device(components):
    from forge_amd.geometry import extract_mesh
    f = cc.fields()["blob_floaters"]
    d = on_device((f,))
    (full,) = extract_mesh(d)
    (sub,) = extract_mesh(d, components=components)
    assert full.vertices.shape[0] == 772 and sub.vertices.shape[0] == 706 and sub.faces.shape[0] == 1408
    vmap = cc.submesh_map(full.vertices.cpu().numpy(), sub.vertices.cpu().numpy())      # ordered, bitwise
    assert np.array_equal(cc.filtered_faces(full.faces.cpu().numpy(), vmap), sub.faces.cpu().numpy())
    kept = torch.from_numpy(vmap >= 0).cuda()
    assert torch.equal(full.normals[kept].view(torch.int32), sub.normals.view(torch.int32))       # the floaters are far from the object
    assert mc.directed_edges_paired(sub.faces.cpu().numpy())
    assert float(sub.volume()) <= float(full.volume()) and float(sub.volume()) > 0.0
    with pytest.raises(ValueError, match="above the extraction level"):
        extract_mesh(d, level=0.5, components={"level": 0.75})


def test_submesh_property_on_a_random_field_in_a_batch():
    from forge_amd.geometry import extract_mesh
    fs = batch_of("random_p0.3")
    d = on_device(fs)
    for full, sub, f in zip(extract_mesh(d, level=mc.QUANT_LEVEL), extract_mesh(d, level=mc.QUANT_LEVEL, components="largest"), fs):
        assert 0 < sub.vertices.shape[0] < full.vertices.shape[0]
        vmap = cc.submesh_map(full.vertices.cpu().numpy(), sub.vertices.cpu().numpy())
        assert np.array_equal(cc.filtered_faces(full.faces.cpu().numpy(), vmap), sub.faces.cpu().numpy()), f.name
        assert mc.directed_edges_paired(sub.faces.cpu().numpy())


def test_colored_mesh_cleans_the_volume_once_for_every_stage():
    """colored_mesh(components="largest") is the hand-composed chain on the cleaned density - extraction, the rendered views and the bake's
    transmittance all see it - and colored_mesh without the argument is the chain on the density as the heads emit it, as before."""
    import bake_cases as bc
    from forge_amd import geometry, nvs, synthetic as syn
    from forge_amd.volume_render import VolRender
    dev = torch.device("cuda")
    cfg = syn.kubric_config(img_size=64, n_pts_per_ray=48)
    vr = VolRender(cfg)
    sd = syn.seeded_state_dict({"render." + k: v for k, v in vr.state_dict().items()}, 3)
    vr.load_state_dict({k[len("render."):]: v for k, v in sd.items()})
    vr = vr.to(dev).eval()
    feat, dens = (t.to(dev) for t in syn.blob_volumes(2, 16, 16, seed=31))
    dens = dens.clone()
    dens[0, 0, 1, 1, 1] = dens[0, 0, 14, 13, 2] = dens[0, 0, 14, 14, 3] = dens[1, 0, 2, 13, 13] = 1.0        # floaters

    class Heads:
        @staticmethod
        def heads(fused):
            return feat, dens

    class Model:
        render, encoder_3d = vr, Heads
    K = syn.intrinsics(64)
    n_views = 8
    fused = torch.zeros(2, 128, 8, 8, 8, device=dev)

    def by_hand(density):
        plain = geometry.extract_mesh(density)
        imgs, _ = nvs.render_360(Model, feat, density, K, 1.5, n_views=n_views)
        R, T = nvs.nvs_cameras(1.5, n_views, dev)
        cams = {"R": R.repeat(2, 1, 1), "T": T.repeat(2, 1), "K": K.to(dev)[None].repeat(2 * n_views, 1, 1)}
        v2v = torch.arange(2).repeat_interleave(n_views).to(dev, torch.int32)
        gain = torch.full((2 * n_views,), 0.05, device=dev)
        return geometry.bake_vertex_colors(plain, density, imgs.reshape(2 * n_views, 3, 64, 64), cams, v2v, view_gain=gain)[0]

    clean = geometry.keep_components(dens, 0.5)
    assert int((clean != dens).sum()) == 4
    for components, density in ((None, dens), ("largest", clean)):
        kw = {} if components is None else {"components": components}
        meshes, _ = geometry.colored_mesh(Model, fused, K, 1.5, n_views=n_views, render_gain=0.05, **kw)
        for m, wm in zip(meshes, by_hand(density)):
            assert m.vertices.shape[0] > 500 and torch.equal(m.vertices, wm.vertices) and torch.equal(m.faces, wm.faces)
            assert torch.equal(m.colors.view(torch.int32), wm.colors.view(torch.int32))
    plain, cleaned = geometry.extract_mesh(dens), geometry.extract_mesh(clean)
    assert all(c.vertices.shape[0] < p.vertices.shape[0] for p, c in zip(plain, cleaned))
