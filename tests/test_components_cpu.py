"""Connected components without a GPU: the numpy restatement of include/forge_hip.h section g4 (tests/components_cases.py) against the known
answers, against scipy.ndimage.label under the 15-point structure, and against the mesh case table it claims to share its edges with; the
sub-mesh property the Kuhn adjacency exists for, on the restated mesh extraction; and the argument checks of the library and of the Python
surface, all of which answer before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import components_cases as cc
import mesh_cases as mc
from forge_amd import _lib, geometry, ops


def test_known_answers():
    F = cc.fields()
    seen = 0
    for f in F.values():
        labels, st = cc.reference(f.density, f.level)
        assert labels.dtype == np.int32 and labels.shape == f.shape
        if f.K is not None:
            assert st.count == f.K, (f.name, st.count)
            seen += 1
        if f.sizes is not None:
            assert st.sizes.tolist() == list(f.sizes), (f.name, st.sizes.tolist())
    assert seen >= 13 + 49 + 10
    assert sum(F[n].K == 1 for n in F if n.startswith("two_voxels")) == 7 and sum(F[n].K == 2 for n in F if n.startswith("two_voxels")) == 6
    for p, (K, first, second) in cc.RANDOM_KNOWN.items():
        st = cc.reference(F["random_p%g" % p].density, mc.QUANT_LEVEL)[1]
        assert (st.count,) + tuple(np.sort(st.sizes)[::-1][:2].tolist()) == (K, first, second), p
    st = cc.reference(F["all_inside"].density, 0.5)[1]
    assert st.sizes.tolist() == [33 * 9 * 8] and st.bbox.tolist() == [[0, 0, 0, 7, 8, 32]]
    assert st.coord_sum.tolist() == [[33 * 9 * (8 * 7 // 2), 33 * 8 * (9 * 8 // 2), 9 * 8 * (33 * 32 // 2)]]
    assert np.array_equal(cc.reference_centroid(st.coord_sum, st.sizes, (33, 9, 8)), np.zeros((1, 3)))
    for name in ("snake16x16x16", "snake9x7x17", "twin_snakes_bridged"):
        assert cc.reference(F[name].density, 0.5)[1].count == 1
    s = cc.reference(F["twin_snakes_apart"].density, 0.5)[1].sizes
    assert len(s) == 2 and s[0] == s[1]
    assert cc.kept_components(s, "largest") == [0]                                      # the tie goes to the lower label


def test_labels_are_numbered_by_lowest_index_and_statistics_add_up():
    for name in ("random_p0.2", "blob_floaters", "extent9x7x17"):
        f = cc.fields()[name]
        labels, st = cc.reference(f.density, f.level)
        flat = labels.ravel()
        first = [int(np.flatnonzero(flat == k + 1)[0]) for k in range(st.count)]
        assert first == sorted(first)
        assert np.array_equal(labels > 0, f.density > np.float32(f.level)) and int(st.sizes.sum()) == int((labels > 0).sum())
        z, y, x = np.nonzero(labels == 1)
        assert st.bbox[0].tolist() == [x.min(), y.min(), z.min(), x.max(), y.max(), z.max()] and st.coord_sum[0].tolist() == [x.sum(), y.sum(), z.sum()]
        D, H, W = f.shape
        want = [mc.world_axis(W)[x].mean(), mc.world_axis(H)[y].mean(), mc.world_axis(D)[z].mean()]
        np.testing.assert_allclose(cc.reference_centroid(st.coord_sum, st.sizes, f.shape)[0], want, rtol=0, atol=1e-12)


def test_selection_rule():
    sizes = np.array([3, 727, 10, 727, 8, 1], np.int32)
    assert cc.kept_components(sizes, "largest") == [1]
    assert cc.kept_components(sizes, "all") == [0, 1, 2, 3, 4, 5]
    assert cc.kept_components(sizes, "all", min_voxels=10) == [1, 2, 3]
    assert cc.kept_components(sizes, "all", min_fraction=0.01) == [1, 2, 3, 4]            # ceil(7.27) = 8
    assert cc.kept_components(sizes, "all", min_fraction=1.0) == [1, 3]
    assert cc.kept_components(sizes, "largest", min_voxels=728) == [] and cc.kept_components(np.zeros(0, np.int32)) == []
    f = cc.fields()["specials"]
    out = cc.reference_clean(f.density, f.level, "largest")
    want = f.density.view(np.uint32).copy()
    want[0, 0, 0] = want[0, 0, 2] = 0                                                    # the two single voxels go, +0.0; NaNs and -0.0 keep their bits
    assert np.array_equal(out.view(np.uint32), want)
    e = cc.fields()["all_outside"]
    assert np.array_equal(cc.reference_clean(e.density, e.level), e.density)


def test_against_scipy_with_the_15_point_structure():
    ndi = pytest.importorskip("scipy.ndimage")
    S = np.zeros((3, 3, 3), int)
    S[1, 1, 1] = 1
    for dx, dy, dz in cc.DIRECTIONS:
        S[1 + dz, 1 + dy, 1 + dx] = S[1 - dz, 1 - dy, 1 - dx] = 1
    assert S.sum() == 15
    for f in cc.fields().values():
        labels, st = cc.reference(f.density, f.level)
        sl, K = ndi.label(f.density > np.float32(f.level), structure=S)
        assert K == st.count, f.name
        flat = sl.ravel()
        order, renum = {}, np.zeros(flat.shape, np.int32)
        for i in np.flatnonzero(flat):                                                   # renumber by first occurrence in linear order
            renum[i] = order.setdefault(int(flat[i]), len(order) + 1)
        assert np.array_equal(renum.reshape(f.shape), labels), f.name


def test_directions_are_the_edges_of_the_mesh_case_table():
    """The adjacency is the edge set of the six Kuhn tetrahedra of csrc/mesh.hip: corner code differences within a tetrahedron, exactly 1..7.
    A guard, not a test of new library code: it pins the RESTATEMENT's directions to the mesh table and fails if that table ever changes; the
    kernels' own decoding of codes 1..7 is pinned by the exact comparisons of tests/test_gpu_components.py."""
    tab = ops.mesh_case_table()
    codes = set()
    for q in range(6):
        corner = tab["tet_corner"][q]
        for i, j in tab["tet_edge"]:
            a, b = corner[i], corner[j]
            assert a & b == a and b != a                                                 # nested corner codes: the edge runs in a positive direction
            codes.add(b ^ a)
    assert codes == set(range(1, 8))
    assert sorted(cc.DIRECTIONS) == sorted((c & 1, (c >> 1) & 1, c >> 2) for c in codes)


def _submesh(density, label_level, level):
    full = mc.reference_mesh(density, level)
    clean = cc.reference_clean(density, label_level, "largest")
    sub = mc.reference_mesh(clean, level)
    assert 0 < len(sub.vertices) < len(full.vertices)
    vmap = cc.submesh_map(full.vertices.astype(np.float32), sub.vertices.astype(np.float32))
    assert np.array_equal(full.vertices[vmap >= 0], sub.vertices)                        # float64 rows: bit for bit
    assert np.array_equal(cc.filtered_faces(full.faces, vmap), sub.faces)
    assert mc.directed_edges_paired(sub.faces)
    return full, sub, vmap


@pytest.mark.parametrize("label_level", [0.5, 0.2])
def test_submesh_property_blob_and_floaters(label_level):
    f = cc.fields()["blob_floaters"]
    full, sub, vmap = _submesh(f.density, label_level, 0.5)
    assert len(sub.vertices) == 706 and len(full.vertices) == 772                        # the blob alone; with its four floaters
    assert np.array_equal(full.normals[vmap >= 0], sub.normals)                          # the floaters are far from the object


@pytest.mark.parametrize("label_level", [mc.QUANT_LEVEL, 31.0 / 128.0])      # the lower one lets the samples at 16/64 in
def test_submesh_property_random_field(label_level):
    _submesh(cc.fields()["extent7x8x9"].density, label_level, mc.QUANT_LEVEL)


def test_library_checks_arguments_before_any_launch(built_lib):
    L = _lib.lib()
    fake = 0x1000                                                                        # never dereferenced
    T = L.forge_components_tile()
    assert T >= 2 and T == ops.components_tile()
    nbytes = L.forge_components_workspace_bytes(2, 8, 8, 8)
    assert nbytes >= 2 * 512 * 12 and nbytes % 16 == 0
    assert L.forge_components_workspace_bytes(0, 8, 8, 8) == -1 and L.forge_components_workspace_bytes(1, 8, 0, 8) == -1
    assert L.forge_components_workspace_bytes(1, 8, 8, -3) == -1
    assert L.forge_components_workspace_bytes(1, 2048, 1024, 1024) == -2                 # D H W = 2^31
    assert L.forge_components_workspace_bytes(1, 1, 1, 2 ** 31 - 1) == -2                # D H W = 2^31 - 1
    assert L.forge_components_workspace_bytes(1, 1, 1, 2 ** 31 - 2) > 0
    label = lambda d=fake, n=2, D=8, H=8, W=8, level=0.5, ws=fake, b=nbytes, counts=fake: L.forge_components_label(d, n, D, H, W, level, ws, b, None, counts, None)
    assert label(d=None) == -1 and b"null pointer" in L.forge_last_error()
    assert label(ws=None) == -1 and label(counts=None) == -1
    for level in (0.0, -1.0, float("inf"), float("nan")):
        assert label(level=level) == -1
    assert b"level" in L.forge_last_error()
    assert label(n=0) == -1 and label(D=0) == -1 and label(W=-1) == -1
    assert label(D=2048, H=1024, W=1024, b=1 << 62) == -2
    assert label(b=nbytes - 1) == -1 and b"workspace" in L.forge_last_error()
    assert label(ws=fake + 4) == -1
    stats = lambda ws=fake, b=nbytes, k=4, sizes=fake, status=fake, D=8: L.forge_components_stats(ws, b, 2, D, 8, 8, k, sizes, fake, fake, status, None)
    assert stats(ws=None) == -1 and stats(status=None) == -1 and stats(sizes=None) == -1 and stats(k=-1) == -1
    assert stats(b=nbytes - 1) == -1 and stats(D=0) == -1
    select = lambda d=fake, ws=fake, b=nbytes, kl=1, mv=1, mf=0.0, out=fake: L.forge_components_select(d, 2, 8, 8, 8, ws, b, kl, mv, ctypes.c_double(mf), out, None)
    assert select(d=None) == -1 and select(ws=None) == -1 and select(out=None) == -1
    assert select(kl=2) == -1 and select(mv=0) == -1 and select(mf=-0.1) == -1 and select(mf=1.5) == -1 and select(mf=float("nan")) == -1
    assert select(b=nbytes - 1) == -1


def test_python_surface_refuses_bad_tensors():
    d = torch.zeros(1, 1, 4, 4, 4)
    for call in (lambda: ops.components_label(d), lambda: geometry.label_components(d), lambda: geometry.keep_components(d),
                 lambda: geometry.extract_mesh(d, components="largest")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    fake = torch.zeros                                                                   # host tensors: shape, dtype and layout are checked before the device
    with pytest.raises(TypeError):
        ops.components_label(fake(1, 1, 4, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.components_label(fake(1, 4, 4, 4))
    with pytest.raises(ValueError):
        ops.components_label(fake(1, 2, 4, 4, 4))
    with pytest.raises(ValueError):
        ops.components_label(fake(1, 1, 4, 4, 8)[..., ::2])
    with pytest.raises(ValueError):
        ops.components_label(fake(1, 1, 4, 4, 4), level=0.0)
    with pytest.raises(ValueError):
        ops.components_select(fake(1, 1, 4, 4, 4), fake(8, dtype=torch.uint8), min_voxels=0)
    with pytest.raises(ValueError):
        ops.components_select(fake(1, 1, 4, 4, 4), fake(8, dtype=torch.uint8), min_fraction=1.5)
    with pytest.raises(ValueError):
        ops.components_select(fake(1, 1, 4, 4, 4), fake(8, dtype=torch.uint8))           # a workspace too small for the shape
    with pytest.raises(ValueError):
        ops.components_stats(fake(1, 1, 4, 4, 4), fake(1 << 20, dtype=torch.uint8), -1)
    with pytest.raises(TypeError):
        ops.components_stats(fake(1, 1, 4, 4, 4), None, 4)
    with pytest.raises(ValueError):
        geometry.keep_components(fake(1, 1, 4, 4, 4), keep="biggest")


def test_extract_mesh_refuses_a_label_level_above_the_extraction_level():
    d = torch.zeros(1, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="above the extraction level"):
        geometry.extract_mesh(d, level=0.5, components={"level": 0.6})
    with pytest.raises(TypeError):
        geometry.extract_mesh(d, components=3)
    assert ops.COMPONENTS_OVERFLOW == 1
