"""Surface metrics without a GPU: the float64 restatement of include/forge_hip.h section g3 (tests/geom_cases.py) against analytic known
answers, the properties of the systematic surface sampling, the argument checks of the three C entry points and the PLY / OBJ readers."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import geom_cases as gc
import mesh_cases as mc
from forge_amd import _lib


# ------------------------------------------------------------------------------------------------------------- restatement: known answers
def test_concentric_spheres():
    """B = (r2 / r1) A on concentric spheres: the nearest point of a_i is its own copy, every distance is |r1 - r2| (up to the fp32 rounding of
    the coordinates, <= 2 u r per coordinate)."""
    r1, r2 = 0.5, 0.45
    a, nrm = gc.sphere_points(400, r1, seed=1)
    b = (a.astype(np.float64) * (r2 / r1)).astype(np.float32)
    gap = abs(r1 - r2)
    out, status, ab, ba = gc.point_metrics(a, b, nrm, nrm, thresholds=(gap * 1.001, gap * 0.999))
    assert status == 0
    assert np.array_equal(ab["idx"], np.arange(400)) and np.array_equal(ba["idx"], np.arange(400))
    tol = 8 * gc.U
    assert out[gc.OUT["accuracy"]] == pytest.approx(gap, abs=tol) and out[gc.OUT["completeness"]] == pytest.approx(gap, abs=tol)
    assert out[gc.OUT["chamfer_l1"]] == pytest.approx(gap, abs=tol) and out[gc.OUT["hausdorff"]] == pytest.approx(gap, abs=tol)
    assert out[gc.OUT["chamfer_l2"]] == pytest.approx(2 * gap * gap, abs=4 * gap * tol)
    assert out[gc.OUT["precision"]] == 1.0 and out[gc.OUT["recall"]] == 1.0 and out[gc.OUT["fscore"]] == 1.0            # tau just above the gap
    assert out[gc.OUT["precision"] + 1] == 0.0 and out[gc.OUT["recall"] + 1] == 0.0 and out[gc.OUT["fscore"] + 1] == 0.0  # just below: P + R = 0 -> 0
    assert out[gc.OUT["normal_consistency"]] == pytest.approx(1.0, abs=4 * gc.U)
    assert np.isnan(out[gc.OUT["fscore"] + 2]) and np.isnan(out[gc.OUT["fscore"] + 3])                                   # thresholds that were not given


def test_identical_sets():
    a, nrm = gc.sphere_points(300, 0.4, seed=2)
    out, status, ab, ba = gc.point_metrics(a, a.copy(), nrm, nrm, thresholds=(0.01,))
    assert status == 0
    assert np.array_equal(ab["idx"], np.arange(300)) and np.array_equal(ba["idx"], np.arange(300))
    for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff"):
        assert out[gc.OUT[k]] == 0.0
    assert out[gc.OUT["fscore"]] == 1.0 and out[gc.OUT["precision"]] == 1.0 and out[gc.OUT["recall"]] == 1.0
    assert out[gc.OUT["normal_consistency"]] == pytest.approx(1.0, abs=4 * gc.U)


def test_ties_counts_and_empty_sides():
    a = gc.uniform_points((20, 3), 3)
    dup = np.concatenate([a, a])                                         # every reference again at a higher index
    r = gc.nn(a, dup)
    assert np.array_equal(r["idx"], np.arange(20)) and (r["d2"] == 0).all()
    r = gc.nn(a, dup, nq=5, np_=0)
    assert np.isinf(r["d2"][:5]).all() and (r["d2"][5:] == 0).all() and (r["idx"] == -1).all()
    out, status, _, _ = gc.point_metrics(a, a, na=0, thresholds=(0.1,))
    assert status == gc.EMPTY and np.isnan(out[gc.OUT["accuracy"]]) and np.isnan(out[gc.OUT["chamfer_l1"]]) and np.isnan(out[gc.OUT["hausdorff"]])


def test_transform_is_applied_to_the_queries():
    a = gc.uniform_points((50, 3), 4)
    shift = np.array([1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, -0.125], np.float32)
    b = (a.astype(np.float64) + [0.25, 0, -0.125]).astype(np.float32)
    out, status, ab, _ = gc.point_metrics(a, b, thresholds=(1e-6,), xf=shift)
    assert np.array_equal(ab["idx"], np.arange(50)) and out[gc.OUT["chamfer_l1"]] <= 2 * gc.U and out[gc.OUT["fscore"]] == 1.0


# ------------------------------------------------------------------------------------------------------------- restatement: sampling
def _blob_mesh():
    m = mc.reference_mesh(mc.blob(8), 0.5)
    return m.vertices.astype(np.float32), m.faces


@pytest.mark.parametrize("name,n", [("octahedron", 7), ("octahedron", 1000), ("octahedron_bad_faces", 333), ("blob8", 64), ("blob8", 5000)])
def test_systematic_sampling_properties(built_lib, name, n):
    if name == "blob8":
        v, f = _blob_mesh()
        bad = []
    elif name == "octahedron":
        v, f = gc.octahedron()
        bad = []
    else:
        v, f, bad = gc.with_bad_faces(*gc.octahedron())
    s = gc.sample_surface(v, f, n)
    assert s["status"] == 0 and (s["areas"][bad] == 0).all()
    dev = gc.check_systematic(s["face"], s["areas"], n)
    print("%s n=%d: max |k_f - n A_f / A| = %.3f" % (name, n, dev))
    assert not np.isin(s["face"], bad).any()
    r1, r2 = s["r1"].astype(np.float64), s["r2"].astype(np.float64)
    assert (r1 >= 0).all() and (r2 >= 0).all() and (r1 + r2 <= 1).all()          # inside the triangle, exactly
    assert (np.round(r1 * 2 ** 24) == r1 * 2 ** 24).all()                          # 24-bit fractions: exact in fp32
    # the points lie in their faces' planes
    fs = f[s["face"]]
    a = v[fs[:, 0]].astype(np.float64)
    assert np.abs(((s["points"] - a) * s["normals"]).sum(axis=1)).max() <= 1e-12


def test_sampling_an_empty_mesh():
    v, f = gc.octahedron()
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 0, 1], [2, 2, 2]], np.int32)):
        s = gc.sample_surface(v, faces, 16)
        assert s["status"] == gc.EMPTY and (s["face"] == -1).all() and (s["points"] == 0).all() and (s["normals"] == 0).all()


def test_barycentrics_are_the_r2_sequence():
    """1 / g and 1 / g^2 of the plastic number g = 1.3247..., as 32-bit fractions."""
    g = 1.32471795724474602596
    assert round(2 ** 32 / g) == 3242174889 and round(2 ** 32 / g ** 2) == 2447445414
    r1, r2 = gc.barycentrics(4)
    assert r1[0] == 0 and r2[0] == 0
    k1, k2 = 3242174889 >> 8, 2447445414 >> 8                                      # sample 1: k1 + k2 > 2^24, folded
    assert k1 + k2 > 2 ** 24 and r1[1] == np.float32((2 ** 24 - k1) * 2.0 ** -24) and r2[1] == np.float32((2 ** 24 - k2) * 2.0 ** -24)


# ----------------------------------------------------------------------------------------------------------------- argument checks
def test_c_abi_argument_errors_without_a_device(built_lib):
    L = _lib.lib()
    fake = 0x1000                                                # never dereferenced: every check runs before the first HIP call
    assert L.forge_nn_queries_per_block() >= 64 and L.forge_nn_tile_points() >= 4 and L.forge_geom_scan_threads() == gc.SCAN_THREADS
    assert L.forge_surface_sample_workspace_bytes(2, 100, 0) >= 2 * 100 * 8 and L.forge_surface_sample_workspace_bytes(2, 100, 1) >= 100 * 8
    assert L.forge_surface_sample_workspace_bytes(0, 100, 0) == -1 and L.forge_surface_sample_workspace_bytes(1, -1, 0) == -1
    assert L.forge_surface_sample_workspace_bytes(65535, 1 << 20, 0) == -2
    ws = 1 << 30

    def sample(vertices=fake, faces=fake, counts=fake, offsets=None, n=1, mv=8, mf=8, ns=16, workspace=fake, nbytes=ws, points=fake, normals=fake,
               face=fake, bary=fake, status=fake):
        return L.forge_surface_sample(vertices, faces, counts, offsets, n, mv, mf, ns, workspace, nbytes, points, normals, face, bary, status, None)

    for name in ("vertices", "faces", "counts", "workspace", "points", "normals", "face", "bary", "status"):
        assert sample(**{name: None}) == -1, name
    assert b"null pointer" in L.forge_last_error()
    assert sample(n=0) == -1 and sample(ns=0) == -1 and sample(mv=-1) == -1 and sample(mf=-1) == -1
    assert sample(nbytes=8 * 8 - 1) == -1 and sample(workspace=fake + 8) == -1
    assert b"workspace" in L.forge_last_error()
    assert sample(n=65536) == -2 and sample(n=4, ns=1 << 30) == -2

    def nn(q=fake, p=fake, qc=None, pc=None, xf=None, B=1, Nq=4, Np=4, d2=fake, idx=fake, qxf=None):
        return L.forge_nn_points(q, p, qc, pc, xf, B, Nq, Np, d2, idx, qxf, None)

    assert nn(q=None) == -1 and nn(p=None) == -1 and nn(d2=None) == -1 and nn(idx=None) == -1
    assert b"null pointer" in L.forge_last_error()
    assert nn(B=0) == -1 and nn(Nq=0) == -1 and nn(Np=0) == -1 and nn(B=-3) == -1
    assert nn(B=65536) == -2 and nn(Nq=0x7fffffff) == -2 and nn(Np=0x7fffffff) == -2

    assert L.forge_geom_metrics_partial_doubles(0) == -1 and L.forge_geom_metrics_partial_doubles(3) > 0
    good = (ctypes.c_double * 4)(0.01, 0.02, 0.05, 0.1)

    def met(d2ab=fake, iab=fake, d2ba=fake, iba=fake, na=None, nb=None, ca=None, cb=None, B=1, Na=4, Nb=4, tau=good, nt=3, partial=fake, out=fake,
            status=fake):
        return L.forge_geom_metrics(d2ab, iab, d2ba, iba, na, nb, ca, cb, B, Na, Nb, tau, nt, partial, out, status, None)

    for name in ("d2ab", "iab", "d2ba", "iba", "partial", "out", "status"):
        assert met(**{name: None}) == -1, name
    assert met(B=0) == -1 and met(Na=0) == -1 and met(Nb=0) == -1
    assert met(nt=5) == -1 and met(nt=-1) == -1 and met(tau=None, nt=1) == -1
    assert b"threshold" in L.forge_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert met(tau=(ctypes.c_double * 4)(0.01, bad, 0.05, 0.1)) == -1
    assert b"not finite" in L.forge_last_error()
    assert met(na=fake) == -1 and met(nb=fake) == -1                    # the normals of one side only
    assert met(partial=fake + 4) == -1 and met(out=fake + 4) == -1      # unaligned
    assert met(B=65536) == -2


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from forge_amd import geometry, ops
    pts = torch.zeros(1, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nn_points(pts, pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.point_metrics(pts, pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.surface_sample(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.geom_metrics(torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="both sides"):
        geometry.point_metrics(pts, pts, normals_a=pts)
    assert ops.GEOM_EMPTY == 1 and ops.GEOM_OUT_DOUBLES == gc.OUT_DOUBLES
    assert dict(ops.GEOM_PER_THRESHOLD) == {k: gc.OUT[k] for k in ("precision", "recall", "fscore")}
    assert list(ops.GEOM_SCALARS) == [k for k in gc.OUT if gc.OUT[k] < 6]
    import forge_amd
    from forge_amd import evaluation
    assert callable(forge_amd.mesh_metrics) and callable(forge_amd.point_metrics) and callable(forge_amd.sample_surface)
    assert callable(evaluation.evaluate_geometry)


# ---------------------------------------------------------------------------------------------------------------------------- readers
def _coloured_mesh(built_lib):
    from forge_amd.geometry import Mesh
    m = mc.reference_mesh(mc.blob(8), 0.5)
    v = torch.from_numpy(m.vertices.astype(np.float32))
    colours = torch.from_numpy(np.random.default_rng(5).random((len(v), 3)).astype(np.float32))
    return Mesh(v, torch.from_numpy(m.normals.astype(np.float32)), torch.from_numpy(m.faces), None, colours)


def test_ply_round_trip(built_lib, tmp_path):
    from forge_amd.geometry import Mesh
    mesh = _coloured_mesh(built_lib)
    path = str(tmp_path / "m.ply")
    mesh.to_ply(path)
    back = Mesh.from_ply(path)
    assert back.vertices.dtype == torch.float32 and back.faces.dtype == torch.int32
    assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.faces, mesh.faces) and torch.equal(back.normals, mesh.normals)
    assert (back.colors - mesh.colors).abs().max() <= 0.5 / 255 + 1e-7              # round-to-nearest bytes: half a step, within the 1 / 255 allowed
    plain = Mesh(mesh.vertices, mesh.normals, mesh.faces)
    plain.to_ply(path)
    back = Mesh.from_ply(path)
    assert back.colors is None and torch.equal(back.vertices, mesh.vertices) and torch.equal(back.faces, mesh.faces)


def test_obj_round_trip(built_lib, tmp_path):
    from forge_amd.geometry import Mesh
    mesh = _coloured_mesh(built_lib)
    path = str(tmp_path / "m.obj")
    mesh.to_obj(path)
    back = Mesh.from_obj(path)
    assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.faces, mesh.faces)        # %.9g round-trips float32
    assert torch.equal(back.normals, mesh.normals) and torch.equal(back.colors, mesh.colors.clamp(0, 1))


ASCII_PLY = """ply
format ascii 1.0
comment a quad and a triangle, double coordinates, int64-free list types
element vertex 5
property double x
property double y
property double z
property uchar red
property uchar green
property uchar blue
element face 2
property list uchar uint vertex_index
end_header
0 0 0 255 0 0
1 0 0 0 255 0
1 1 0 0 0 255
0 1 0 255 255 255
0.5 0.5 1 0 0 0
4 0 1 2 3
3 0 1 4
"""


def test_hand_written_ascii_ply(tmp_path):
    from forge_amd.geometry import Mesh
    path = tmp_path / "quad.ply"
    path.write_text(ASCII_PLY)
    m = Mesh.from_ply(str(path))
    assert m.vertices.shape == (5, 3) and m.vertices.dtype == torch.float32 and m.vertices[4].tolist() == [0.5, 0.5, 1.0]
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]                   # the quad as a fan
    assert m.colors[1].tolist() == [0.0, 1.0, 0.0]
    n = m.normals                                                                  # missing: area-weighted vertex normals
    assert torch.allclose(n.norm(dim=1), torch.ones(5), atol=1e-6)
    assert torch.allclose(n[3], torch.tensor([0.0, 0.0, 1.0]))                     # vertex 3 touches the quad's second triangle only
    assert n[0, 2] > 0 and n[0, 1] < 0                                             # vertex 0: the quad (+z) and the tilted triangle (-y, +z)


def test_binary_ply_with_mixed_polygons_and_extra_elements(tmp_path):
    """A binary file no fast path fits: short indices, a triangle and a quad, an extra scalar property on the face, an element to skip."""
    from forge_amd.geometry import Mesh
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty float quality\n"
            "element face 2\nproperty list uchar short vertex_indices\nproperty uchar flags\nelement edge 1\nproperty int vertex1\nproperty int vertex2\n"
            "end_header\n")
    body = b"".join(struct.pack("<4f", *p) for p in [(0, 0, 0, 9), (1, 0, 0, 9), (1, 1, 0, 9), (0, 1, 0, 9)])
    body += struct.pack("<B3hB", 3, 0, 1, 2, 7) + struct.pack("<B4hB", 4, 0, 1, 2, 3, 7) + struct.pack("<2i", 0, 1)
    path = tmp_path / "mixed.ply"
    path.write_bytes(head.encode("ascii") + body)
    m = Mesh.from_ply(str(path))
    assert m.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3]] and m.vertices[2].tolist() == [1.0, 1.0, 0.0] and m.colors is None


OBJ = """# every index form, negative indices, a pentagon
mtllib scene.mtl
o thing
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v -0.5 0.5 0
vt 0 0
vt 1 0
vt 1 1
vn 0 0 1
vn 0 0 -1
s off
f 1/1/1 2/2/1 3/3/1
f 1//1 3//1 4//1
f -5 -4 -3 -2 -1
f 1/1 2/2 3/3
"""


def test_hand_written_obj(tmp_path):
    from forge_amd.geometry import Mesh
    path = tmp_path / "forms.obj"
    path.write_text(OBJ)
    m = Mesh.from_obj(str(path))
    assert m.vertices.shape == (5, 3) and m.vertices[4].tolist() == [-0.5, 0.5, 0.0]
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 2]]          # the pentagon as a fan of three
    assert torch.allclose(m.normals, torch.tensor([[0.0, 0.0, 1.0]]).expand(5, 3))   # some corners name no normal: area-weighted normals, all +z
    only_n = tmp_path / "normals.obj"
    only_n.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 -1\nf 1//1 2//1 3//-1\n")
    assert Mesh.from_obj(str(only_n)).normals.tolist() == [[0.0, 0.0, -1.0]] * 3    # every corner names one: taken as written, not recomputed


@pytest.mark.parametrize("text,line", [
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4),                       # a vertex that does not exist
    ("v 0 0 0\nv 1 0\n", 2),                                          # two coordinates
    ("v 0 0 0\ncurv 1 2\n", 2),                                       # a keyword that is not understood
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/2/3/4 2 3\n", 4),                # too many slashes
    ("v 0 0 0\nv 1 0 0\nf 1 2\n", 3),                                 # a face of two corners
])
def test_malformed_obj_names_the_line(tmp_path, text, line):
    from forge_amd.geometry import Mesh
    path = tmp_path / "bad.obj"
    path.write_text(text)
    with pytest.raises(ValueError, match="line %d" % line):
        Mesh.from_obj(str(path))


@pytest.mark.parametrize("mutate,match", [
    (lambda s: s.replace("format ascii 1.0", "format binary_big_endian 1.0"), "line 2"),
    (lambda s: s.replace("property double y", "property quad y"), "line 6"),
    (lambda s: s.replace("1 1 0 0 0 255\n", "1 1 0 0 0\n"), "line 16"),
    (lambda s: s.replace("4 0 1 2 3\n", "4 0 1 2\n"), "line 19"),
    (lambda s: s.replace("3 0 1 4\n", "3 0 1 5\n"), "vertex 5"),
    (lambda s: s.replace("end_header\n", ""), "end_header"),
])
def test_malformed_ply_is_refused(tmp_path, mutate, match):
    from forge_amd.geometry import Mesh
    path = tmp_path / "bad.ply"
    path.write_text(mutate(ASCII_PLY))
    with pytest.raises(ValueError, match=match):
        Mesh.from_ply(str(path))


def test_truncated_binary_ply_is_refused(built_lib, tmp_path):
    from forge_amd.geometry import Mesh
    mesh = _coloured_mesh(built_lib)
    path = tmp_path / "cut.ply"
    mesh.to_ply(str(path))
    raw = path.read_bytes()
    path.write_bytes(raw[:len(raw) - 20])
    with pytest.raises(ValueError, match="truncated"):
        Mesh.from_ply(str(path))
