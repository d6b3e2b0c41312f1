"""Mesh extraction without a GPU: the case table of csrc/mesh.hip, the properties of the contract's numpy restatement (tests/mesh_cases.py),
the argument checks of the C entry points and the mesh writers."""
import ctypes
import itertools
import math
import struct

import numpy as np
import pytest
import torch

import mesh_cases as mc
from forge_amd import _lib


@pytest.fixture(scope="module")
def tab(built_lib):
    return mc.table()


_REF = {}


def ref(name, D):
    """Restatement results, computed once per module run and never modified."""
    if (name, D) not in _REF:
        field = {"blob": mc.blob, "torus": mc.torus, "ones": mc.ones}[name](D)
        _REF[(name, D)] = mc.reference_mesh(field, 0.5)
    return _REF[(name, D)]


# ------------------------------------------------------------------------------------------------------------------------- case table
def test_table_layout(tab):
    assert [len(tab[k]) for k in ("tet_corner", "tet_flip", "tet_edge", "case_ntri", "case_tri")] == [6, 6, 6, 16, 16]
    paths = []
    for perm in itertools.permutations(range(3)):               # the Kuhn paths in lexicographic order of the axis permutation
        a, b, _ = perm
        paths.append([0, 1 << a, (1 << a) | (1 << b), 7])
    assert tab["tet_corner"] == paths
    for q, corner in enumerate(tab["tet_corner"]):              # tet_flip = the path's orientation
        m = np.array([[(c >> k) & 1 for k in range(3)] for c in corner[1:]], float)
        assert round(np.linalg.det(m)) == (-1 if tab["tet_flip"][q] else 1)
    assert tab["tet_edge"] == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]


def test_table_counts_by_inside_corners(tab):
    assert tab["case_ntri"][0] == 0 and tab["case_ntri"][15] == 0
    for case in range(16):
        assert tab["case_ntri"][case] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bin(case).count("1")]


def test_table_triangle_edges_join_inside_and_outside(tab):
    for case in range(16):
        for tr in range(tab["case_ntri"][case]):
            tri = tab["case_tri"][case][tr]
            assert len(set(tri)) == 3
            for e in tri:
                i, j = tab["tet_edge"][e]
                assert ((case >> i) & 1) != ((case >> j) & 1)


def _cyclic(tri):
    k = tri.index(min(tri))
    return tuple(tri[k:] + tri[:k])


def test_table_complement_reverses_winding(tab):
    for case in range(1, 15):
        mine = {_cyclic(list(tab["case_tri"][case][t])) for t in range(tab["case_ntri"][case])}
        other = {_cyclic(list(reversed(tab["case_tri"][15 - case][t]))) for t in range(tab["case_ntri"][15 - case])}
        assert mine == other, case


def test_table_winding_faces_the_outside(tab):
    """On the positively oriented tetrahedron the table is written for, every triangle's normal points from the inside to the outside corners."""
    V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], float)
    for case in range(1, 15):
        ins = [i for i in range(4) if (case >> i) & 1]
        outs = [i for i in range(4) if not (case >> i) & 1]
        for tr in range(tab["case_ntri"][case]):
            p = [V[tab["tet_edge"][e]].mean(axis=0) for e in tab["case_tri"][case][tr]]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            assert n @ (V[outs].mean(axis=0) - V[ins].mean(axis=0)) > 0


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("D", [8, 16])
@pytest.mark.parametrize("name,chi", [("blob", 2), ("torus", 0)])
def test_restatement_is_closed_and_oriented(tab, name, chi, D):
    m = ref(name, D)
    assert len(m.vertices) > 0
    assert mc.directed_edges_paired(m.faces)
    assert mc.euler_characteristic(len(m.vertices), m.faces) == chi
    assert mc.signed_volume(m.vertices, m.faces) > 0
    assert np.array_equal(np.unique(m.faces), np.arange(len(m.vertices)))          # every vertex is used


def test_restatement_random_fields_are_closed(tab):
    for field in (mc.quantised((8, 8, 8), 3), mc.noncubic()):
        m = mc.reference_mesh(field, mc.QUANT_LEVEL)
        assert mc.directed_edges_paired(m.faces)
        assert mc.signed_volume(m.vertices, m.faces) > 0


def test_restatement_all_ones_volume(tab):
    """The zero shell closes the all-ones volume half a cell outside its border samples: 61.25 cell volumes at D = 4."""
    m = ref("ones", 4)
    assert mc.directed_edges_paired(m.faces) and mc.euler_characteristic(len(m.vertices), m.faces) == 2
    assert mc.signed_volume(m.vertices, m.faces) / (1.0 / 4) ** 3 == pytest.approx(61.25, abs=1e-9)


def test_restatement_empty(tab):
    m = mc.reference_mesh(mc.below(4), 0.5)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)


@pytest.mark.parametrize("D,vol_tol", [(8, 0.05), (16, 0.02)])
def test_restatement_blob_radius_and_volume(tab, D, vol_tol):
    m = ref("blob", D)
    h = 1.0 / D
    r_err = np.abs(np.linalg.norm(m.vertices, axis=1) - mc.R0).max()
    vol = mc.signed_volume(m.vertices, m.faces)
    exact = 4.0 / 3.0 * math.pi * mc.R0 ** 3
    print("D=%d: max | |v| - r0 | = %.4f (2 h^2 = %.4f), volume off by %.2f %%" % (D, r_err, 2 * h * h, 100 * abs(vol / exact - 1)))
    assert r_err <= 2 * h * h
    assert abs(vol / exact - 1) <= vol_tol


def test_restatement_axis_order(tab):
    m = mc.reference_mesh(mc.ellipsoid(16), 0.5)
    for a in range(3):
        assert abs(m.vertices[:, a].max() - mc.ELLIPSOID_RADII[a]) <= 1.0 / 16
        assert abs(m.vertices[:, a].min() + mc.ELLIPSOID_RADII[a]) <= 1.0 / 16


# ----------------------------------------------------------------------------------------------------------------- argument checks
def test_c_abi_argument_errors_without_a_device(built_lib):
    L = _lib.lib()
    fake = 0x1000                                                # never dereferenced: every check runs before the first HIP call
    assert L.forge_mesh_case_table(None, 154) == -1
    assert L.forge_mesh_case_table((ctypes.c_int * 10)(), 10) == -1
    assert L.forge_mesh_workspace_bytes(1, 64, 64, 64) > 65 ** 3 * 12
    assert L.forge_mesh_workspace_bytes(1, 0, 4, 4) == -1
    assert L.forge_mesh_workspace_bytes(0, 4, 4, 4) == -1
    assert L.forge_mesh_workspace_bytes(1, 600, 600, 600) == -2         # 601^3 cells x 12 triangles is past 32-bit offsets
    assert L.forge_mesh_workspace_bytes(1, 562, 562, 562) > 0           # 563^3 = 178 453 547 <= (2^31 - 1) / 12
    ws = 1 << 30

    def count(density=fake, n=1, D=4, H=4, W=4, level=0.5, workspace=fake, nbytes=ws, counts=fake):
        return L.forge_mesh_count(density, n, D, H, W, level, workspace, nbytes, counts, None)

    assert count(density=None) == -1 and count(workspace=None) == -1 and count(counts=None) == -1
    assert b"null pointer" in L.forge_last_error()
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        assert count(level=bad) == -1
    assert b"level" in L.forge_last_error()
    assert count(D=0) == -1 and count(H=-1) == -1 and count(n=0) == -1
    assert count(D=600, H=600, W=600) == -2
    assert count(nbytes=16) == -1
    assert b"workspace" in L.forge_last_error()

    def emit(density=fake, features=None, n=1, C=0, D=4, H=4, W=4, level=0.5, vs=1.0, workspace=fake, nbytes=ws, counts=fake, offsets=None, mv=8, mf=8,
             vertices=fake, normals=fake, faces=fake, vfeat=None, status=fake):
        return L.forge_mesh_emit(density, features, n, C, D, H, W, level, vs, workspace, nbytes, counts, offsets, mv, mf, vertices, normals, faces, vfeat,
                                 status, None)

    assert emit(density=None) == -1 and emit(counts=None) == -1 and emit(status=None) == -1 and emit(vertices=None) == -1 and emit(faces=None) == -1
    assert emit(level=0.0) == -1 and emit(level=float("nan")) == -1 and emit(vs=0.0) == -1
    assert emit(mv=-1) == -1 and emit(W=0) == -1 and emit(nbytes=16) == -1
    assert emit(features=fake, C=6, vfeat=fake) == -2                   # C % 4
    assert emit(features=fake, C=0, vfeat=fake) == -2
    assert emit(features=fake, C=8, vfeat=None) == -1
    assert emit(D=600, H=600, W=600) == -2


def test_extract_mesh_refuses_cpu_tensors():
    from forge_amd import geometry, ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.extract_mesh(torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_count(torch.zeros(1, 1, 4, 4, 4))
    assert ops.MESH_OVERFLOW == 1


# ---------------------------------------------------------------------------------------------------------------------------- writers
def _cpu_mesh(tab):
    from forge_amd.geometry import Mesh
    m = ref("blob", 8)
    return Mesh(torch.from_numpy(m.vertices.astype(np.float32)), torch.from_numpy(m.normals.astype(np.float32)), torch.from_numpy(m.faces))


def test_ply_round_trip(tab, tmp_path):
    mesh = _cpu_mesh(tab)
    path = tmp_path / "blob.ply"
    mesh.to_ply(str(path))
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property float")]
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert len(body) == nv * 24 + nf * 13
    v = np.frombuffer(body[:nv * 24], "<f4").reshape(nv, 6)
    faces = []
    for k in range(nf):
        cnt, a, b, c = struct.unpack_from("<Biii", body, nv * 24 + 13 * k)
        assert cnt == 3
        faces.append((a, b, c))
    assert np.array_equal(v[:, :3], mesh.vertices.numpy()) and np.array_equal(v[:, 3:], mesh.normals.numpy())
    assert np.array_equal(np.array(faces, np.int32), mesh.faces.numpy())


def test_obj_round_trip(tab, tmp_path):
    mesh = _cpu_mesh(tab)
    path = tmp_path / "blob.obj"
    mesh.to_obj(str(path))
    v, vn, f = [], [], []
    for line in path.read_text().split("\n"):
        w = line.split()
        if not w or w[0] == "#":
            continue
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            idx = [x.split("//") for x in w[1:]]
            assert all(a == b for a, b in idx)
            f.append([int(a) - 1 for a, _ in idx])
    assert np.array_equal(np.array(v, np.float32), mesh.vertices.numpy())          # %.9g round-trips float32
    assert np.array_equal(np.array(vn, np.float32), mesh.normals.numpy())
    assert np.array_equal(np.array(f, np.int32), mesh.faces.numpy())


def test_mesh_volume_and_area_on_cpu_tensors(tab):
    """volume() and area() are plain torch ops: they run wherever the mesh lives."""
    mesh = _cpu_mesh(tab)
    m = ref("blob", 8)
    assert float(mesh.volume()) == pytest.approx(mc.signed_volume(m.vertices, m.faces), rel=1e-6)
    v, f = m.vertices, m.faces
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()
    assert float(mesh.area()) == pytest.approx(area, rel=1e-6)
