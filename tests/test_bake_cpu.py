"""The vertex-colour bake without a GPU: analytic known answers of the contract's numpy restatement (tests/bake_cases.py), the argument checks of
forge_mesh_bake, the refusal of CPU tensors and the coloured mesh writers."""
import struct

import numpy as np
import pytest
import torch

import bake_cases as bc
import mesh_cases as mc
from forge_amd import _lib
from forge_amd.ops import BAKE_MODES          # the restatement's `mode` values are the ones ops.mesh_bake hands to forge_mesh_bake

ZERO8 = np.zeros((8, 8, 8), np.float32)
HALF8 = bc.half_extents((8, 8, 8))


def one_camera(Hi=16, Wi=16, center=(0.0, 0.0, -1.5)):
    return bc.pack([center], Hi, Wi)


def project(cam, p):
    """(x, y) of the contract for world points p [rows,3], in float64."""
    c = cam.astype(np.float64)
    q = p @ c[:9].reshape(3, 3).T + c[9:12]
    return c[12] * q[:, 0] / q[:, 2] + c[14] - 0.5, c[13] * q[:, 1] / q[:, 2] + c[15] - 0.5


# ------------------------------------------------------------------------------------------------------ known answers of the restatement
@pytest.mark.parametrize("cos_power", [1, 2, 5])
def test_free_space_affine_image_and_cosine_weight(cos_power):
    """Zero density, one view, an image that is an affine function of the pixel position: bilinear interpolation reproduces it exactly at the
    projected point, T = 1, so the colour is that function there and the weight is cos^p of the angle between normal and view direction."""
    Hi, Wi = 16, 24
    cam = one_camera(Hi, Wi)
    hh, ww = np.meshgrid(np.arange(Hi, dtype=np.float64), np.arange(Wi, dtype=np.float64), indexing="ij")
    coef = np.array([[0.1, 0.02, 0.01], [0.7, -0.015, 0.02], [0.3, 0.0, -0.01]])                 # a + b w + c h per channel
    images = np.stack([a + b * ww + c * hh for a, b, c in coef])[None].astype(np.float32)
    rng = np.random.default_rng(0)
    p = rng.uniform(-0.3, 0.3, (40, 3)).astype(np.float32)
    nh = rng.standard_normal((40, 3))
    nh[:, 2] = -np.abs(nh[:, 2]) - 0.5                                                           # towards the camera at z = -1.5
    nh = (nh / np.linalg.norm(nh, axis=1, keepdims=True)).astype(np.float32)
    r = bc.reference_bake(p, nh, ZERO8, HALF8, images, cam, [0], S=14, step=0.125, offset=0.125, cos_power=cos_power, w_min=0.0, mode=BAKE_MODES["blend"])
    x, y = project(cam[0], p.astype(np.float64))
    want = np.stack([a + b * x + c * y for a, b, c in coef], axis=1)
    assert np.abs(r.colors - want).max() < 5e-7                                                  # the pixels are the function rounded to float32: 6e-8 each
    d = np.array([0.0, 0.0, -1.5]) - p.astype(np.float64)
    cosine = (nh.astype(np.float64) * d / np.linalg.norm(d, axis=1, keepdims=True)).sum(axis=1)
    assert (cosine > 0).all()
    assert np.abs(r.weight - cosine ** cos_power).max() < 1e-12
    assert (r.best == 0).all() and r.margin > 1.0


def test_slab_between_vertex_and_camera_blocks_exactly():
    """Density >= 1 on whole planes between the vertex and the camera: some sample has a_s = 1, so T = 0 exactly, the colour is `fill`, best -1."""
    dens = ZERO8.copy()
    dens[1:3] = 1.75                                                                             # planes z index 1, 2: world z = -0.3125, -0.1875
    p = np.array([[0.0, 0.0, 0.2], [0.1, -0.1, 0.3], [-0.2, 0.05, 0.1]], np.float32)
    nh = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (3, 1))
    images = bc.random_images(1, 3, 16, 16, 1)
    r = bc.reference_bake(p, nh, dens, HALF8, images, one_camera(), [0], S=15, step=0.125, offset=0.0, fill=0.25)
    assert (r.weight == 0.0).all() and (r.best == -1).all() and (r.colors == 0.25).all()
    clear = bc.reference_bake(p, nh, ZERO8, HALF8, images, one_camera(), [0], S=15, step=0.125, offset=0.0, fill=0.25)
    assert (clear.weight > 0.9).all() and (clear.best == 0).all()                                # the same rows see the camera through free space


def test_two_opposite_cameras_each_vertex_takes_its_side():
    sc = bc.scene("blob8_one_view")
    dens, v, nh, _ = sc.volumes[0]
    centers = [(0.0, 0.0, -1.5), (0.0, 0.0, 1.5)]
    cam = bc.pack(centers, 16, 16)
    r = bc.reference_bake(v, nh, dens, sc.half, bc.random_images(2, 3, 16, 16, 2), cam, [0, 0], S=15, step=0.125, offset=0.125)
    checked = 0
    for k, c in enumerate(centers):
        d = np.asarray(c) - v.astype(np.float64)
        cosine = (nh.astype(np.float64) * d / np.linalg.norm(d, axis=1, keepdims=True)).sum(axis=1)
        side = cosine > 0.2
        checked += side.sum()
        assert (r.best[side] == k).all() and (r.per_view[1 - k][side] == 0.0).all()
    assert checked > 0.5 * len(v)


def test_vertices_behind_the_camera_or_outside_the_image_get_no_colour():
    cam = one_camera()
    p = np.array([[0.0, 0.0, -2.0],            # behind the camera at z = -1.5
                  [1.2, 0.0, 0.0],             # in front, but projects right of the image
                  [0.0, -1.2, 0.0],            # above it
                  [0.0, 0.0, 0.0]], np.float32)
    nh = np.zeros((4, 3), np.float32)          # zero normals: facing 1, so only the in-view test decides
    r = bc.reference_bake(p, nh, ZERO8, HALF8, bc.random_images(1, 3, 16, 16, 3), cam, [0], S=4, step=0.125, offset=0.125, fill=0.5)
    assert r.weight.tolist() == [0.0, 0.0, 0.0, 1.0] and r.best.tolist() == [-1, -1, -1, 0]
    assert (r.colors[:3] == 0.5).all() and r.margin > 1e-3


def test_views_of_other_volumes_and_unknown_volumes_are_ignored():
    sc = bc.scene("two_blobs8_interleaved")
    a, b = sc.reference()
    assert (a.per_view[[1, 3, 4]] == 0).all() and (b.per_view[[0, 2, 3, 5]] == 0).all()
    assert set(np.unique(a.best)) <= {-1, 0, 2, 5} and set(np.unique(b.best)) <= {-1, 1, 4}


# ----------------------------------------------------------------------------------------------------------------- argument checks
def test_c_abi_argument_errors_without_a_device(built_lib):
    L = _lib.lib()
    fake = 0x1000                                                # never dereferenced: every check runs before the first HIP call
    EINVAL, ESHAPE = -1, -2

    def bake(vertices=fake, normals=fake, counts=fake, offsets=None, n=1, mv=8, density=fake, D=4, H=4, W=4, half=(0.4, 0.4, 0.4), images=fake,
             view_weight=None, C=3, Hi=8, Wi=8, cam=fake, view2vol=fake, view_gain=None, V=1, S=4, step=0.25, offset=0.25, cos_power=2, z_near=1e-3,
             w_min=1e-3, mode=0, fill=0.5, colors=fake, weight=fake, best=fake):
        return L.forge_mesh_bake(vertices, normals, counts, offsets, n, mv, density, D, H, W, *half, images, view_weight, C, Hi, Wi, cam, view2vol, view_gain, V,
                                 S, step, offset, cos_power, z_near, w_min, mode, fill, colors, weight, best, None)

    for name in ("vertices", "normals", "counts", "density", "images", "cam", "view2vol", "colors", "weight", "best"):
        assert bake(**{name: None}) == EINVAL, name
        assert b"null pointer" in L.forge_last_error()
    for bad in (0.0, -0.25, float("inf"), float("nan")):
        assert bake(step=bad) == EINVAL
    assert b"step" in L.forge_last_error()
    assert bake(S=0) == EINVAL and bake(V=0) == EINVAL
    assert bake(cos_power=0) == EINVAL and bake(cos_power=9) == EINVAL
    assert b"cos_power" in L.forge_last_error()
    assert bake(mode=2) == EINVAL and bake(mode=-1) == EINVAL
    assert bake(w_min=-1e-3) == EINVAL and bake(offset=-0.1) == EINVAL
    assert bake(n=0) == EINVAL and bake(D=0) == EINVAL and bake(Hi=0) == EINVAL and bake(mv=-1) == EINVAL
    assert bake(half=(0.4, 0.0, 0.4)) == EINVAL and bake(z_near=0.0) == EINVAL
    assert bake(C=0) == ESHAPE and bake(C=5) == ESHAPE
    assert b"channels" in L.forge_last_error()
    assert bake(D=2048, H=2048, W=2048) == ESHAPE                       # 2^33 voxels: beyond the 32-bit tap index
    assert bake(Hi=65536, Wi=65536) == ESHAPE
    assert bake(n=70000) == ESHAPE
    assert bake(n=4096, mv=1 << 20) == ESHAPE                           # 2^32 rows in capacity mode
    # zero rows: nothing to launch, also with null row arrays (empty tensors have no storage)
    assert bake(mv=0, vertices=None, normals=None, colors=None, weight=None, best=None) == 0


def test_bake_refuses_cpu_tensors():
    from forge_amd import geometry, ops
    mesh = geometry.Mesh(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32))
    cam = torch.from_numpy(one_camera())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.bake_vertex_colors([mesh], torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 3, 16, 16), cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_bake(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 3, 16, 16),
                      cam, torch.zeros(1, dtype=torch.int32), half=(0.4, 0.4, 0.4), S=4, step=0.25, offset=0.25)
    assert ops.BAKE_MODES is BAKE_MODES and BAKE_MODES == {"blend": 0, "best": 1}


def test_pack_bake_cameras_scales_intrinsics_to_the_images():
    from forge_amd import geometry
    K = torch.tensor([[[355.0, 0.0, 128.0], [0.0, 350.0, 120.0], [0.0, 0.0, 1.0]]])
    cams = {"R": torch.eye(3)[None], "T": torch.tensor([[0.0, 0.0, 1.5]]), "K": K}
    same = geometry.pack_bake_cameras(cams, (256, 256))
    assert same.shape == (1, 16) and same[0, 12:].tolist() == [355.0, 350.0, 128.0, 120.0] and same[0, :9].tolist() == torch.eye(3).reshape(9).tolist()
    half = geometry.pack_bake_cameras(cams, (64, 128), img_size=256)           # Hi = 64, Wi = 128: x by 1/2, y by 1/4
    assert half[0, 12:].tolist() == [177.5, 87.5, 64.0, 30.0]
    assert geometry.pack_bake_cameras(same, (256, 256)) is not None and torch.equal(geometry.pack_bake_cameras(same, (1, 1)), same)
    with pytest.raises(ValueError):
        geometry.pack_bake_cameras(torch.zeros(3, 12), (4, 4))


# ---------------------------------------------------------------------------------------------------------------------------- writers
def _meshes():
    from forge_amd.geometry import Mesh
    _, v, nh, f = bc.ref_mesh32("blob8", lambda: mc.blob(8))
    rng = np.random.default_rng(5)
    col = rng.uniform(-0.2, 1.2, (len(v), 4)).astype(np.float32)                 # beyond [0, 1]: the writers clamp; a 4th channel: ignored
    col[:4, :3] = [[0.0, 1.0, 0.5], [0.5 / 255, 1.5 / 255, 2.5 / 255], [0.25, 0.75, 1.0], [0.999, 0.001, 0.4]]
    plain = Mesh(torch.from_numpy(v), torch.from_numpy(nh), torch.from_numpy(f))
    return plain, Mesh(plain.vertices, plain.normals, plain.faces, colors=torch.from_numpy(col)), col


def _legacy_ply(mesh):
    """The bytes to_ply wrote before colours existed, restated."""
    v = np.concatenate([mesh.vertices.numpy(), mesh.normals.numpy()], axis=1).astype("<f4")
    f = mesh.faces.numpy().astype("<i4")
    head = ("ply\nformat binary_little_endian 1.0\ncomment forge_amd.geometry\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (v.shape[0], f.shape[0]))
    body = b"".join(struct.pack("<Biii", 3, *tri) for tri in f.tolist())
    return head.encode("ascii") + v.tobytes() + body


def _legacy_obj(mesh):
    lines = ["# forge_amd.geometry\n"]
    lines += ["v %.9g %.9g %.9g\n" % tuple(p) for p in mesh.vertices.tolist()]
    lines += ["vn %.9g %.9g %.9g\n" % tuple(p) for p in mesh.normals.tolist()]
    lines += ["f %d//%d %d//%d %d//%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in mesh.faces.tolist()]
    return "".join(lines)


def test_colourless_files_are_unchanged_byte_for_byte(tmp_path):
    from forge_amd.geometry import Mesh
    plain, coloured, col = _meshes()
    two = Mesh(plain.vertices, plain.normals, plain.faces, colors=torch.from_numpy(col[:, :2].copy()))      # fewer than 3 channels: no RGB either
    for k, m in enumerate((plain, two)):
        m.to_ply(str(tmp_path / ("m%d.ply" % k)))
        m.to_obj(str(tmp_path / ("m%d.obj" % k)))
        assert (tmp_path / ("m%d.ply" % k)).read_bytes() == _legacy_ply(plain)
        assert (tmp_path / ("m%d.obj" % k)).read_text() == _legacy_obj(plain)
    assert plain.colors is None and "colors" not in repr(plain)


def test_ply_round_trip_with_colours(tmp_path):
    _, mesh, col = _meshes()
    path = tmp_path / "blob.ply"
    mesh.to_ply(str(path))
    head, body = path.read_bytes().split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    props = [l.split()[1:] for l in lines if l.startswith("property") and "list" not in l]
    assert props == [["float", k] for k in ("x", "y", "z", "nx", "ny", "nz")] + [["uchar", k] for k in ("red", "green", "blue")]
    assert lines.index("property uchar red") == lines.index("property float nz") + 1 and len(body) == nv * 27 + nf * 13
    rec = np.frombuffer(body[:nv * 27], dtype=[("v", "<f4", (6,)), ("c", "u1", (3,))])
    assert np.array_equal(rec["v"][:, :3], mesh.vertices.numpy()) and np.array_equal(rec["v"][:, 3:], mesh.normals.numpy())
    want = np.rint(np.clip(col[:, :3].astype(np.float64), 0.0, 1.0) * 255.0)
    got = rec["c"].astype(np.float64)
    exact = np.abs(np.clip(col[:, :3].astype(np.float64), 0, 1) * 255.0 % 1.0 - 0.5) > 1e-4           # away from a rounding tie of the fp32 product
    assert np.array_equal(got[exact], want[exact]) and np.abs(got - want).max() <= 1.0
    assert rec["c"][0].tolist() == [0, 255, 128] and rec["c"][2].tolist() == [64, 191, 255] and rec["c"][3].tolist() == [255, 0, 102]
    faces = np.array([struct.unpack_from("<Biii", body, nv * 27 + 13 * k) for k in range(nf)])
    assert (faces[:, 0] == 3).all() and np.array_equal(faces[:, 1:].astype(np.int32), mesh.faces.numpy())


def test_obj_round_trip_with_colours(tmp_path):
    _, mesh, col = _meshes()
    path = tmp_path / "blob.obj"
    mesh.to_obj(str(path))
    v, vn, f = [], [], []
    for line in path.read_text().split("\n"):
        w = line.split()
        if not w or w[0] == "#":
            continue
        if w[0] == "v":
            assert len(w) == 7
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            f.append([int(x.split("//")[0]) - 1 for x in w[1:]])
    v = np.array(v, np.float32)
    assert np.array_equal(v[:, :3], mesh.vertices.numpy()) and np.array_equal(v[:, 3:], np.clip(col[:, :3], 0.0, 1.0))     # %.9g round-trips float32
    assert np.array_equal(np.array(vn, np.float32), mesh.normals.numpy()) and np.array_equal(np.array(f, np.int32), mesh.faces.numpy())
