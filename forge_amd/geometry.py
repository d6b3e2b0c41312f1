"""Geometry export: the reconstructed density volume as a triangle mesh.

extract_mesh runs marching tetrahedra on the Kuhn split of every cell (csrc/mesh.hip, include/forge_hip.h section g1) on the volume
`encoder_3d.get_density3D` returns, in the frame and with the field the ray-marcher uses: vertices are (x, y, z) <-> (W, H, D) in the canonical
world frame VolRender takes cameras in, and the volume is surrounded by a shell of virtual zeros, so every mesh is closed. The reference has no
counterpart; there is no CPU path.

bake_vertex_colors gives those meshes their appearance (csrc/bake.hip, section g2): every vertex is projected into posed images of its volume - the
input photographs, the model's own rendered views - and takes their colours weighted by how well it faces each camera and by the transmittance of the
density field between it and the camera centre, so a camera that cannot see a vertex does not colour it. colored_mesh runs the whole chain from a
fused volume: heads, extract_mesh, nvs.render_360, one bake over photographs and rendered views."""
import math
from collections import namedtuple

import torch

from . import ops

MeshBatch = namedtuple("MeshBatch", "vertices normals faces features counts status")
MeshBatch.__doc__ = """extract_mesh with capacities: padded device tensors of the whole batch. vertices / normals [n,max_vertices,3] float32,
faces [n,max_faces,3] int32, features [n,max_vertices,C] or None, counts [n,2] int32 (the vertices and triangles each volume NEEDS), status [n] int32
(ops.MESH_OVERFLOW where the need exceeds a capacity: what was written is then the prefix of the full result). Rows past a volume's count are zero."""


class Mesh:
    """One volume's surface on the device: vertices [Nv,3] float32 (world frame), normals [Nv,3] float32 (unit, towards the low-density side; zero
    where the field's gradient vanishes), faces [Nf,3] int32 (counter-clockwise seen from the low-density side), features [Nv,C] float32 or None,
    colors [Nv,C] float32 or None (bake_vertex_colors; written to PLY / OBJ as RGB when C >= 3)."""

    def __init__(self, vertices, normals, faces, features=None, colors=None):
        self.vertices, self.normals, self.faces, self.features, self.colors = vertices, normals, faces, features, colors

    def __repr__(self):
        return "Mesh(%d vertices, %d faces%s)" % (self.vertices.shape[0], self.faces.shape[0],
                                                  "" if self.features is None else ", %d feature channels" % self.features.shape[1])

    def _corners(self):
        v = self.vertices.to(torch.float64)
        f = self.faces.long()
        return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]

    def volume(self):
        """Enclosed volume (float64 0-d tensor on the device): the sum of the signed tetrahedra (origin, a, b, c); positive for this module's
        winding. Exact for a closed surface, which every extracted mesh is."""
        a, b, c = self._corners()
        return (a * torch.linalg.cross(b, c)).sum() / 6.0

    def area(self):
        """Surface area (float64 0-d tensor on the device)."""
        a, b, c = self._corners()
        return torch.linalg.cross(b - a, c - a).norm(dim=1).sum() / 2.0

    def _rgb(self):
        """colors as RGB in [0, 1] on the host ([Nv,3] float32), or None without colours or with fewer than 3 channels."""
        if self.colors is None or self.colors.shape[1] < 3:
            return None
        return self.colors[:, :3].detach().to(torch.float32).clamp(0.0, 1.0).cpu()

    def to_ply(self, path):
        """Binary little-endian PLY: x y z nx ny nz per vertex (float32), with colours (C >= 3) followed by `uchar red green blue` =
        round-to-nearest of clamp(c, 0, 1) 255; then `3 i j k` per face (uchar count, int32 indices)."""
        import numpy as np
        v = torch.cat([self.vertices, self.normals], dim=1).detach().cpu().numpy().astype("<f4")
        f = self.faces.detach().cpu().numpy().astype("<i4")
        rgb = self._rgb()
        head = ("ply\nformat binary_little_endian 1.0\ncomment forge_amd.geometry\nelement vertex %d\n"
                "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n%s"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
                % (v.shape[0], "" if rgb is None else "property uchar red\nproperty uchar green\nproperty uchar blue\n", f.shape[0]))
        if rgb is not None:
            vc = np.empty(v.shape[0], dtype=[("v", "<f4", (6,)), ("c", "u1", (3,))])
            vc["v"] = v
            vc["c"] = np.rint(rgb.numpy() * np.float32(255.0)).astype("u1")
            v = vc
        rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
        rec["n"] = 3
        rec["i"] = f
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii"))
            fh.write(v.tobytes())
            fh.write(rec.tobytes())

    def to_obj(self, path):
        """Wavefront OBJ: `v` (with colours, C >= 3: `v x y z r g b`, clamped to [0, 1]), `vn`, then `f i//i j//j k//k` (1-based; vertex i uses
        normal i)."""
        v = self.vertices.detach().cpu().tolist()
        n = self.normals.detach().cpu().tolist()
        f = self.faces.detach().cpu().tolist()
        rgb = self._rgb()
        with open(path, "w") as fh:
            fh.write("# forge_amd.geometry\n")
            if rgb is None:
                fh.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in v)
            else:
                fh.writelines("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(p + c) for p, c in zip(v, rgb.tolist()))
            fh.writelines("vn %.9g %.9g %.9g\n" % tuple(p) for p in n)
            fh.writelines("f %d//%d %d//%d %d//%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in f)


def extract_mesh(density, level=0.5, volume_size=1.0, features=None, max_vertices=None, max_faces=None):
    """Iso-surface `density = level` of density [n,1,D,H,W] (float32, on the device) as triangle meshes; features [n,C,D,H,W] (channels-last,
    C % 4 == 0), when given, are interpolated onto the vertices. volume_size is config.render.volume_size. level must be finite and > 0.

    Without capacities: one read-back of the per-volume counts (the only host synchronisation), exact allocation, a list of n Mesh (an empty
    surface gives empty tensors). With max_vertices and max_faces: no synchronisation at all - a MeshBatch of padded tensors with device counts
    and status, which can sit inside a captured graph. The order of vertices and triangles is specified (include/forge_hip.h) and reproducible."""
    if (max_vertices is None) != (max_faces is None):
        raise ValueError("extract_mesh: give both max_vertices and max_faces, or neither")
    counts, ws = ops.mesh_count(density, level)
    n = density.shape[0]
    if max_vertices is not None:
        mv, mf = int(max_vertices), int(max_faces)
        C = 0 if features is None else features.shape[1]
        dev = density.device
        out = (torch.zeros(n, mv, 3, device=dev), torch.zeros(n, mv, 3, device=dev), torch.zeros(n, mf, 3, dtype=torch.int32, device=dev),
               None if features is None else torch.zeros(n, mv, C, device=dev))
        v, nr, f, vf, status = ops.mesh_emit(density, ws, counts, mv, mf, level, volume_size, features, out=out)
        return MeshBatch(v, nr, f, vf, counts, status)
    ends = torch.cumsum(counts, dim=0, dtype=torch.int32)
    offsets = (ends - counts).contiguous()
    host = counts.cpu()                                           # the one synchronisation
    total_v, total_f = (int(x) for x in host.sum(dim=0, dtype=torch.int64))
    if max(total_v, total_f) > 2 ** 31 - 1:
        raise ValueError("extract_mesh: %d vertices and %d triangles in one batch exceed int32 rows; extract fewer volumes per call" % (total_v, total_f))
    v, nr, f, vf, _ = ops.mesh_emit(density, ws, counts, total_v, total_f, level, volume_size, features, offsets=offsets)
    meshes, v0, f0 = [], 0, 0
    for nv, nf in host.tolist():
        meshes.append(Mesh(v[v0:v0 + nv], nr[v0:v0 + nv], f[f0:f0 + nf], None if vf is None else vf[v0:v0 + nv]))
        v0 += nv
        f0 += nf
    return meshes


def pack_bake_cameras(cameras, image_hw, img_size=None, device=None):
    """The {'R' [V,3,3], 'T' [V,3], 'K' [V,3,3]} dict VolRender takes (K in pixels of img_size x img_size images) -> cam [V,16] as forge_mesh_bake
    takes it, for images of image_hw = (Hi, Wi): fx, cx scaled by Wi / img_size, fy, cy by Hi / img_size (img_size None: K is already in pixels of the
    images). A packed [V,16] tensor is taken as it is."""
    if torch.is_tensor(cameras):
        if cameras.dim() != 2 or cameras.shape[1] != 16:
            raise ValueError("bake: packed cameras must be [V,16], got %s" % (tuple(cameras.shape),))
        return cameras.to(device=device, dtype=torch.float32).contiguous()
    R, T, K = (cameras[k].to(device=device, dtype=torch.float32) for k in ("R", "T", "K"))
    V = R.shape[0]
    Hi, Wi = image_hw
    sx, sy = (1.0, 1.0) if img_size is None else (Wi / float(img_size), Hi / float(img_size))
    return torch.cat([R.reshape(V, 9), T.reshape(V, 3), K[:, 0, 0:1] * sx, K[:, 1, 1:2] * sy, K[:, 0, 2:3] * sx, K[:, 1, 2:3] * sy], dim=1).contiguous()


def bake_vertex_colors(meshes, density, images, cameras, view2vol=None, volume_size=1.0, img_size=None, view_weight=None, view_gain=None,
                       step=None, S=None, offset=None, **knobs):
    """Colours for the vertices of extract_mesh(density, ...) from posed images, visibility-aware (include/forge_hip.h section g2).

    meshes: the list of Mesh or the MeshBatch extract_mesh returned for `density` [n,1,D,H,W]; images [V,C,Hi,Wi] (C in 1..4) on the device; cameras:
    the {'R','T','K'} dict VolRender takes, K at img_size resolution (img_size None: at the images' own), or packed [V,16]; view2vol [V]: the volume
    each view depicts (None: view v depicts volume v, or the one volume there is); view_weight [V,Hi,Wi] (a confidence or foreground map) and
    view_gain [V] optional. Defaults: step = volume_size / max(D,H,W), S = ceil(1.8 volume_size / step) samples (the segment to a camera at the
    usual distance crosses the whole volume), offset = step (the segment starts one step off the surface, along the normal). Further knobs
    (cos_power, z_near, w_min, mode, fill) go to ops.mesh_bake.

    A list of Mesh is packed into one launch and comes back as (meshes with .colors set, [(weight, best) per mesh]); a MeshBatch gives the padded
    tensors (colors [n,max_vertices,C], weight, best), zero / -1 past a volume's count, with no host synchronisation (graph-capturable)."""
    if not torch.is_tensor(density) or not torch.is_tensor(images):
        raise TypeError("bake_vertex_colors: density and images must be tensors")
    ops._require_cuda(density, images)
    if density.dim() != 5 or images.dim() != 4:
        raise ValueError("bake_vertex_colors: density [n,1,D,H,W] and images [V,C,Hi,Wi], got %s and %s" % (tuple(density.shape), tuple(images.shape)))
    dev = density.device
    n, _, D, H, W = (int(s) for s in density.shape)
    V, C, Hi, Wi = (int(s) for s in images.shape)
    volume_size = float(volume_size)
    step = volume_size / max(D, H, W) if step is None else float(step)
    S = int(math.ceil(1.8 * volume_size / step)) if S is None else int(S)
    offset = step if offset is None else float(offset)
    half = tuple(0.5 * (N - 1) * volume_size / N for N in (W, H, D))                  # the mesh's rule; the renderer's for cubic volumes
    cam = pack_bake_cameras(cameras, (Hi, Wi), img_size, dev)
    if view2vol is None:
        if V != n and n != 1:
            raise ValueError("bake_vertex_colors: %d views for %d volumes: pass view2vol" % (V, n))
        view2vol = torch.arange(V, dtype=torch.int32, device=dev) if n != 1 else torch.zeros(V, dtype=torch.int32, device=dev)
    else:
        view2vol = view2vol.to(device=dev, dtype=torch.int32).contiguous()
    if view_gain is not None:
        view_gain = torch.as_tensor(view_gain, dtype=torch.float32, device=dev).contiguous()
    images = images.contiguous()
    kw = dict(view_weight=view_weight, view_gain=view_gain, half=half, S=S, step=step, offset=offset, **knobs)
    if isinstance(meshes, MeshBatch):
        mv = meshes.vertices.shape[1]
        out = (torch.zeros(n, mv, C, device=dev), torch.zeros(n, mv, device=dev), torch.full((n, mv), -1, dtype=torch.int32, device=dev))
        return ops.mesh_bake(meshes.vertices, meshes.normals, meshes.counts, density, images, cam, view2vol, out=out, **kw)
    meshes = list(meshes)
    if len(meshes) != n:
        raise ValueError("bake_vertex_colors: %d meshes for %d volumes" % (len(meshes), n))
    sizes = [[int(m.vertices.shape[0]), int(m.faces.shape[0])] for m in meshes]
    counts = torch.tensor(sizes, dtype=torch.int32).reshape(n, 2)
    offsets = (torch.cumsum(counts, dim=0, dtype=torch.int32) - counts).to(dev)
    colors, weight, best = ops.mesh_bake(torch.cat([m.vertices for m in meshes]).contiguous(), torch.cat([m.normals for m in meshes]).contiguous(),
                                         counts.to(dev), density, images, cam, view2vol, offsets=offsets, **kw)
    out, extras, v0 = [], [], 0
    for m, (nv, _) in zip(meshes, sizes):
        out.append(Mesh(m.vertices, m.normals, m.faces, m.features, colors[v0:v0 + nv]))
        extras.append((weight[v0:v0 + nv], best[v0:v0 + nv]))
        v0 += nv
    return out, extras


@torch.no_grad()
def colored_mesh(model, features_fused, K_cv2, camera_z, photos=None, photo_cameras=None, level=0.5, n_views=28, render_gain=0.05, **knobs):
    """From a fused volume to coloured meshes: features_fused [b,128,d,d,d] (encoder_3d.fuse) -> both heads -> extract_mesh(density, level) ->
    nvs.render_360 (n_views rendered views per scene) -> ONE bake over the photographs (gain 1) followed by the rendered views (gain render_gain),
    so a region no photograph sees takes the model's own rendering. photos [b,t,3,Hi,Wi] with photo_cameras, the {'R','T','K'} dict of their b t
    (refined) cameras, scene-major, K_cv2-style intrinsics in pixels of the photographs - exactly what `model.render` would be given; K_cv2 [3,3]
    the intrinsics of the rendered views (config.dataset.img_size). The 360-degree path hands PyTorch3D-convention (R, T) to the renderer as if
    they were OpenCV extrinsics (nvs.py); the bake is given the same (R, T) and inverts the same mapping, so the quirk cancels.
    Returns what bake_vertex_colors returns for a list: (meshes, [(weight, best) per mesh])."""
    from . import nvs
    features_mv, densities_mv = model.encoder_3d.heads(features_fused)
    densities_mv = densities_mv.contiguous()
    volume_size = model.render.volume_physical_size
    b, dev = densities_mv.shape[0], densities_mv.device
    meshes = extract_mesh(densities_mv, level=level, volume_size=volume_size)
    imgs = nvs.render_360(model, features_mv, densities_mv, K_cv2, camera_z, n_views=n_views)[0]
    R, T = nvs.nvs_cameras(camera_z, n_views, dev)
    cams = {"R": R.repeat(b, 1, 1), "T": T.repeat(b, 1), "K": K_cv2.to(dev)[None].repeat(b * n_views, 1, 1)}
    images = imgs.reshape(b * n_views, *imgs.shape[2:])
    v2v = torch.arange(b, dtype=torch.int32, device=dev).repeat_interleave(n_views)
    gain = torch.full((b * n_views,), float(render_gain), device=dev)
    if photos is not None:
        if photo_cameras is None:
            raise ValueError("colored_mesh: photos need photo_cameras")
        t = photos.shape[1]
        if tuple(photos.shape[2:]) != tuple(images.shape[1:]):
            raise ValueError("colored_mesh: photos %s and rendered views %s must have the same channels and resolution" % (tuple(photos.shape[2:]), tuple(images.shape[1:])))
        images = torch.cat([photos.reshape(b * t, *photos.shape[2:]).to(dev, torch.float32), images])
        cams = {k: torch.cat([photo_cameras[k].to(device=dev, dtype=torch.float32), cams[k]]) for k in ("R", "T", "K")}
        v2v = torch.cat([torch.arange(b, dtype=torch.int32, device=dev).repeat_interleave(t), v2v])
        gain = torch.cat([torch.ones(b * t, device=dev), gain])
    return bake_vertex_colors(meshes, densities_mv, images, cams, view2vol=v2v, volume_size=volume_size, view_gain=gain, **knobs)
