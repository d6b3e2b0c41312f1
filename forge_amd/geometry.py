"""Geometry export: the reconstructed density volume as a triangle mesh.

extract_mesh runs marching tetrahedra on the Kuhn split of every cell (csrc/mesh.hip, include/forge_hip.h section g1) on the volume
`encoder_3d.get_density3D` returns, in the frame and with the field the ray-marcher uses: vertices are (x, y, z) <-> (W, H, D) in the canonical
world frame VolRender takes cameras in, and the volume is surrounded by a shell of virtual zeros, so every mesh is closed. The reference has no
counterpart; there is no CPU path."""
from collections import namedtuple

import torch

from . import ops

MeshBatch = namedtuple("MeshBatch", "vertices normals faces features counts status")
MeshBatch.__doc__ = """extract_mesh with capacities: padded device tensors of the whole batch. vertices / normals [n,max_vertices,3] float32,
faces [n,max_faces,3] int32, features [n,max_vertices,C] or None, counts [n,2] int32 (the vertices and triangles each volume NEEDS), status [n] int32
(ops.MESH_OVERFLOW where the need exceeds a capacity: what was written is then the prefix of the full result). Rows past a volume's count are zero."""


class Mesh:
    """One volume's surface on the device: vertices [Nv,3] float32 (world frame), normals [Nv,3] float32 (unit, towards the low-density side; zero
    where the field's gradient vanishes), faces [Nf,3] int32 (counter-clockwise seen from the low-density side), features [Nv,C] float32 or None."""

    def __init__(self, vertices, normals, faces, features=None):
        self.vertices, self.normals, self.faces, self.features = vertices, normals, faces, features

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

    def to_ply(self, path):
        """Binary little-endian PLY: x y z nx ny nz per vertex (float32), then `3 i j k` per face (uchar count, int32 indices)."""
        import numpy as np
        v = torch.cat([self.vertices, self.normals], dim=1).detach().cpu().numpy().astype("<f4")
        f = self.faces.detach().cpu().numpy().astype("<i4")
        head = ("ply\nformat binary_little_endian 1.0\ncomment forge_amd.geometry\nelement vertex %d\n"
                "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (v.shape[0], f.shape[0]))
        rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
        rec["n"] = 3
        rec["i"] = f
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii"))
            fh.write(v.tobytes())
            fh.write(rec.tobytes())

    def to_obj(self, path):
        """Wavefront OBJ: `v`, `vn`, then `f i//i j//j k//k` (1-based; vertex i uses normal i)."""
        v = self.vertices.detach().cpu().tolist()
        n = self.normals.detach().cpu().tolist()
        f = self.faces.detach().cpu().tolist()
        with open(path, "w") as fh:
            fh.write("# forge_amd.geometry\n")
            fh.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in v)
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
