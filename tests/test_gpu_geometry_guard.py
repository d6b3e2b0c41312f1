"""A negative offset of the packed row layout is never followed (csrc/geom_common.h row_span; include/forge_hip.h sections g1, g2, g3): the volume
touches no row of any array in forge_mesh_emit, forge_mesh_bake and forge_surface_sample alike, whether the vertex offset, the face offset or
both are negative. Two 4^3 volumes, offsets[1] = (-2, -2), (-2, valid), (valid, -2). Every array a kernel
could reach below is a view that starts GUARD rows inside a larger allocation filled with a sentinel, so even a wrong guard stays inside the
allocation and shows as a changed sentinel row."""
import numpy as np
import pytest
import torch

import bake_cases as bc
import mesh_cases as mc
from forge_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 8
BAD = ("both", "vertices", "faces")                                    # which offset of volume 1 is -2
SENTINEL = {torch.float32: -777.25, torch.int32: -12345}
_CACHE = {}


def guarded(rows, tail, dtype):
    """(the whole allocation, the view of `rows` rows that starts GUARD rows in), all sentinel"""
    whole = torch.full((GUARD + rows + GUARD,) + tail, SENTINEL[dtype], dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + rows]


def untouched(whole, lo, hi):
    """every row of the allocation outside the view's rows lo .. hi - 1 still holds the sentinel"""
    keep = torch.ones(whole.shape[0], dtype=torch.bool, device=whole.device)
    keep[GUARD + lo:GUARD + hi] = False
    return bool((whole[keep] == SENTINEL[whole.dtype]).all())


def setup():
    """density, counts, workspace, the good and the bad offsets, the host counts, and the unguarded packed mesh (views inside sentinel allocations)"""
    if not _CACHE:
        dens = torch.from_numpy(np.stack([mc.blob(4, (0.03, -0.02, 0.01)), mc.blob(4, (-0.02, 0.01, 0.03))])[:, None]).cuda()
        counts, ws = ops.mesh_count(dens)
        good = (torch.cumsum(counts, dim=0, dtype=torch.int32) - counts).contiguous()
        bad = {"both": good.clone(), "vertices": good.clone(), "faces": good.clone()}
        bad["both"][1] = -2
        bad["vertices"][1, 0] = -2
        bad["faces"][1, 1] = -2
        host = counts.cpu().tolist()
        assert min(host[0] + host[1]) > 2                              # both volumes have something to emit
        tv, tf = host[0][0] + host[1][0], host[0][1] + host[1][1]
        arrays = [guarded(tv, (3,), torch.float32), guarded(tv, (3,), torch.float32), guarded(tf, (3,), torch.int32)]
        _, _, _, _, status = ops.mesh_emit(dens, ws, counts, tv, tf, offsets=good, out=tuple(v for _, v in arrays) + (None,))
        assert status.cpu().tolist() == [0, 0]
        _CACHE.update(dens=dens, counts=counts, ws=ws, good=good, bad=bad, host=host, tv=tv, tf=tf, mesh=arrays)
    return _CACHE


@pytest.mark.parametrize("which", BAD)
def test_mesh_emit_does_not_follow_a_negative_offset(which):
    s = setup()
    (nv0, nf0), tv, tf = s["host"][0], s["tv"], s["tf"]
    arrays = [guarded(tv, (3,), torch.float32), guarded(tv, (3,), torch.float32), guarded(tf, (3,), torch.int32)]
    _, _, _, _, status = ops.mesh_emit(s["dens"], s["ws"], s["counts"], tv, tf, offsets=s["bad"][which], out=tuple(v for _, v in arrays) + (None,))
    assert status.cpu().tolist() == [0, ops.MESH_OVERFLOW]
    for (whole, view), (_, ref), n0 in zip(arrays, s["mesh"], (nv0, nv0, nf0)):
        assert torch.equal(view[:n0], ref[:n0])                        # volume 0: the unguarded call's rows
        assert untouched(whole, 0, n0)                                 # the rows before the view, volume 1's rows, the rows after


def bake_inputs():
    images = torch.from_numpy(bc.random_images(3, 3, 16, 16, 5)).cuda()
    cam = torch.from_numpy(bc.pack(bc.orbit(3, phase_deg=15.0), 16, 16)).cuda()
    step, S, offset = bc.defaults((4, 4, 4))
    return images, cam, torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda"), dict(half=bc.half_extents((4, 4, 4)), S=S, step=step, offset=offset)


@pytest.mark.parametrize("which", BAD)
def test_mesh_bake_does_not_follow_a_negative_offset(which):
    s = setup()
    nv0, tv = s["host"][0][0], s["tv"]
    (_, vertices), (_, normals), _ = s["mesh"]
    images, cam, v2v, kw = bake_inputs()
    runs = {}
    for name, offsets in (("good", s["good"]), ("bad", s["bad"][which])):
        arrays = [guarded(tv, (3,), torch.float32), guarded(tv, (), torch.float32), guarded(tv, (), torch.int32)]
        ops.mesh_bake(vertices, normals, s["counts"], s["dens"], images, cam, v2v, offsets=offsets, out=tuple(v for _, v in arrays), **kw)
        runs[name] = arrays
    for (whole, view), (whole_ref, ref) in zip(runs["bad"], runs["good"]):
        assert untouched(whole_ref, 0, tv) and not untouched(whole_ref, 0, nv0)      # the unguarded call wrote both volumes, and only them
        assert torch.equal(view[:nv0], ref[:nv0])
        assert untouched(whole, 0, nv0)                                # volume 1's rows and the rows before the view are as they were


@pytest.mark.parametrize("which", BAD)
def test_surface_sample_does_not_follow_a_negative_offset(which):
    s = setup()
    (_, vertices), _, (_, faces) = s["mesh"]
    good = ops.surface_sample(vertices, faces, s["counts"], 64, offsets=s["good"])
    bad = ops.surface_sample(vertices, faces, s["counts"], 64, offsets=s["bad"][which])
    for g, b in zip(good, bad):
        assert torch.equal(g[0], b[0])
    points, normals, face, _, status = bad
    assert status.cpu().tolist() == [0, ops.GEOM_EMPTY]
    assert not points[1].any() and not normals[1].any() and bool((face[1] == -1).all())
    for whole, _ in s["mesh"]:
        assert untouched(whole, 0, whole.shape[0] - 2 * GUARD)         # inputs: read only
