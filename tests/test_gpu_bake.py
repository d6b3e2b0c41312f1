"""The vertex-colour bake on the MI355X (forge_amd.geometry.bake_vertex_colors -> csrc/bake.hip) against the float64 numpy restatement of its
contract (tests/bake_cases.py). Colour and weight tolerance of a case: 4 x the largest |float32 restatement - float64 restatement| of that case
(the factor test_gpu_parity.py grants an fp32 path over the reference's own fp32 error), computed here and printed.

Measured on the MI355X with W_MIN = 1e-3 (profiles/r19_bake_probe.txt): allowed colour error 2.3e-6 .. 4.9e-6, the kernel's 5.8e-7 .. 1.2e-6;
allowed weight error 6.9e-7 .. 1.6e-6, the kernel's 1.7e-7 .. 3.9e-7: the kernel errs as the fp32 restatement does, a quarter of what is allowed."""
import numpy as np
import pytest
import torch

import bake_cases as bc
import mesh_cases as mc
from forge_amd.ops import BAKE_MODES

pytestmark = pytest.mark.gpu

W_MIN = 1e-3
FILL = 0.5
_CACHE = {}
HAND_KNOBS = ((1, 0.125), (15, 0.125), (1, 0.3))          # (S, step) of the hand-made rows


def on_device(name):
    """(Scene, list of Mesh, density [n,1,D,H,W], dict of device inputs, float64 references, float32 references): built once, never modified."""
    if name not in _CACHE:
        from forge_amd.geometry import Mesh
        sc = bc.scene(name)
        meshes = [Mesh(torch.from_numpy(v).cuda(), torch.from_numpy(nr).cuda(), torch.from_numpy(f).cuda()) for _, v, nr, f in sc.volumes]
        dens = torch.from_numpy(np.stack([d for d, _, _, _ in sc.volumes])[:, None]).cuda()
        dev = {"images": torch.from_numpy(sc.images).cuda(), "cam": torch.from_numpy(sc.cam).cuda(), "view2vol": torch.from_numpy(sc.view2vol).cuda(),
               "view_weight": None if sc.view_weight is None else torch.from_numpy(sc.view_weight).cuda(),
               "view_gain": None if sc.view_gain is None else torch.from_numpy(sc.view_gain).cuda()}
        _CACHE[name] = [sc, meshes, dens, dev, {}]
    return _CACHE[name]


def references(name, mode):
    """(float64, float32) restatements of a scene for mode 0 / 1 (BAKE_MODES' values), computed once."""
    refs = on_device(name)[4]
    if mode not in refs:
        sc = on_device(name)[0]
        kw = dict(w_min=W_MIN, fill=FILL, mode=mode)
        refs[mode] = (sc.reference(np.float64, **kw), sc.reference(np.float32, **kw))
    return refs[mode]


def bake(name, mode="blend"):
    from forge_amd.geometry import bake_vertex_colors
    sc, meshes, dens, dev, _ = on_device(name)
    return bake_vertex_colors(meshes, dens, dev["images"], dev["cam"], dev["view2vol"], volume_size=sc.volume_size, view_weight=dev["view_weight"],
                              view_gain=dev["view_gain"], w_min=W_MIN, fill=FILL, mode=mode, **sc.knobs)


def compare(label, colors, weight, best, r64, r32, mode):
    """One volume's rows against the restatement, by the rules of the module docstring; returns nothing, asserts."""
    colors, weight, best = colors.cpu().numpy().astype(np.float64), weight.cpu().numpy().astype(np.float64), best.cpu().numpy()
    rows = len(r64.weight)
    assert colors.shape == r64.colors.shape and weight.shape == (rows,) and best.shape == (rows,) and best.dtype == np.int32
    assert r64.margin >= 1e-3                                          # no projected vertex within 1e-3 pixel of the image hull (or of z_near)
    near_tie = r64.top_two_gap() < 1e-4
    sure = r64.weight >= 2 * W_MIN
    band = (r64.weight >= W_MIN / 2) & ~sure
    low = r64.weight < W_MIN / 2
    yard = sure & ~near_tie & (r32.best == r64.best) if mode == 1 else sure          # best view: a colour is comparable only where the view is the same
    tol_c = 4 * np.abs(r32.colors.astype(np.float64) - r64.colors)[yard].max()
    tol_w = 4 * np.abs(r32.weight.astype(np.float64) - r64.weight).max()
    err_c = np.abs(colors - r64.colors).max(axis=1)
    err_w = np.abs(weight - r64.weight)
    check = sure & ~near_tie if mode == 1 else sure
    print("%s: %d rows | colour error %.3g (allowed %.3g) on %d rows | weight error %.3g (allowed %.3g) | band [w_min/2, 2 w_min) %.2f %% | near-ties %.2f %%"
          % (label, rows, err_c[check].max(), tol_c, check.sum(), err_w.max(), tol_w, 100 * band.mean(), 100 * near_tie[r64.weight > W_MIN].mean()))
    assert tol_c > 0 and tol_w > 0 and tol_w < W_MIN / 4
    assert band.mean() <= 0.05
    assert near_tie[r64.weight > W_MIN].mean() <= 0.01
    assert (err_w <= tol_w).all()
    assert (err_c[check] <= tol_c).all()
    is_fill = (colors == FILL).all(axis=1)
    assert (is_fill[band] | (err_c[band] <= tol_c)).all()
    assert is_fill[low].all()
    assert np.array_equal(best[~near_tie], r64.best[~near_tie])


@pytest.mark.parametrize("name", bc.SCENES)
def test_blend_against_float64(name):
    meshes, extras = bake(name)
    r64, r32 = references(name, BAKE_MODES["blend"])
    assert len(meshes) == len(r64)
    for k, (m, (w, b)) in enumerate(zip(meshes, extras)):
        assert m.colors.dtype == torch.float32 and w.dtype == torch.float32 and b.dtype == torch.int32 and len(r64[k].weight) > 0
        compare("%s[%d]" % (name, k), m.colors, w, b, r64[k], r32[k], 0)
    if name == "two_blobs8_interleaved":                                # the view of an unknown volume colours nobody
        assert all(int((b == 3).sum()) == 0 for _, b in extras)


def test_best_view_mode_against_float64():
    meshes, extras = bake("ellipsoid16_orbit6", mode="best")
    r64, r32 = references("ellipsoid16_orbit6", BAKE_MODES["best"])
    compare("ellipsoid16_orbit6 best view", meshes[0].colors, *extras[0], r64[0], r32[0], 1)
    blend = bake("ellipsoid16_orbit6")
    assert torch.equal(extras[0][0], blend[1][0][0]) and torch.equal(extras[0][1], blend[1][0][1])          # weight and best do not depend on the mode
    assert not torch.equal(meshes[0].colors, blend[0][0].colors)


def test_hand_made_rows_through_ops():
    """Branches a mesh never produces: a zero normal (facing 1, no offset), a vertex behind the camera, one projecting outside the image, and S = 1."""
    from forge_amd import ops
    dens, p, nh, cam, images = bc.hand_made_rows()
    rows = len(p)
    half = bc.half_extents((8, 8, 8))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for S, step in HAND_KNOBS:
        knobs = dict(S=S, step=step, offset=0.125, cos_power=1, w_min=W_MIN, fill=FILL)
        r64 = bc.reference_bake(p, nh, dens, half, images, cam, [0, 0], dtype=np.float64, **knobs)
        r32 = bc.reference_bake(p, nh, dens, half, images, cam, [0, 0], dtype=np.float32, **knobs)
        c, w, b = ops.mesh_bake(dev(p[None]), dev(nh[None]), dev(np.array([[rows, 0]], np.int32)), dev(dens[None, None]), dev(images), dev(cam),
                                dev(np.zeros(2, np.int32)), half=half, **knobs)
        assert tuple(c.shape) == (1, rows, 2) and tuple(w.shape) == (1, rows) and tuple(b.shape) == (1, rows)
        compare("hand-made rows, S = %d, step = %g" % (S, step), c[0], w[0], b[0], r64, r32, 0)
        assert b[0, 2:4].tolist() == [-1, -1] and w[0, 2:4].tolist() == [0.0, 0.0] and (c[0, 2:4] == FILL).all()
        assert float(w[0, 0]) > 0 and float(w[0, 1]) > 0


def test_no_surface_gives_no_rows():
    from forge_amd import ops
    from forge_amd.geometry import bake_vertex_colors, extract_mesh
    dens = torch.from_numpy(mc.below(8)[None, None]).cuda()
    meshes = extract_mesh(dens)
    cam = torch.from_numpy(bc.pack(bc.orbit(2), 16, 16)).cuda()
    images = torch.from_numpy(bc.random_images(2, 3, 16, 16, 1)).cuda()
    out, extras = bake_vertex_colors(meshes, dens, images, cam)
    assert tuple(out[0].colors.shape) == (0, 3) and tuple(extras[0][0].shape) == (0,) and tuple(extras[0][1].shape) == (0,)
    assert extras[0][1].dtype == torch.int32
    c, w, b = ops.mesh_bake(torch.empty(1, 0, 3, device="cuda"), torch.empty(1, 0, 3, device="cuda"), torch.zeros(1, 2, dtype=torch.int32, device="cuda"), dens,
                            images, cam, torch.zeros(2, dtype=torch.int32, device="cuda"), half=bc.half_extents((8, 8, 8)), S=4, step=0.125, offset=0.125)
    assert tuple(c.shape) == (1, 0, 3) and tuple(w.shape) == (1, 0) and tuple(b.shape) == (1, 0)


# --------------------------------------------------------------------------------------------------------------------- capacity mode
CANARY_F, CANARY_I = -7.25, -77


def _capacity_inputs():
    dens = torch.from_numpy(np.stack([mc.blob(8), mc.below(8)])[:, None]).cuda()
    cam = torch.from_numpy(bc.pack(bc.orbit(3, phase_deg=30.0, elev_deg=(0.0, 25.0, -25.0)), 16, 16)).cuda()
    images = torch.from_numpy(bc.random_images(3, 3, 16, 16, 12)).cuda()
    v2v = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    return dens, cam, images, v2v


@pytest.mark.parametrize("mv", [100, 302, 400])
def test_capacity_mode_prefix_overflow_and_canary(mv):
    from forge_amd import ops
    from forge_amd.geometry import bake_vertex_colors, extract_mesh
    dens, cam, images, v2v = _capacity_inputs()
    full, extras = bake_vertex_colors(extract_mesh(dens), dens, images, cam, v2v)
    nv = full[0].vertices.shape[0]
    assert nv == 302 and full[1].vertices.shape[0] == 0
    batch = extract_mesh(dens, max_vertices=mv, max_faces=700)
    assert batch.status.cpu().tolist() == [ops.MESH_OVERFLOW if mv < nv else 0, 0]
    n = 2
    cb = torch.full((n * mv * 3 + 96,), CANARY_F, device="cuda")
    wb = torch.full((n * mv + 96,), CANARY_F, device="cuda")
    bb = torch.full((n * mv + 96,), CANARY_I, dtype=torch.int32, device="cuda")
    out = (cb[:n * mv * 3].view(n, mv, 3), wb[:n * mv].view(n, mv), bb[:n * mv].view(n, mv))
    step, S, offset = bc.defaults((8, 8, 8))
    c, w, b = ops.mesh_bake(batch.vertices, batch.normals, batch.counts, dens, images, cam, v2v, half=bc.half_extents((8, 8, 8)), S=S, step=step, offset=offset,
                            out=out)
    k = min(mv, nv)
    assert torch.equal(c[0, :k], full[0].colors[:k]) and torch.equal(w[0, :k], extras[0][0][:k]) and torch.equal(b[0, :k], extras[0][1][:k])
    assert float(w[0, :k].max()) > 0.5
    # nothing else was written: the rest of volume 0's rows, all of the empty volume 1's rows, and the region behind the capacity
    assert (c[0, k:] == CANARY_F).all() and (w[0, k:] == CANARY_F).all() and (b[0, k:] == CANARY_I).all()
    assert (c[1] == CANARY_F).all() and (w[1] == CANARY_F).all() and (b[1] == CANARY_I).all()
    assert (cb[-96:] == CANARY_F).all() and (wb[-96:] == CANARY_F).all() and (bb[-96:] == CANARY_I).all()
    # the MeshBatch route of bake_vertex_colors: the same rows, zero / -1 past the count
    c2, w2, b2 = bake_vertex_colors(batch, dens, images, cam, v2v)
    assert torch.equal(c2[0, :k], c[0, :k]) and torch.equal(w2[0, :k], w[0, :k]) and torch.equal(b2[0, :k], b[0, :k])
    assert (c2[0, k:] == 0).all() and (w2[1] == 0).all() and (b2[0, k:] == -1).all() and (b2[1] == -1).all()


def test_determinism():
    a, ea = bake("two_blobs8_interleaved")
    b, eb = bake("two_blobs8_interleaved")
    for x, y, (wx, bx), (wy, by) in zip(a, b, ea, eb):
        assert torch.equal(x.colors.view(torch.int32), y.colors.view(torch.int32)) and torch.equal(wx.view(torch.int32), wy.view(torch.int32))
        assert torch.equal(bx, by)


def test_extract_and_bake_run_in_one_captured_graph():
    """Capacity-mode extraction and the bake, no host synchronisation in either: captured once on one stream, replayed once, bitwise the eager result."""
    from forge_amd.geometry import bake_vertex_colors, extract_mesh
    dens, cam, images, v2v = _capacity_inputs()
    eager_mesh = extract_mesh(dens, max_vertices=320, max_faces=640)
    eager = bake_vertex_colors(eager_mesh, dens, images, cam, v2v)
    static = dens.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch = extract_mesh(static, max_vertices=320, max_faces=640)
        baked = bake_vertex_colors(batch, static, images, cam, v2v)
    g.replay()
    torch.cuda.synchronize()
    assert batch.counts.cpu().tolist() == [[302, 600], [0, 0]] and batch.status.cpu().tolist() == [0, 0]
    assert torch.equal(batch.vertices, eager_mesh.vertices)
    for x, y in zip(baked, eager):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert float(baked[1][0, :302].max()) > 0.5 and (baked[2][0, 302:] == -1).all()


def test_colored_mesh_is_the_hand_composed_chain():
    """colored_mesh = heads -> extract_mesh -> nvs.render_360 -> one bake over photographs (gain 1) and rendered views (gain render_gain), bit for
    bit. The model: a seeded VolRender at 64 x 64 and a heads stand-in that returns two blob volumes at 16^3."""
    from forge_amd import geometry, nvs, synthetic as syn
    from forge_amd.volume_render import VolRender
    dev = torch.device("cuda")
    cfg = syn.kubric_config(img_size=64, n_pts_per_ray=48)
    vr = VolRender(cfg)
    sd = syn.seeded_state_dict({"render." + k: v for k, v in vr.state_dict().items()}, 3)
    vr.load_state_dict({k[len("render."):]: v for k, v in sd.items()})
    vr = vr.to(dev).eval()
    feat, dens = (t.to(dev) for t in syn.blob_volumes(2, 16, 16, seed=31))

    class Heads:
        @staticmethod
        def heads(fused):
            return feat, dens

    class Model:
        render, encoder_3d = vr, Heads
    K = syn.intrinsics(64)
    t, n_views = 2, 8
    photos = torch.from_numpy(bc.random_images(2 * t, 3, 64, 64, 21)).reshape(2, t, 3, 64, 64).to(dev)
    pc = bc.pack(bc.orbit(2 * t, phase_deg=40.0, elev_deg=20.0), 64, 64)
    photo_cams = {"R": torch.from_numpy(pc[:, :9].reshape(-1, 3, 3).copy()), "T": torch.from_numpy(pc[:, 9:12].copy()), "K": K[None].repeat(2 * t, 1, 1)}
    meshes, extras = geometry.colored_mesh(Model, torch.zeros(2, 128, 8, 8, 8, device=dev), K, 1.5, photos=photos, photo_cameras=photo_cams, n_views=n_views,
                                           render_gain=0.05)
    # by hand
    plain = geometry.extract_mesh(dens)
    imgs, _ = nvs.render_360(Model, feat, dens, K, 1.5, n_views=n_views)
    R, T = nvs.nvs_cameras(1.5, n_views, dev)
    cams = {"R": torch.cat([photo_cams["R"].to(dev), R.repeat(2, 1, 1)]), "T": torch.cat([photo_cams["T"].to(dev), T.repeat(2, 1)]),
            "K": K.to(dev)[None].repeat(2 * (t + n_views), 1, 1)}
    v2v = torch.cat([torch.arange(2).repeat_interleave(t), torch.arange(2).repeat_interleave(n_views)]).to(dev, torch.int32)
    gain = torch.cat([torch.ones(2 * t), torch.full((2 * n_views,), 0.05)]).to(dev)
    want, wextras = geometry.bake_vertex_colors(plain, dens, torch.cat([photos.reshape(2 * t, 3, 64, 64), imgs.reshape(2 * n_views, 3, 64, 64)]), cams, v2v,
                                                view_gain=gain)
    for m, wm, (w, b), (ww, wb) in zip(meshes, want, extras, wextras):
        assert m.vertices.shape[0] > 500 and torch.equal(m.vertices, wm.vertices) and torch.equal(m.faces, wm.faces)
        assert torch.equal(m.colors.view(torch.int32), wm.colors.view(torch.int32)) and torch.equal(w, ww) and torch.equal(b, wb)
        assert int((b >= 2 * t).sum()) > 0 and int(((b >= 0) & (b < 2 * t)).sum()) > 0         # photographs and rendered views both win somewhere
        assert float(m.colors.min()) >= 0.0
