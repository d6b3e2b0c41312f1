"""GPU (-m gpu): the HIP path, called through the C-ABI (forge_amd/_lib.py -> libforge_hip.so),
against the CPU oracle and the committed golden vectors from the reference.

Stated fp32 tolerances (the op is trilinear interpolation / compositing of O(1) values):
  rotate fwd            max-abs 2e-5          render fwd   max-abs 2e-5 (features/opacity/depth)
  backward (vs autograd through the oracle)   max-abs 1e-4 relative to the gradient scale
  full forward vs oracle / reference golden   max-abs 2e-4 and PSNR > 95 dB (4e-4 / 90 dB against the reference's own output); measured 4.6e-5 / 110 dB
"""
import os

import numpy as np
import pytest
import torch

import forge_oracle as fo
from forge_amd import ops, synthetic as syn

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from forge_amd import _lib
    _lib.lib()          # fail loudly if libforge_hip.so is missing — no fallback
    return torch.device("cuda:0")


def assert_forward_close(imgs, oi, masks, om, tag, max_abs=2e-4, psnr=95.0, mask_abs=1e-4):
    """Full-forward bound against the oracle / the reference golden: ~4x what is measured (max-abs 4.6e-5, 110.5 dB on the
    bench scene; the round-4 bound of 2e-3 / 60 dB would have let a 50 dB regression pass). Relative to the image scale when the seeded
    conv_rgb emits intensities above 1 (its ReLU is unbounded above)."""
    imgs, masks = imgs.detach().cpu(), masks.detach().cpu()
    scale = max(1.0, oi.abs().max().item())
    e_i, e_m, p = (imgs - oi).abs().max().item() / scale, (masks - om).abs().max().item(), fo.psnr(imgs / scale, oi / scale)
    if os.environ.get("FORGE_TEST_REPORT"):
        print("  forward %-40s max-abs %.2e (scale %.2f)  mask %.2e  PSNR %.1f dB" % (tag, e_i, scale, e_m, p))
    assert e_i < max_abs and p > psnr and e_m < mask_abs, (tag, e_i, p, e_m)


def _cam_pack(R, Tt, Kh):
    V = R.shape[0]
    return torch.cat([R.reshape(V, 9), Tt.reshape(V, 3), Kh[:, 0, 0:1], Kh[:, 1, 1:2], Kh[:, 0, 2:3], Kh[:, 1, 2:3]], dim=1)


# ------------------------------------------------------------------ rotate
def test_rotate_golden_d16(dev, golden):
    from forge_amd.rotate import Rotate_world
    g = golden("rotate_d16")
    rot = Rotate_world(syn.kubric_config()).to(dev)
    out = rot(T(g["voxels"]).to(dev), T(g["poses"]).to(dev), grid_size=16).cpu()
    assert torch.equal(out[:, 0], T(g["voxels"])[:, 0])
    assert (out - T(g["out"])).abs().max().item() < 2e-5


def test_rotate_identity_quirk_d32(dev, golden):
    from forge_amd.rotate import Rotate_world
    g = golden("rotate_identity_d32")
    rot = Rotate_world(syn.kubric_config()).to(dev)
    vox = T(g["voxels"]).repeat(1, 1, 4, 1, 1, 1)          # C=4 (kernel needs C % 4 == 0)
    out = rot(vox.to(dev), T(g["poses"]).to(dev), grid_size=32).cpu()
    assert (out[:, :, :1] - T(g["out"])).abs().max().item() < 2e-5
    assert (out[:, 1] - vox[:, 1]).abs().max().item() > 0.3      # identity pose is NOT an identity resample


@pytest.mark.parametrize("D,C,B,t", [(16, 8, 2, 3), (32, 128, 1, 5), (48, 4, 1, 2), (64, 16, 1, 2), (128, 4, 1, 2)])    # every grid of models/rotate.py:18-35
def test_rotate_vs_oracle(dev, D, C, B, t):
    from forge_amd.rotate import Rotate_world
    g = torch.Generator().manual_seed(D + C)
    jit = (torch.rand(10, 2, generator=g) - 0.5) * 0.4
    poses, _, _ = syn.orbit_cameras(10, 1.5, 20.0, jit)
    P = torch.stack([poses[torch.randperm(10, generator=g)[:t]] for _ in range(B)])
    vox = torch.randn(B, t, C, D, D, D, generator=g)
    ref = fo.rotate_world(vox, P, 1.0)
    out = Rotate_world(syn.kubric_config()).to(dev)(vox.to(dev), P.to(dev), grid_size=D).cpu()
    assert out.shape == ref.shape
    # the un-normalised coordinate ((s + 1) D - 1) / 2 is rounded at magnitude 2 D: its ulp (2^-23 x 2 D: 1.5e-5 of a voxel at D = 128) moves a
    # trilinear weight by as much, whichever fp32 implementation computes it - the bound scales with D beyond 64
    tol = max(2e-5, 3.0 * D * 2.0 ** -23)
    assert (out - ref).abs().max().item() < tol * max(1.0, ref.abs().max().item())


def test_rotate_layout_agnostic_and_far_pose(dev):
    """plain-contiguous NCDHW input and channels-last input give the same answer; a pose that throws the
    volume completely out of the grid gives exact zeros (zeros padding)."""
    from forge_amd.rotate import Rotate_world
    rot = Rotate_world(syn.kubric_config()).to(dev)
    vox = torch.randn(1, 2, 8, 16, 16, 16, device=dev)
    P = torch.eye(4, device=dev)[None, None].repeat(1, 2, 1, 1)
    P[0, 1, :3, 3] = torch.tensor([5.0, 0, 0])
    a = rot(vox, P, grid_size=16)
    vox_cl = vox.reshape(2, 8, 16, 16, 16).contiguous(memory_format=torch.channels_last_3d).reshape(1, 2, 8, 16, 16, 16)
    b = rot(vox_cl, P, grid_size=16)
    assert torch.equal(a, b)
    assert a[:, 1].abs().max().item() == 0.0
    with pytest.raises(ValueError):
        rot(torch.zeros(1, 2, 4, 20, 20, 20, device=dev), P, grid_size=20)


def test_rotate_backward_vs_oracle_autograd(dev):
    from forge_amd.rotate import Rotate_world
    g = torch.Generator().manual_seed(3)
    poses, _, _ = syn.orbit_cameras(5, 1.5, 15.0)
    P = poses[None, :3].contiguous()
    vox = torch.randn(1, 3, 8, 16, 16, 16, generator=g)
    wgt = torch.randn(1, 3, 8, 16, 16, 16, generator=g)
    v_ref = vox.clone().requires_grad_(True)
    P_ref = P.clone().requires_grad_(True)
    (fo.rotate_world(v_ref, P_ref, 1.0) * wgt).sum().backward()
    v = vox.to(dev).requires_grad_(True)
    Pd = P.to(dev).requires_grad_(True)
    (Rotate_world(syn.kubric_config()).to(dev)(v, Pd, grid_size=16) * wgt.to(dev)).sum().backward()
    scale = v_ref.grad.abs().max().item()
    assert (v.grad.cpu() - v_ref.grad).abs().max().item() < 1e-4 * scale
    pscale = P_ref.grad.abs().max().item()
    assert (Pd.grad.cpu() - P_ref.grad).abs().max().item() < 2e-3 * pscale      # pose gradient (row f2)


# ------------------------------------------------------------------ render
def _render_hip(dev, feat, dens, R, Tt, Kh, Hr, Wr, S, zmin, zmax, vol, depth=True, view2vol=None):
    nvol, C, D, H, W = feat.shape
    V = R.shape[0]
    v2v = torch.arange(V, dtype=torch.int32) if view2vol is None else view2vol
    h = [0.5 * (n - 1) * vol / D for n in (W, H, D)]
    outs = ops.render_rays(feat.to(dev), dens.to(dev), _cam_pack(R, Tt, Kh).to(dev), v2v.to(dev), Hr, Wr, S, zmin, zmax, h, depth)
    return torch.cat(outs, dim=1).permute(0, 2, 3, 1).cpu()          # [V,Hr,Wr,C+1(+1)] like pytorch3d


def test_render_golden_raw(dev, golden):
    g = golden("render_d16")
    feat, dens, R, Tt, K = (T(g[k]) for k in ("feat", "dens", "R", "T", "K"))
    S, img = int(g["n_pts"]), int(g["img_size"])
    got = _render_hip(dev, feat, dens, R, Tt, fo.halve_intrinsics(K), img // 2, img // 2, S,
                      float(g["min_depth"]), float(g["max_depth"]), float(g["vol_size"]))
    assert (got - T(g["raw"])).abs().max().item() < 2e-5


def test_volrender_module_golden(dev, golden):
    """VolRender.forward incl. conv_rgb / upsampling / origin projection vs the reference module's outputs."""
    from forge_amd.volume_render import VolRender
    g = golden("render_d16")
    cfg = syn.kubric_config(img_size=int(g["img_size"]), n_pts_per_ray=int(g["n_pts"]))
    vr = VolRender(cfg)
    vr.load_state_dict({k[len("w.render."):]: T(g[k]) for k in g.files if k.startswith("w.render.")})
    vr = vr.to(dev).eval()
    K = T(g["K"]).to(dev)
    K_before = K.clone()
    cam = {"R": T(g["R"]).to(dev), "T": T(g["T"]).to(dev), "K": K}
    with torch.no_grad():
        imgs, sil, depth, oproj = vr(cam, T(g["feat"]).to(dev), T(g["dens"]).to(dev), render_depth=True, return_origin_proj=True)
    assert torch.equal(K, K_before)                                 # no in-place halving of the caller's K
    assert (imgs.cpu() - T(g["imgs"])).abs().max().item() < 1e-4
    assert (sil.cpu() - T(g["sil"])).abs().max().item() < 2e-5
    assert (depth.cpu() - T(g["depth"])).abs().max().item() < 2e-5
    assert (oproj.cpu() - T(g["origin_proj"])).abs().max().item() < 1e-3
    with torch.no_grad():
        two = vr(cam, T(g["feat"]).to(dev), T(g["dens"]).to(dev))
    assert len(two) == 2 and torch.equal(two[0], imgs)


@pytest.mark.parametrize("D,C,img,S", [(32, 16, 128, 64), (64, 16, 256, 64), (16, 4, 64, 33), (24, 32, 40, 17), (16, 8, 64, 200)])
def test_render_vs_oracle(dev, D, C, img, S):
    feat, dens = syn.blob_volumes(2, D, C, seed=D)
    _, extr, _ = syn.orbit_cameras(10, 1.5, 15.0)
    E = extr[[0, 3, 6]].clone()
    E[2, 1, 3] -= 0.3
    Kh = fo.halve_intrinsics(syn.intrinsics(img)[None].repeat(3, 1, 1))
    v2v = torch.tensor([0, 1, 1], dtype=torch.int32)
    ref = fo.render_rays(feat[v2v.long()], dens[v2v.long()], E[:, :3, :3], E[:, :3, 3], Kh, img // 2, img // 2, S, 0.5, 2.0, 1.0, True)
    got = _render_hip(dev, feat, dens, E[:, :3, :3], E[:, :3, 3], Kh, img // 2, img // 2, S, 0.5, 2.0, 1.0, view2vol=v2v)
    assert (got - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


def test_render_edge_cases(dev):
    """all rays miss the volume -> exact zeros; density exactly 1 somewhere -> T hits 0 exactly (early-out
    path) and still matches; densities > 1 (negative transmittance) match; non-square render target."""
    D, C = 16, 16
    feat = torch.randn(1, C, D, D, D)
    dens = torch.zeros(1, 1, D, D, D)
    dens[0, 0, 6:10, 6:10, 6:10] = 1.0          # interior voxels with d == 1 exactly
    dens[0, 0, 2:4] = 1.7
    E = syn.SyntheticDataset(1.5).get_canonical_extrinsics_cv2()[None].clone()
    Kh = fo.halve_intrinsics(syn.intrinsics(64)[None])
    ref = fo.render_rays(feat, dens, E[:, :3, :3], E[:, :3, 3], Kh, 32, 32, 64, 0.5, 2.0, 1.0, True)
    got = _render_hip(dev, feat, dens, E[:, :3, :3], E[:, :3, 3], Kh, 32, 32, 64, 0.5, 2.0, 1.0)
    assert (got - ref).abs().max().item() < 3e-5 * max(1.0, ref.abs().max().item())
    far = E.clone()
    far[0, 0, 3] = 10.0
    got = _render_hip(dev, feat, dens, far[:, :3, :3], far[:, :3, 3], Kh, 32, 32, 64, 0.5, 2.0, 1.0)
    assert got.abs().max().item() == 0.0
    # non-square, odd sizes
    ref = fo.render_rays(feat, dens, E[:, :3, :3], E[:, :3, 3], Kh, 19, 37, 31, 0.5, 2.0, 1.0, False)
    got = _render_hip(dev, feat, dens, E[:, :3, :3], E[:, :3, 3], Kh, 19, 37, 31, 0.5, 2.0, 1.0, depth=False)
    assert got.shape == ref.shape and (got - ref).abs().max().item() < 3e-5 * max(1.0, ref.abs().max().item())


def test_render_backward_vs_oracle_autograd(dev):
    D, C, img, S = 16, 16, 48, 40
    feat, dens = syn.blob_volumes(2, D, C, seed=11)
    dens[0, 0, 7:9, 7:9, 7:9] = 1.0              # exact-zero transmittance inside the march
    _, extr, _ = syn.orbit_cameras(10, 1.5, 15.0)
    E = extr[[1, 4, 8]]
    Kh = fo.halve_intrinsics(syn.intrinsics(img)[None].repeat(3, 1, 1))
    v2v = torch.tensor([0, 1, 0], dtype=torch.int32)
    Hr = img // 2
    g = torch.Generator().manual_seed(5)
    wgt = torch.randn(3, Hr, Hr, C + 2, generator=g)
    f_ref = feat.clone().requires_grad_(True)
    d_ref = dens.clone().requires_grad_(True)
    ref = fo.render_rays(f_ref[v2v.long()], d_ref[v2v.long()], E[:, :3, :3], E[:, :3, 3], Kh, Hr, Hr, S, 0.5, 2.0, 1.0, True)
    (ref * wgt).sum().backward()
    f = feat.to(dev).requires_grad_(True)
    d = dens.to(dev).requires_grad_(True)
    h = [fo.grid_half_extent(D, 1.0)] * 3
    outs = ops.render_rays(f, d, _cam_pack(E[:, :3, :3], E[:, :3, 3], Kh).to(dev), v2v.to(dev), Hr, Hr, S, 0.5, 2.0, h, True)
    got = torch.cat(outs, dim=1).permute(0, 2, 3, 1)
    (got * wgt.to(dev)).sum().backward()
    assert (got.detach().cpu() - ref.detach()).abs().max().item() < 3e-5 * max(1.0, ref.abs().max().item())
    fs, ds = f_ref.grad.abs().max().item(), d_ref.grad.abs().max().item()
    assert (f.grad.cpu() - f_ref.grad).abs().max().item() < 1e-4 * fs
    assert (d.grad.cpu() - d_ref.grad).abs().max().item() < 1e-4 * ds


def test_layout_helpers(dev):
    from forge_amd import _lib
    x = torch.randn(2, 12, 5, 6, 7, device=dev)
    y = torch.empty(2, 5, 6, 7, 12, device=dev)
    _lib.check(_lib.lib().forge_ncdhw_to_ndhwc(_lib.ptr(x), _lib.ptr(y), 2, 12, 5 * 6 * 7, _lib.current_stream()), "to_ndhwc")
    assert torch.equal(y, x.permute(0, 2, 3, 4, 1).contiguous())
    z = torch.empty_like(x)
    _lib.check(_lib.lib().forge_ndhwc_to_ncdhw(_lib.ptr(y), _lib.ptr(z), 2, 12, 5 * 6 * 7, _lib.current_stream()), "to_ncdhw")
    assert torch.equal(z, x)


# ------------------------------------------------------------------ whole model
def test_forward_pose3d_golden_and_oracle(dev, golden):
    """FORGE_poseEstimator3D gt-pose forward at reference shapes (5x256^2 in, 10 views out, 32^3/64^3 grids)
    vs the reference model's own output (golden, subsampled)."""
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    g = golden("forward_pose3d")
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), int(g["weight_seed"])))
    model = model.to(dev).eval()
    sample = syn.make_sample(1, 5, 256, 1.5, seed=int(g["sample_seed"]))
    K_before = sample["K_cv2"].clone()
    with torch.no_grad():
        imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
    assert torch.equal(sample["K_cv2"], K_before)
    imgs, masks = imgs.cpu(), masks.cpu()
    ref_i, ref_m = T(g["imgs_sub"]), T(g["masks_sub"])
    # against the REFERENCE's own output (the oracle sits 8.7e-5 / 1e-5 from it): 4e-4 / 90 dB
    assert_forward_close(imgs[:, :, ::4, ::4], ref_i, masks[:, :, ::4, ::4], ref_m, "pose3d vs reference golden", max_abs=4e-4, psnr=90.0, mask_abs=2e-4)
    assert (imgs.mean(dim=(1, 2, 3)) - T(g["imgs_mean"])).abs().max().item() < 1e-4


def test_forge_gt_pose_5in5out_vs_oracle(dev):
    """The bench configuration: FORGE, GT poses, 5 input views -> 1 fusion -> 5 rendered views."""
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    w = syn.seeded_state_dict(model.state_dict(), 0)
    model.load_state_dict(w)
    model = model.to(dev).eval()
    sample = syn.make_sample(1, 5, 256, 1.5, seed=2)
    with torch.no_grad():
        imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
        oi, om = fo.forward_hot_path(sample["images"], sample["cam_poses_cv2_canonicalized"],
                                     sample["cam_extrinsics_cv2_canonicalized"], sample["K_cv2"], w, cfg,
                                     order_by_distance=True)
    assert imgs.shape == (5, 3, 256, 256)
    assert_forward_close(imgs, oi, masks, om, "FORGE 5-in / 5-out (bench scene family)")


@pytest.mark.parametrize("t", [1, 2, 3])
def test_forge_ragged_view_counts_vs_oracle(dev, t):
    """fewer input views than the training configuration (t = 1: the fusion GRU runs a single step on the un-warped reference view;
    t = 2, 3: `demo.py` style few-view inputs): same kernels, different sequence lengths / launch plans."""
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    w = syn.seeded_state_dict(model.state_dict(), 0)
    model.load_state_dict(w)
    model = model.to(dev).eval()
    sample = syn.make_sample(1, t, 256, 1.5, seed=20 + t)
    with torch.no_grad():
        imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
        oi, om = fo.forward_hot_path(sample["images"], sample["cam_poses_cv2_canonicalized"],
                                     sample["cam_extrinsics_cv2_canonicalized"], sample["K_cv2"], w, cfg,
                                     order_by_distance=True)
    assert imgs.shape == (t, 3, 256, 256)
    assert_forward_close(imgs, oi, masks, om, "FORGE t = %d input views" % t)


def test_forge_non_default_render_config_vs_oracle(dev):
    """the config surface the model reads (config/config.py: render.{volume_size, n_pts_per_ray, min_depth, max_depth, k_size}): a
    non-default combination - 48 samples on [0.7, 2.3], a 1.2-unit volume, 3x3 conv_rgb kernels (ConvTranspose2d k=4, p=1)."""
    from forge_amd.model import FORGE
    cfg = syn.kubric_config(volume_size=1.2, n_pts_per_ray=48, min_depth=0.7, max_depth=2.3)
    cfg.render.k_size = 3
    model = FORGE(cfg)
    w = syn.seeded_state_dict(model.state_dict(), 5)
    model.load_state_dict(w)
    model = model.to(dev).eval()
    sample = syn.make_sample(1, 4, 256, 1.5, seed=31)
    with torch.no_grad():
        imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
        oi, om = fo.forward_hot_path(sample["images"], sample["cam_poses_cv2_canonicalized"],
                                     sample["cam_extrinsics_cv2_canonicalized"], sample["K_cv2"], w, cfg,
                                     order_by_distance=True)
    assert imgs.shape == (4, 3, 256, 256)
    assert_forward_close(imgs, oi, masks, om, "FORGE non-default render config")


def test_fuse_groups_shared_inputs_equals_separate_fusions(dev):
    """FORGE_poseEstimator3D's three fusions (views (0,1,2), (3,4), (0..4) of the same rotated features) with the input halves of the GRU
    convolutions computed once per view (fuse_groups_autograd_hip) against three independent fuse_autograd_hip calls: outputs, input
    gradient and parameter gradients. Stated tolerance: 2e-4 of the respective max magnitude (fp32 summation order, atomics in wgrad)."""
    # Seed: the two paths order their fp32 sums differently (K = 3 x 128 halves + residual vs K = 3 x 256), so a LeakyReLU argument of
    # fusion_conv that lies within rounding of zero can take the other slope in one of them; that single activation then moves its 5^3
    # neighbourhood of dx and the fusion_conv weight gradients by ~1e-3 of their max - a property of LeakyReLU, not of either path.
    # tools/debug/groups_grad_noise.py lists the agreement per seed (8e-7 relative L2 without such an event, 2e-4 with one: seed 11 on
    # the Winograd kernels); this seed has none on either kernel family, so the tight bounds below test the arithmetic.
    _groups_vs_separate_fusions_autograd(dev, 1, 128, 12)


def test_fuse_groups_shared_inputs_equals_separate_fusions_8_plane_form(dev):
    """The same comparison and bounds at 2 scenes = 2048 tile rows per GRU step, where every point GEMM of the hand-scheduled node takes the
    8-plane form (convops.wino_half_applies). (Training needs C a multiple of 128: the weight gradients of the two-input convolutions.)
    The seed has no LeakyReLU sign flip, as above."""
    from forge_amd import convops as co
    assert co.wino_half_applies(2 * 16 * 8 * 8, 256, 128) and co.wino_half_applies(2 * 16 * 8 * 8, 128, 128)
    _groups_vs_separate_fusions_autograd(dev, 2, 128, 12)


def _groups_vs_separate_fusions_autograd(dev, b, C, seed):
    import copy
    from forge_amd.fusion import ConvGRU_3D
    torch.manual_seed(seed)
    a = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=C, hidden_size=C).to(dev).train()
    bmod = copy.deepcopy(a)
    x = (torch.randn(b, 5, C, 16, 16, 16) * 0.5).to(dev)
    groups = [[0, 1, 2], [3, 4], [0, 1, 2, 3, 4]]
    ws = [torch.randn(b, C, 16, 16, 16, device=dev) for _ in groups]
    xa = x.clone().requires_grad_(True)
    outs_a = a.fuse_groups_autograd_hip(xa, groups)
    sum((o * w).sum() for o, w in zip(outs_a, ws)).backward()
    xb = x.clone().requires_grad_(True)
    outs_b = [bmod.fuse_autograd_hip(xb[:, g]) for g in groups]
    sum((o * w).sum() for o, w in zip(outs_b, ws)).backward()
    rel = lambda u, v: (u - v).abs().max().item() / max(v.abs().max().item(), 1e-6)
    for oa, ob in zip(outs_a, outs_b):
        assert rel(oa.detach(), ob.detach()) < 2e-4
    assert rel(xa.grad, xb.grad) < 2e-4
    gscale = max(p.grad.abs().max().item() for p in bmod.parameters() if p.grad is not None)
    for (k, pa), (_, pb) in zip(a.named_parameters(), bmod.named_parameters()):
        assert (pa.grad - pb.grad).abs().max().item() < 3e-4 * max(pb.grad.abs().max().item(), 1e-2 * gscale), k


def test_conv_launcher_batch_chunking_is_exact(dev, monkeypatch):
    """operands beyond the kernel's 2 GiB buffer-offset range are launched in batch chunks (convops.conv_igemm): with the limit lowered
    so that a 6-scene batch splits into chunks of 2, 1-scene ... the fused-GRU, residual and lifted epilogues must give bit-identical
    results to the single launch."""
    from forge_amd import convops as co
    from forge_amd.fusion import ConvGRU_3D
    torch.manual_seed(5)
    monkeypatch.setattr(co.STATE, "winograd", False)            # the direct implicit-GEMM launcher is what chunks; the Winograd path falls back to it
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=128, hidden_size=128).to(dev).eval()
    x = (torch.randn(6, 3, 128, 8, 8, 8) * 0.5).to(dev)
    with torch.no_grad():
        ref = gru.fuse_hip(x).clone()
        monkeypatch.setattr(co, "MAX_OPERAND_BYTES", 3 * 8 * 8 * 8 * 128 * 4 * 2)          # two scenes' worth of the [b,t,...] input
        chunked = gru.fuse_hip(x)
        assert torch.equal(ref, chunked)
        # the Winograd path splits the batch into scene chunks whose transformed operands fit (convops.wino_scene_chunk): bit-identical too
        monkeypatch.setattr(co.STATE, "winograd", True)
        monkeypatch.setattr(co, "MAX_OPERAND_BYTES", (1 << 31) - 1)
        wref = gru.fuse_hip(x).clone()
        monkeypatch.setattr(co, "MAX_OPERAND_BYTES", 2 * 3 * 8 * 4 * 4 * 128 * 4)          # two scenes' worth of V_x per Winograd point
        assert co.wino_scene_chunk(6, 8, 8, 8, 128, views=3) == 2
        assert torch.equal(gru.fuse_hip(x), wref)
        assert (wref - ref).abs().max().item() < 2e-5


def test_training_loss_and_gradients_vs_oracle_autograd(dev):
    """End-to-end pin of the TRAINING path: FORGE_poseEstimator3D in train mode (BatchNorm batch statistics, three fusions, heads
    batched as the reference batches them), loss = 5 MSE(rgb) + MSE(mask), against autograd through the CPU oracle (training=True) on
    the same sample and weights: loss value, and the gradient of parameters from every stage. Stated tolerance: 1e-2 of each gradient's max
    magnitude (1.5e-2 on the ResNet trunk's parameters) and a per-layer cosine >= 0.99995 - see test_training_gradients_vs_reference_golden."""
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    w = syn.seeded_state_dict(model.state_dict(), 0)
    model.load_state_dict(w)
    model = model.to(dev).train()
    sample = syn.make_sample(1, 5, 256, 1.5, seed=4)
    tgt_i = sample["images"][0].repeat(2, 1, 1, 1)
    tgt_m = sample["fg_probabilities"][0].repeat(2, 1, 1, 1)
    imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
    loss = 5.0 * torch.nn.functional.mse_loss(imgs, tgt_i.to(dev)) + torch.nn.functional.mse_loss(masks, tgt_m.to(dev))
    loss.backward()
    keys = ["encoder_3d.feature_extraction.0.weight", "encoder_3d.feature_extraction.6.2.conv2.weight", "encoder_3d.conv1.0.weight",
            "encoder_3d.fusion_feature.cells.0.conv_gate.weight", "encoder_3d.fusion_feature.cells.0.out_gate.bias",
            "encoder_3d.fusion_feature.fusion_conv.3.weight", "encoder_3d.fusion_feature.fusion_norm.weight",
            "encoder_3d.features_head.0.weight", "encoder_3d.density_head.3.weight", "encoder_3d.density_head.6.weight",
            "render.conv_rgb.0.weight", "render.conv_rgb.3.weight", "render.conv_rgb.6.bias"]
    wo = {k: (v.clone().requires_grad_(True) if k in keys else v.clone()) for k, v in w.items()}
    oi, om = fo.forward_pose3d_gt(sample, wo, cfg, training=True)
    lo = 5.0 * torch.nn.functional.mse_loss(oi, tgt_i) + torch.nn.functional.mse_loss(om, tgt_m)
    lo.backward()
    assert abs(loss.item() - lo.item()) < 1e-4 * max(1.0, abs(lo.item()))
    named = dict(model.named_parameters())
    for k in keys:
        ref, got = wo[k].grad, named[k].grad.cpu()
        err = (got - ref).abs().max().item()
        tol = 1.5e-2 if "feature_extraction" in k else 1e-2       # as in test_training_gradients_vs_reference_golden
        assert err < tol * ref.abs().max().item() + 1e-9, (k, err, ref.abs().max().item())
        if ref.numel() > 1:                          # per-layer direction check (see test_training_gradients_vs_reference_golden)
            cos = torch.nn.functional.cosine_similarity(got.double().flatten(), ref.double().flatten(), dim=0).item()
            assert cos > 0.99995, (k, cos)


def test_training_gradients_vs_reference_golden(dev, golden):
    """The HIP training path against the REFERENCE's own training run (tests/golden/train_pose3d.npz: loss and gradients produced by
    models/model_single_pose_estimator.py FORGE_poseEstimator3D.train() + backward in the build container)."""
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    gold = golden("train_pose3d")
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), int(gold["weight_seed"])))
    model = model.to(dev).train()
    sample = syn.make_sample(1, 5, 256, 1.5, seed=int(gold["sample_seed"]))
    tgt_i = sample["images"][0].repeat(2, 1, 1, 1).to(dev)
    tgt_m = sample["fg_probabilities"][0].repeat(2, 1, 1, 1).to(dev)
    imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
    loss = 5.0 * torch.nn.functional.mse_loss(imgs, tgt_i) + torch.nn.functional.mse_loss(masks, tgt_m)
    loss.backward()
    assert abs(loss.item() - float(gold["loss"])) < 1e-4 * abs(float(gold["loss"]))
    assert (imgs.detach()[:, :, ::16, ::16].cpu() - torch.from_numpy(gold["imgs_sub"])).abs().max().item() < 2e-3
    keys = [k[len("grad__"):] for k in gold.files if k.startswith("grad__")]
    gscale = max(float(np.abs(gold["grad__" + k]).max()) for k in keys)
    named = dict(model.named_parameters())
    for k in keys:
        ref = torch.from_numpy(gold["grad__" + k])
        err = (named[k].grad.cpu() - ref).abs().max().item()
        # Round 4: the step's own run-to-run distance is now <= 1.1e-6 of each gradient's max (the ray-march backward is a deterministic gather;
        # what is left are the fp32 atomics of the weight-gradient split-K: tools/debug/train_grad_margins.py), so the bound is no longer a noise
        # floor of this build but the distance between two fp32 evaluations of the graph: measured against this golden 2.4e-4 ... 2.9e-3 outside
        # the trunk, 6.6e-3 / 1.2e-2 on the trunk's first convolution / last BatchNorm weight - where the reference's own fp32 gradients sit
        # 0.3-1.6e-2 from a float64 evaluation (53 train-mode BatchNorm layers over a batch of 5; tools/debug/feat3d_train_noise.py).
        tol = 1.5e-2 if "feature_extraction" in k else 1e-2
        assert err < tol * max(ref.abs().max().item(), 1e-3 * gscale), (k, err, ref.abs().max().item())
        # direction check per layer: a max-norm band cannot see a gradient that is wrong by a percent everywhere, the cosine can
        # (0.99995 <=> 1 % relative L2; measured 1 - cos <= 3.8e-5). Tensors whose gradient is pure cancellation noise (|g| < 1e-3 of the
        # largest gradient: biases in front of a BatchNorm) are not direction-checked.
        if ref.numel() > 1 and ref.abs().max().item() > 1e-3 * gscale:
            cos = torch.nn.functional.cosine_similarity(named[k].grad.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
            assert cos > 0.99995, (k, cos)


@pytest.mark.parametrize("path,factor", [("winograd", 4.0), ("direct", 1.5)])
def test_training_gradients_vs_float64_reference(dev, golden, path, factor):
    """the GT-pose training step against the REFERENCE's float64 evaluation of the same graph (train_pose3d.npz grad64__*,
    oracle/make_golden.py::train_goldens), per golden key, relative to how far the reference's own fp32 run sits from that float64 result
    (0.8-4e-3 of max on the trunk, 1e-4 .. 1e-3 elsewhere):
        direct    (convops.winograd(False): implicit-GEMM launches only)   err(HIP, f64) <= 1.5 x err(ref fp32, f64) + 3e-4   measured <= 1.37x
                  on the trunk, <= 1.7x elsewhere where the floor does not carry it
        winograd  (the default path: F(2x2,3x3) point GEMMs in the fusion, conv1 and layer3/4 forward, data and weight gradients)   <= 4 x ... + 3e-4
                  measured 1.5-3.2x: the transforms' rounding amplification, the price of 2.25x fewer multiplies (profiles/r05_train_grad_margins.txt)
    The reference's own GPU runs are cuDNN TF32 (kubric_train_pose_3D.py:119-124, torch 1.10 defaults): 10-bit mantissas, two orders noisier."""
    from forge_amd import convops as co
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    from test_gpu_configs import check_gradients_vs_float64_golden
    gold = golden("train_pose3d")
    cfg = syn.kubric_config()
    with co.winograd(path == "winograd"):
        model = FORGE_poseEstimator3D(cfg)
        model.load_state_dict(syn.seeded_state_dict(model.state_dict(), int(gold["weight_seed"])))
        model = model.to(dev).train()
        sample = syn.make_sample(1, 5, 256, 1.5, seed=int(gold["sample_seed"]))
        tgt_i = sample["images"][0].repeat(2, 1, 1, 1).to(dev)
        tgt_m = sample["fg_probabilities"][0].repeat(2, 1, 1, 1).to(dev)
        imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
        loss = 5.0 * torch.nn.functional.mse_loss(imgs, tgt_i) + torch.nn.functional.mse_loss(masks, tgt_m)
        loss.backward()
        torch.cuda.synchronize()
    assert abs(loss.item() - float(gold["loss64"])) < 2e-6 * abs(float(gold["loss64"])), (loss.item(), float(gold["loss64"]))
    assert check_gradients_vs_float64_golden(gold, dict(model.named_parameters()), factor=factor) >= 16


def test_training_step_runs(dev):
    """fwd + bwd + Adam through the HIP ops in train mode (BN batch stats), loss finite and decreasing grads exist."""
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    sample = syn.make_sample(1, 5, 256, 1.5, seed=4)
    imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
    tgt_i = sample["images"][0].repeat(2, 1, 1, 1).to(dev)
    tgt_m = sample["fg_probabilities"][0].repeat(2, 1, 1, 1).to(dev)
    loss = 5.0 * torch.nn.functional.mse_loss(imgs, tgt_i) + torch.nn.functional.mse_loss(masks, tgt_m)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
    opt.step()
    assert torch.isfinite(loss)
    g = model.encoder_3d.fusion_feature.cells[0].conv_gate.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0
    g0 = model.encoder_3d.feature_extraction[0].weight.grad
    assert g0 is not None and torch.isfinite(g0).all() and g0.abs().max().item() > 0      # the gradient reaches the image encoder


# ------------------------------------------------------------------ fp32-MFMA implicit-GEMM convolution
def _rows(x):      # [N,C,D,H,W] -> channels-last rows [N,D,H,W,C]
    return x.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("Cin,Cout,dims", [(64, 96, (6, 7, 5)), (32, 16, (5, 4, 9)), (128, 256, (4, 4, 4))])
def test_conv_igemm_plain_vs_conv3d(dev, Cin, Cout, dims):
    """stated tolerance: 2e-5 * sqrt(K/1000) * |out|max (fp32 accumulation-order differences only)"""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(Cin + Cout)
    D, H, W = dims
    x = torch.randn(2, Cin, D, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g)
    ref = torch.nn.functional.conv3d(x, w, b, padding=1)
    out = torch.empty(2, D, H, W, Cout, device=dev)
    co.conv_igemm(_rows(x).to(dev), Cin, Cin, None, 0, 0, co.pack_conv3d_weight(w).to(dev), b.to(dev), None, None, 1.0,
                  None, None, None, out, None, (2, D, H, W), (D, H, W), Cout, Cout, co.TAPS_3x3x3, epilogue=co.EPI_BIAS)
    got = out.permute(0, 4, 1, 2, 3).cpu()
    tol = 2e-5 * max(1.0, (27 * Cin / 1000) ** 0.5) * ref.abs().max().item()
    assert (got - ref).abs().max().item() < tol


def test_conv_igemm_concat_affine_residual(dev):
    """two channel-concatenated inputs (the cat([x,h]) of the GRU), folded BN + LeakyReLU + residual epilogue."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(1)
    x1, x2 = torch.randn(1, 32, 5, 6, 7, generator=g), torch.randn(1, 64, 5, 6, 7, generator=g)
    w = torch.randn(48, 96, 3, 3, 3, generator=g) / 50
    b, sc, sh = torch.randn(48, generator=g), torch.rand(48, generator=g) + 0.5, torch.randn(48, generator=g)
    res = torch.randn(1, 48, 5, 6, 7, generator=g)
    ref = torch.nn.functional.conv3d(torch.cat([x1, x2], 1), w, b, padding=1) * sc[None, :, None, None, None] + sh[None, :, None, None, None] + res
    ref = torch.nn.functional.leaky_relu(ref, 0.01)
    out = torch.empty(1, 5, 6, 7, 48, device=dev)
    co.conv_igemm(_rows(x1).to(dev), 32, 32, _rows(x2).to(dev), 64, 64, co.pack_conv3d_weight(w).to(dev), b.to(dev), sc.to(dev),
                  sh.to(dev), 0.01, _rows(res).to(dev), None, None, out, None, (1, 5, 6, 7), (5, 6, 7), 48, 48, co.TAPS_3x3x3,
                  epilogue=co.EPI_AFFINE_ACT)
    assert (out.permute(0, 4, 1, 2, 3).cpu() - ref).abs().max().item() < 5e-5 * ref.abs().max().item()


@pytest.mark.parametrize("tile", list("ABCDE"))
def test_conv_igemm_every_tile_and_splitk(dev, tile, monkeypatch):
    """every workgroup tile x split-K factor of the launch plan (forced through the experiment overrides) on a ragged problem
    (M = 630 rows, Cout = 96: partial tiles in both directions) with the folded-BN + residual + LeakyReLU epilogue."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(7)
    Cin, Cout, dims = 64, 96, (5, 7, 9)
    x = torch.randn(2, Cin, *dims, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    b, sc, sh = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    res = torch.randn(2, Cout, *dims, generator=g)
    bc = lambda v: v[None, :, None, None, None]
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv3d(x, w, b, padding=1) * bc(sc) + bc(sh) + res, 0.01)
    xd, wd, rd = _rows(x).to(dev), co.pack_conv3d_weight(w).to(dev), _rows(res).to(dev)
    M = 2 * dims[0] * dims[1] * dims[2]
    seen = 0
    for k in (1, 2, 3, 4, 6):
        monkeypatch.setattr(co.STATE, "plan_override", (tile, k))
        if co.conv_plan(M, Cout, Cin, 27, co.EPI_AFFINE_ACT, Cout) != (tile, k):
            continue
        seen += 1
        out = torch.full((2, *dims, Cout), float("nan"), device=dev)
        co.conv_igemm(xd, Cin, Cin, None, 0, 0, wd, b.to(dev), sc.to(dev), sh.to(dev), 0.01, rd, None, None, out, None,
                      (2, *dims), dims, Cout, Cout, co.TAPS_3x3x3, epilogue=co.EPI_AFFINE_ACT)
        err = (out.permute(0, 4, 1, 2, 3).cpu() - ref).abs().max().item()
        assert err < 5e-5 * ref.abs().max().item(), (tile, k, err)
    assert seen >= 4


def test_lds_dma_staging_short_k_and_ragged_edges(dev):
    """the K loop stages its operands by LDS-DMA (`buffer_load ... lds`, csrc/conv_igemm.hip): K slices of ONE and TWO steps (the pipeline's
    prologue-only cases), two concatenated inputs, ragged rows and columns (out-of-range lanes must land as zeros in LDS), on every tile,
    against a float64 reference of the same sums; and all tiles agree with each other to fp32 summation-order noise."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(11)
    for (B, D, C1, C2, Cout, taps, ks) in ((1, 10, 32, 0, 40, ((0, 0, 0),), 1), (1, 6, 64, 0, 72, ((0, 0, 0),), 1), (1, 6, 64, 0, 72, ((0, 0, 0),), 2),
                                          (3, 5, 32, 32, 130, ((0, 0, -1), (0, 0, 0), (0, 0, 1)), 1), (2, 7, 64, 32, 96, co.TAPS_3x3x3, 3)):
        M = B * D ** 3
        x = torch.randn(M, C1, generator=g)
        h = torch.randn(M, C2, generator=g) if C2 else None
        w = torch.randn(len(taps), Cout, C1 + C2, generator=g) * 0.05
        bias = torch.randn(Cout, generator=g)
        xin = (torch.cat([x, h], 1) if C2 else x).double().reshape(B, D, D, D, C1 + C2)
        ref = bias.double().expand(B, D, D, D, Cout).clone()
        for ti, (dz, dy, dx) in enumerate(taps):
            sh = torch.zeros_like(xin)
            zs, ys, xs = (slice(max(0, -d), D - max(0, d)) for d in (dz, dy, dx))
            zt, yt, xt = (slice(max(0, d), D - max(0, -d)) for d in (dz, dy, dx))
            sh[:, zs, ys, xs] = xin[:, zt, yt, xt]
            ref += sh @ w[ti].double().t()
        ref = ref.reshape(M, Cout)
        outs = []
        for tile in "ABCDE":
            o = torch.full((M, Cout), float("nan"), device=dev)
            with co.force_plan(tile=tile, ksplit=ks):
                co.conv_igemm(x.to(dev), C1, C1, None if h is None else h.to(dev), C2, C2, w.to(dev), bias.to(dev), None, None, 1.0, None, None, None, o, None,
                              (B, D, D, D), (D, D, D), Cout, Cout, taps, epilogue=co.EPI_BIAS)
            err = (o.cpu().double() - ref).abs().max().item()
            assert err < 2e-5 * max(1.0, ref.abs().max().item()), (tile, B, D, C1, C2, Cout, len(taps), ks, err)
            outs.append(o)
        for o in outs[1:]:
            assert (o - outs[0]).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("Cin,Cout,dims,k", [(8, 1, (6, 7, 9), 3), (8, 3, (1, 20, 17), 5), (16, 4, (3, 5, 4), 3), (4, 2, (2, 3, 70), 3)])
def test_conv_direct_fwd_dgrad_wgrad_vs_torch(dev, Cin, Cout, dims, k):
    """direct kernels for tiny channel counts (density head 8->1 3x3x3, conv_rgb 8->3 5x5) against torch's conv autograd on the CPU."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(Cin * 10 + Cout)
    D, H, W = dims
    x = torch.randn(2, Cin, D, H, W, generator=g, requires_grad=True)
    kd = k if D > 1 else 1
    w = (torch.randn(Cout, Cin, kd, k, k, generator=g) / (kd * k * k * Cin) ** 0.5).requires_grad_(True)
    b = torch.randn(Cout, generator=g, requires_grad=True)
    ref = torch.nn.functional.conv3d(x, w, b, padding=(kd // 2, k // 2, k // 2))
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy)
    taps = [(a - kd // 2, bb - k // 2, c - k // 2) for a in range(kd) for bb in range(k) for c in range(k)]
    xd = _rows(x.detach()).to(dev).requires_grad_(True)
    wd = w.detach().to(dev).requires_grad_(True)
    bd = b.detach().to(dev).requires_grad_(True)
    out = co.conv_direct_rows(xd, wd.reshape(Cout, Cin, -1).permute(2, 0, 1), bd, taps)
    out.backward(_rows(gy).to(dev))
    tol = lambda t: 3e-5 * max(1.0, t.abs().max().item())
    assert (out.detach().permute(0, 4, 1, 2, 3).cpu() - ref.detach()).abs().max().item() < tol(ref.detach())
    assert (xd.grad.permute(0, 4, 1, 2, 3).cpu() - x.grad).abs().max().item() < tol(x.grad)
    assert (wd.grad.cpu() - w.grad).abs().max().item() < 1e-4 * max(1.0, w.grad.abs().max().item())
    assert (bd.grad.cpu() - b.grad).abs().max().item() < 1e-4 * max(1.0, b.grad.abs().max().item())


def test_conv_rgb_autograd_hip_vs_torch(dev):
    """a7 with an autograd graph (models/volume_render.py:29-37,73): forward, input gradient and every parameter gradient of the HIP
    path (narrow-N GEMM / narrow wgrad / direct kernels) against torch's own conv autograd on the CPU, BatchNorm in train mode."""
    import copy
    from forge_amd import synthetic as syn
    from forge_amd.volume_render import VolRender
    torch.manual_seed(3)
    ref = VolRender(syn.kubric_config()).train()
    with torch.no_grad():
        for prm in ref.conv_rgb.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    hip = copy.deepcopy(ref).to(dev)
    x = torch.randn(3, 16, 24, 40)
    gy = torch.randn(3, 3, 48, 80)
    xr = x.clone().requires_grad_(True)
    yr = torch.relu(ref.conv_rgb(xr))
    yr.backward(gy)
    xh = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yh = hip._conv_rgb_autograd_hip(xh)
    yh.backward(gy.to(dev))
    rel = lambda a, b: (a.cpu() - b).abs().max().item() / max(b.abs().max().item(), 1e-6)
    assert rel(yh.detach(), yr.detach()) < 1e-4
    assert rel(xh.grad, xr.grad) < 2e-4
    gscale = max(pr.grad.abs().max().item() for pr in ref.conv_rgb.parameters())
    for (k, ph), (_, pr) in zip(hip.conv_rgb.named_parameters(), ref.conv_rgb.named_parameters()):
        # (a conv bias in front of a train-mode BatchNorm has an analytically zero gradient: absolute floor from the overall scale)
        assert (ph.grad.cpu() - pr.grad).abs().max().item() < 5e-4 * max(pr.grad.abs().max().item(), 1e-2 * gscale), k
    for bh, br in zip(hip.conv_rgb.buffers(), ref.conv_rgb.buffers()):          # BatchNorm running statistics were updated identically
        assert rel(bh.float(), br.float()) < 1e-4


@pytest.mark.parametrize("n,H,W,k,pad", [(3, 24, 40, 6, 2), (1, 7, 33, 6, 2), (2, 16, 64, 4, 1), (5, 9, 5, 6, 2)])
def test_narrow_transposed_conv_s2_autograd_vs_torch(dev, n, H, W, k, pad):
    """ConvTranspose2d(16, 16, k, stride 2) on NHWC rows (conv_rgb[0], models/volume_render.py:29-31) with autograd: forward (phase GEMMs on the
    narrow-N kernel), data gradient (stride-2 gather GEMM) and weight gradient - conv_wgrad_lines_kernel<Mfma16x16x4, 16, 2, 9, 4>: k^2 <= 36 taps on <= 6
    lines, the gathered operand on the 2x finer grid - against torch's own autograd; widths that are no multiple of the 32-voxel segment,
    single rows of segments, several images."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(n * 100 + W)
    x = torch.randn(n, 16, H, W, generator=g)
    w = torch.randn(16, 16, k, k, generator=g) * 0.1
    b = torch.randn(16, generator=g) * 0.1
    gy = torch.randn(n, 16, 2 * H, 2 * W, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.nn.functional.conv_transpose2d(xr, wr, br, stride=2, padding=pad)
    ref.backward(gy)
    xd = x.permute(0, 2, 3, 1).reshape(n, 1, H, W, 16).contiguous().to(dev).requires_grad_(True)
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = co.convT_s2_rows(xd, wd, bd, pad, 2)
    assert out.shape == (n, 1, 2 * H, 2 * W, 16)
    out.backward(gy.permute(0, 2, 3, 1).reshape(n, 1, 2 * H, 2 * W, 16).contiguous().to(dev))
    rel = lambda a, e: (a.cpu() - e).abs().max().item() / max(e.abs().max().item(), 1e-12)
    assert rel(out.detach()[:, 0].permute(0, 3, 1, 2), ref.detach()) < 3e-5
    assert rel(xd.grad[:, 0].permute(0, 3, 1, 2), xr.grad) < 1e-4
    assert rel(wd.grad, wr.grad) < 1e-4
    assert rel(bd.grad, br.grad) < 1e-4


@pytest.mark.parametrize("case", ["convT3d_128_32", "conv3d_64_128", "conv2d_9taps_32", "conv3d_48_2taps", "small_M_ungrouped"])
def test_conv_wgrad_tap_grouped_tiles_vs_float64(dev, case):
    """forge_conv_wgrad on narrow single inputs with several taps and M >= 131072 rows - conv_wgrad_kernel<32, 4> / <64, 2>: TG taps share one
    128-column tile (the heads' ConvTranspose3d(128, 32, 4, s2) weight gradient: 64 taps, stride-2 gathered operand; conv1's Conv3d(64, 128, 3):
    27 taps; tap counts that are no multiple of the group; Cin below the group's channel width; a small problem that stays on the ungrouped
    tiles) - against the float64 contraction dW[t] = dY^T X_t written with torch slices and matmuls (stock float64 kernels)."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(len(case))
    if case == "convT3d_128_32":        # 'dy' operand = x [n,D,H,W,128] (rows), gathered operand = dY [n,2D,2H,2W,32] at 2 z - 1 + k, 64 taps
        n, D, H, W, Cy, Cx, ist = 2, 16, 64, 64, 128, 32, 2
        taps = [(kz - 1, ky - 1, kx - 1) for kz in range(4) for ky in range(4) for kx in range(4)]
    elif case == "conv3d_64_128":
        n, D, H, W, Cy, Cx, ist = 1, 33, 64, 63, 128, 64, 1
        taps = co.TAPS_3x3x3
    elif case == "conv2d_9taps_32":     # 9 taps in groups of 4: the last group holds one tap
        n, D, H, W, Cy, Cx, ist = 3, 1, 256, 200, 64, 32, 1
        taps = [(0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    elif case == "conv3d_48_2taps":     # Cin = 48 < 64 (ragged channel width inside the group), 2 taps = one group
        n, D, H, W, Cy, Cx, ist = 2, 8, 96, 90, 96, 48, 1
        taps = [(0, 0, 0), (1, 0, -1)]
    else:
        n, D, H, W, Cy, Cx, ist = 2, 4, 6, 5, 128, 32, 2
        taps = [(kz - 1, ky - 1, kx - 1) for kz in range(4) for ky in range(4) for kx in range(4)]
    Di, Hi, Wi = (D * ist if D > 1 else 1), H * ist, W * ist
    dy = torch.randn(n, D, H, W, Cy, generator=g).to(dev)
    x = torch.randn(n, Di, Hi, Wi, Cx, generator=g).to(dev)
    pad = 4
    xp = torch.nn.functional.pad(x.double(), (0, 0, pad, pad, pad, pad, pad if D > 1 else 0, pad if D > 1 else 0))
    dyf = dy.double().reshape(-1, Cy)
    ref = torch.empty(len(taps), Cy, Cx, dtype=torch.float64, device=dev)
    for t, (dz, dy_, dx) in enumerate(taps):
        z0 = (dz + pad) if D > 1 else 0
        xs = xp[:, z0:z0 + (D - 1) * ist + 1:ist, dy_ + pad:dy_ + pad + (H - 1) * ist + 1:ist, dx + pad:dx + pad + (W - 1) * ist + 1:ist]
        ref[t] = dyf.t() @ xs.reshape(-1, Cx)
    dw = torch.zeros(len(taps), Cy, Cx, device=dev)
    co.conv_wgrad(dy, x, Cx, None, 0, dw, (n, D, H, W), (Di, Hi, Wi), Cy, list(taps), istride=ist)
    err = (dw.double() - ref).abs().max().item()
    assert err < 2e-5 * ref.abs().max().item(), (case, err, ref.abs().max().item())


def test_conv_igemm_strided2d_and_transpose_phases(dev):
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(2)
    # 3x3 stride-2 2-D conv as a D=1 grid (ResNet layer2[0].conv2 shape family)
    x = torch.randn(2, 64, 18, 14, generator=g)
    w = torch.randn(96, 64, 3, 3, generator=g) / 24
    ref = torch.nn.functional.conv2d(x, w, None, stride=2, padding=1)
    Ho, Wo = ref.shape[-2:]
    taps = [(0, ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
    wp = w.reshape(96, 64, 9).permute(2, 0, 1).contiguous()
    out = torch.empty(2, 1, Ho, Wo, 96, device=dev)
    co.conv_igemm(x.permute(0, 2, 3, 1).contiguous().to(dev), 64, 64, None, 0, 0, wp.to(dev), None, None, None, 1.0, None, None, None,
                  out, None, (2, 1, Ho, Wo), (1, 18, 14), 96, 96, taps, istride=2, epilogue=co.EPI_BIAS)
    # NB: with is=2 the D axis also scales (z*2+dz with z=0, dz=0 -> 0): fine for D=1
    assert (out[:, 0].permute(0, 3, 1, 2).cpu() - ref).abs().max().item() < 3e-5 * ref.abs().max().item()
    # ConvTranspose3d(k4,s2,p1) as 8 phase GEMMs
    x = torch.randn(1, 32, 4, 5, 3, generator=g)
    wt = torch.randn(32, 40, 4, 4, 4, generator=g) / 16
    b = torch.randn(40, generator=g)
    ref = torch.nn.functional.conv_transpose3d(x, wt, b, stride=2, padding=1)
    out = torch.empty(1, 8, 10, 6, 40, device=dev)
    for (pz, py, px), tp, wp in co.convT3d_k4s2p1_phases(wt):
        co.conv_igemm(_rows(x).to(dev), 32, 32, None, 0, 0, wp.to(dev), b.to(dev), None, None, 1.0, None, None, None, out, None,
                      (1, 4, 5, 3), (4, 5, 3), 40, 40, tp, out_grid=(8, 10, 6), ostride=2, phase=(pz, py, px), epilogue=co.EPI_BIAS)
    assert (out.permute(0, 4, 1, 2, 3).cpu() - ref).abs().max().item() < 3e-5 * ref.abs().max().item()


    # the same 8 phases merged into ONE launch (phase = (-1,-1,-1)): identical results, for every tile the plan may pick
    taps_all, wp_all = co.convT_phases_merged(wt, 1, 3)
    for tile in "CDE":
        with co.force_plan(tile=tile):
            out2 = torch.full((1, 8, 10, 6, 40), float("nan"), device=dev)
            co.conv_igemm(_rows(x).to(dev), 32, 32, None, 0, 0, wp_all.to(dev), b.to(dev), None, None, 1.0, None, None, None, out2, None,
                          (1, 4, 5, 3), (4, 5, 3), 40, 40, taps_all, out_grid=(8, 10, 6), ostride=2, phase=(-1, -1, -1), epilogue=co.EPI_BIAS)
        assert torch.equal(out2, out), tile
    # 2-D, narrow-N kernel: ConvTranspose2d(16, 16, 6, stride 2, padding 2) as 4 merged phases (conv_rgb's first layer)
    x2 = torch.randn(2, 16, 9, 11, generator=g)
    wt2 = torch.randn(16, 16, 6, 6, generator=g) / 24
    b2 = torch.randn(16, generator=g)
    ref2 = torch.nn.functional.conv_transpose2d(x2, wt2, b2, stride=2, padding=2)
    taps2, wp2 = co.convT_phases_merged(wt2, 2, 2)
    o2 = torch.full((2, 1, 18, 22, 16), float("nan"), device=dev)
    co.conv_igemm(x2.permute(0, 2, 3, 1).contiguous().to(dev), 16, 16, None, 0, 0, wp2.to(dev), b2.to(dev), None, None, 1.0, None, None, None, o2, None,
                  (2, 1, 9, 11), (1, 9, 11), 16, 16, taps2, out_grid=(1, 18, 22), ostride=2, phase=(-1, -1, -1), epilogue=co.EPI_BIAS)
    assert (o2[:, 0].permute(0, 3, 1, 2).cpu() - ref2).abs().max().item() < 3e-5 * ref2.abs().max().item()


def test_fuse_hip_vs_oracle(dev):
    """ConvGRU fusion (fusion_conv h0 + t GRU steps + fusion_norm) through the fused MFMA path vs the oracle."""
    from forge_amd.fusion import ConvGRU_3D
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=32, hidden_size=32)
    pre = "encoder_3d.fusion_feature."
    w = syn.seeded_state_dict({pre + k: v for k, v in gru.state_dict().items()}, 9)
    gru.load_state_dict({k[len(pre):]: v for k, v in w.items()})
    gru = gru.to(dev).eval()
    x = torch.randn(2, 3, 32, 8, 8, 8, generator=torch.Generator().manual_seed(4))
    ref = fo.fuse(x, w)
    with torch.no_grad():
        got = gru.fuse_hip(x.to(dev)).cpu()
        stock = gru(x.to(dev), [gru.fusion_conv(x.to(dev).mean(dim=1))]).cpu()     # reference-style call: h0 from the caller (torch/MIOpen fusion_conv), recurrence on HIP
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())
    assert (stock - ref).abs().max().item() < 1e-3 * max(1.0, ref.abs().max().item())


def test_heads_and_conv1_hip_vs_golden(dev, golden):
    from forge_amd.encoder import Encoder3D
    g = golden("heads_toy")
    enc = Encoder3D(syn.kubric_config())
    tmpl = {"encoder_3d." + k: v for k, v in enc.state_dict().items()}
    w = syn.seeded_state_dict(tmpl, int(g["weight_seed"]))
    enc.load_state_dict({k[len("encoder_3d."):]: v for k, v in w.items()})
    enc = enc.to(dev).eval()
    z = T(g["z"]).to(dev)
    with torch.no_grad():
        dens = enc.get_density3D(z).cpu()
        feat = enc.get_render_features(z).cpu()
    assert (dens - T(g["density"])).abs().max().item() < 5e-5
    assert (feat - T(g["features"])).abs().max().item() < 5e-5
    # conv1 on a random 64-channel volume
    x = torch.randn(2, 64, 32, 6, 6, generator=torch.Generator().manual_seed(8))
    ref = torch.nn.functional.leaky_relu(fo._bn(torch.nn.functional.conv3d(x, w["encoder_3d.conv1.0.weight"], w["encoder_3d.conv1.0.bias"], padding=1),
                                                w, "encoder_3d.conv1.1"), 0.01)
    with torch.no_grad():
        got = enc._conv1_hip(x.permute(0, 2, 3, 4, 1).contiguous().to(dev)).cpu()
    assert (got - ref).abs().max().item() < 5e-5 * max(1.0, ref.abs().max().item())


def test_encoder_trunk_hip_vs_oracle(dev):
    """ResNet-50 layers 1-4 on the GEMM kernel + fused 2D->3D lift + conv1 vs the oracle's get_feat3D
    (tolerance: 53 conv layers deep, activations O(1..25))."""
    from forge_amd.encoder import Encoder3D
    enc = Encoder3D(syn.kubric_config())
    w = syn.seeded_state_dict({"encoder_3d." + k: v for k, v in enc.state_dict().items()}, 0)
    enc.load_state_dict({k[len("encoder_3d."):]: v for k, v in w.items()})
    enc = enc.to(dev).eval()
    img = torch.rand(2, 3, 128, 96, generator=torch.Generator().manual_seed(21))       # non-square, small
    ref = fo.get_feat3D(img, w)
    with torch.no_grad():
        got = enc.get_feat3D(img.to(dev)).cpu()
        z2d = enc.feature_extraction(img.to(dev))                                       # stock trunk, same device
        lifted = enc._trunk_hip(img.to(dev))
    assert got.shape == ref.shape == (2, 128, 32, 16, 12)
    assert (got - ref).abs().max().item() < 2e-4 * max(1.0, ref.abs().max().item())
    # the fused lift equals view(-1,64,32,H,W) of the stock trunk output
    ref_l = z2d.view(-1, 64, 32, 16, 12).permute(0, 2, 3, 4, 1)
    assert (lifted - ref_l).abs().max().item() < 2e-4 * max(1.0, ref_l.abs().max().item())


@pytest.mark.parametrize("Cin,Cout", [(32, 16), (16, 8), (16, 1), (48, 12)])
def test_conv_igemm_narrow_n(dev, Cin, Cout):
    """Cout <= 16 -> the v_mfma_f32_16x16x4_f32 variant (K-step 16)."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(Cin * 7 + Cout)
    x = torch.randn(2, Cin, 5, 9, 7, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    b, sc, sh = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv3d(x, w, b, padding=1) * sc[None, :, None, None, None]
                                         + sh[None, :, None, None, None], 0.01)
    out = torch.zeros(2, 5, 9, 7, 16, device=dev)                      # row stride 16 > Cout: padded output
    co.conv_igemm(_rows(x).to(dev), Cin, Cin, None, 0, 0, co.pack_conv3d_weight(w).to(dev), b.to(dev), sc.to(dev), sh.to(dev), 0.01,
                  None, None, None, out, None, (2, 5, 9, 7), (5, 9, 7), Cout, 16, co.TAPS_3x3x3, epilogue=co.EPI_AFFINE_ACT)
    got = out[..., :Cout].permute(0, 4, 1, 2, 3).cpu()
    assert (got - ref).abs().max().item() < 3e-5 * max(1.0, ref.abs().max().item())
    assert out[..., Cout:].abs().max().item() == 0.0 if Cout < 16 else True


@pytest.mark.parametrize("dims,k2d", [((4, 6, 70), False), ((3, 5, 2), False), ((1, 9, 300), True), ((1, 7, 3), True)])
def test_conv_igemm_narrow_lines_kernel_vs_generic_and_torch(dev, dims, k2d):
    """Cout <= 16 with complete x-lines of taps (3x3x3, dx fastest; 5x5) runs conv_igemm_n16_lines_kernel - the slab of a (dz, dy) line staged once,
    its dx taps as shifted views, x-line ends masked; the SAME taps in a shuffled order run the generic narrow kernel. Both against torch (3e-5) and
    against each other (summation order only), with two concatenated inputs, a residual, rows that are not a multiple of the 256-row tile, x-lines
    shorter than the tile / than the tap radius, and batch boundaries inside a tile."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(sum(dims) + k2d)
    D, H, W = dims
    n, C1, C2, Cout = 3, 16, 16, 12
    kd, k = (1, 5) if k2d else (3, 3)
    x1, x2 = torch.randn(n, C1, D, H, W, generator=g), torch.randn(n, C2, D, H, W, generator=g)
    w = torch.randn(Cout, C1 + C2, kd, k, k, generator=g) / (kd * k * k * (C1 + C2)) ** 0.5
    b, sc, sh = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    res = torch.randn(n, Cout, D, H, W, generator=g)
    bc = lambda v: v[None, :, None, None, None]
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv3d(torch.cat([x1, x2], 1), w, b, padding=(kd // 2, k // 2, k // 2)) * bc(sc) + bc(sh) + res, 0.01)
    taps = [(dz, dy, dx) for dz in range(-(kd // 2), kd // 2 + 1) for dy in range(-(k // 2), k // 2 + 1) for dx in range(-(k // 2), k // 2 + 1)]
    wp = w.permute(2, 3, 4, 0, 1).reshape(len(taps), Cout, C1 + C2).contiguous()
    perm = torch.randperm(len(taps), generator=g).tolist()
    outs = []
    for order in (list(range(len(taps))), perm):                         # complete lines -> lines kernel; shuffled -> generic kernel
        out = torch.full((n, D, H, W, 16), float("nan"), device=dev)
        res16 = torch.nn.functional.pad(_rows(res), (0, 16 - Cout)).to(dev)           # the residual shares the output's row stride (16)
        co.conv_igemm(_rows(x1).to(dev), C1, C1, _rows(x2).to(dev), C2, C2, wp[order].contiguous().to(dev), b.to(dev), sc.to(dev), sh.to(dev), 0.01,
                      res16, None, None, out, None, (n, D, H, W), (D, H, W), Cout, 16, [taps[i] for i in order], epilogue=co.EPI_AFFINE_ACT)
        got = out[..., :Cout].permute(0, 4, 1, 2, 3).cpu()
        assert (got - ref).abs().max().item() < 3e-5 * max(1.0, ref.abs().max().item())
        outs.append(got)
    assert (outs[0] - outs[1]).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


def test_conv_igemm_2d_5x5_and_transpose2d(dev):
    """the conv_rgb shapes: 25-tap 5x5 conv and ConvTranspose2d(k6,s2,p2) as 4 phase GEMMs of 9 taps."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 16, 11, 13, generator=g)
    w = torch.randn(8, 16, 5, 5, generator=g) / 20
    b = torch.randn(8, generator=g)
    ref = torch.nn.functional.conv2d(x, w, b, padding=2)
    wp, taps = co.pack_conv2d_weight(w)
    out = torch.empty(2, 11, 13, 8, device=dev)
    co.conv_igemm(x.permute(0, 2, 3, 1).contiguous().to(dev), 16, 16, None, 0, 0, wp.to(dev), b.to(dev), None, None, 1.0, None, None, None,
                  out, None, (2, 1, 11, 13), (1, 11, 13), 8, 8, taps, epilogue=co.EPI_BIAS)
    assert (out.permute(0, 3, 1, 2).cpu() - ref).abs().max().item() < 3e-5 * ref.abs().max().item()
    wt = torch.randn(16, 16, 6, 6, generator=g) / 24
    ref = torch.nn.functional.conv_transpose2d(x, wt, b.repeat(2), stride=2, padding=2)
    out = torch.empty(2, 22, 26, 16, device=dev)
    for (pz, py, px), tp, wpp in co.convT_phases(wt, 2, 2):
        co.conv_igemm(x.permute(0, 2, 3, 1).contiguous().to(dev), 16, 16, None, 0, 0, wpp.to(dev), b.repeat(2).to(dev), None, None, 1.0,
                      None, None, None, out, None, (2, 1, 11, 13), (1, 11, 13), 16, 16, tp, out_grid=(1, 22, 26), ostride=2,
                      phase=(0, py, px), epilogue=co.EPI_BIAS)
    assert (out.permute(0, 3, 1, 2).cpu() - ref).abs().max().item() < 3e-5 * ref.abs().max().item()


def test_render_camera_gradients_vs_oracle_autograd(dev):
    """row f2: d loss / d (R, T, fx, fy, cx, cy) of the ray-marcher (pose refinement, kubric_eval.py:450-503)."""
    D, C, img, S = 16, 16, 48, 40
    feat, dens = syn.blob_volumes(2, D, C, seed=13)
    _, extr, _ = syn.orbit_cameras(10, 1.5, 15.0)
    E = extr[[1, 4, 8]]
    Kh0 = fo.halve_intrinsics(syn.intrinsics(img)[None].repeat(3, 1, 1))
    v2v = torch.tensor([0, 1, 0], dtype=torch.int32)
    Hr = img // 2
    wgt = torch.randn(3, Hr, Hr, C + 2, generator=torch.Generator().manual_seed(6))
    R = E[:, :3, :3].clone().requires_grad_(True)
    Tt = E[:, :3, 3].clone().requires_grad_(True)
    Kh = Kh0.clone().requires_grad_(True)
    ref = fo.render_rays(feat[v2v.long()], dens[v2v.long()], R, Tt, Kh, Hr, Hr, S, 0.5, 2.0, 1.0, True)
    (ref * wgt).sum().backward()
    cam = _cam_pack(E[:, :3, :3], E[:, :3, 3], Kh0).to(dev).requires_grad_(True)
    h = [fo.grid_half_extent(D, 1.0)] * 3
    outs = ops.render_rays(feat.to(dev), dens.to(dev), cam, v2v.to(dev), Hr, Hr, S, 0.5, 2.0, h, True)
    (torch.cat(outs, dim=1).permute(0, 2, 3, 1) * wgt.to(dev)).sum().backward()
    g = cam.grad.cpu()
    exp = torch.cat([R.grad.reshape(3, 9), Tt.grad, Kh.grad[:, 0, 0:1], Kh.grad[:, 1, 1:2], Kh.grad[:, 0, 2:3], Kh.grad[:, 1, 2:3]], dim=1)
    for sl, name in ((slice(0, 9), "R"), (slice(9, 12), "T"), (slice(12, 14), "f"), (slice(14, 16), "c")):
        scale = exp[:, sl].abs().max().item()
        assert (g[:, sl] - exp[:, sl]).abs().max().item() < 2e-3 * scale, name


def test_pose_refinement_step_runs(dev):
    """gradients reach a 7-D pose (quaternion + translation) through rotate and render, as in kubric_eval.py:450-503."""
    from forge_amd import geo_utils
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    for p_ in model.parameters():
        p_.requires_grad_(False)
    sample = syn.make_sample(1, 3, 256, 1.5, seed=5)
    with torch.no_grad():
        feats = model.encoder_3d.get_feat3D(sample["images"][0].to(dev)).reshape(1, 3, 128, 32, 32, 32)
    pose7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][0, 1:]).to(dev).requires_grad_(True)       # [2,7]
    can = syn.SyntheticDataset(1.5).get_canonical_pose_cv2(dev)
    poses = torch.cat([can[None], can[None] @ geo_utils.quat2mat(pose7)], dim=0)[None]                 # [1,3,4,4]
    ft = model.rotate(voxels=feats, camPoses_cv2=poses, grid_size=32)
    fused = model.encoder_3d.fuse(ft)
    E = torch.inverse(poses[0])
    cams = {"R": E[:, :3, :3], "T": E[:, :3, 3], "K": sample["K_cv2"][0].to(dev)}
    v2v = torch.zeros(3, dtype=torch.int32, device=dev)
    imgs, masks = model.render(cams, model.encoder_3d.get_render_features(fused), model.encoder_3d.get_density3D(fused), view2vol=v2v)
    loss = torch.nn.functional.mse_loss(imgs, sample["images"][0].to(dev)) + torch.nn.functional.mse_loss(masks, sample["fg_probabilities"][0].to(dev))
    loss.backward()
    assert pose7.grad is not None and torch.isfinite(pose7.grad).all() and pose7.grad.abs().max().item() > 0


def test_graphed_forward_matches_eager(dev):
    """hipGraph replay of the whole inference step gives the eager result, and tracks new inputs."""
    from forge_amd.graph import GraphedForward
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    s1 = {k: v.to(dev) for k, v in syn.make_sample(1, 5, 256, 1.5, seed=7).items()}
    s2 = {k: v.to(dev) for k, v in syn.make_sample(1, 5, 256, 1.5, seed=8).items()}
    with torch.no_grad():
        e1 = [t.clone() for t in model(s1, ds, dev)]
        e2 = [t.clone() for t in model(s2, ds, dev)]
    g = GraphedForward(model, s1, ds, dev)
    o1 = [t.clone() for t in g(s1)]
    o2 = [t.clone() for t in g(s2)]
    for a, b in zip(e1 + e2, o1 + o2):
        assert torch.equal(a, b)
    assert not torch.equal(o1[0], o2[0])


def test_pipelined_forward_matches_eager_with_samples_dropped_after_the_call(dev):
    """PipelinedForward (several hipGraph replays in flight on private streams): every step's outputs equal the eager forward bit for bit,
    also when the caller drops each sample right after p(sample) and allocates other tensors of the same size on its own stream (a
    data-loader loop): the sample's memory is held (record_stream) until the slot's copy has read it."""
    from forge_amd.graph import PipelinedForward
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    host = [syn.make_sample(1, 5, 256, 1.5, seed=20 + i) for i in range(5)]
    with torch.no_grad():
        eager = [[t.clone() for t in model({k: v.to(dev) for k, v in h.items()}, ds, dev)] for h in host]
    p = PipelinedForward(model, {k: v.to(dev) for k, v in host[0].items()}, ds, dev, depth=3, warmup=1)
    for rnd in range(2):                                   # 10 calls on 3 slots: every slot is reused
        outs = []
        for i, h in enumerate(host):
            s = {k: v.to(dev) for k, v in h.items()}
            o = p(s)
            shapes = [v.shape for v in s.values() if torch.is_tensor(v)]
            del s                                          # the allocator may now recycle the blocks ...
            junk = [torch.full(sh, float("nan"), device=dev) for sh in shapes]      # ... and the caller's stream writes same-sized tensors at once
            if (i + 1) % 3 == 0 or i == len(host) - 1:     # outputs of a slot are valid after wait() and until the slot's next call
                p.wait()
                torch.cuda.synchronize()
                outs.append((i, [t.clone() for t in o]))
            del junk
        for i, o in outs:
            for a, b in zip(eager[i], o):
                assert torch.equal(a, b), (rnd, i)


def test_render_360_vs_oracle(dev):
    """row f3: 28-view orbit + depth from ONE volume in one launch vs the oracle renderer fed the same (quirky) cameras."""
    from forge_amd import nvs
    from forge_amd.volume_render import VolRender
    cfg = syn.kubric_config(img_size=64, n_pts_per_ray=48)
    vr = VolRender(cfg)
    w = syn.seeded_state_dict({"render." + k: v for k, v in vr.state_dict().items()}, 3)
    vr.load_state_dict({k[len("render."):]: v for k, v in w.items()})
    vr = vr.to(dev).eval()
    feat, dens = syn.blob_volumes(2, 16, 16, seed=31)
    K = syn.intrinsics(64)

    class M:            # minimal model stand-in: render_360 only needs `.render`
        render = vr
    imgs, masks, depths = nvs.render_360(M, feat.to(dev), dens.to(dev), K, 1.5, n_views=28, render_depth=True)
    assert imgs.shape == (2, 28, 3, 64, 64) and depths.shape == (2, 28, 1, 64, 64)
    R, T = nvs.nvs_cameras(1.5)
    for s in range(2):
        ref = fo.vol_render(feat[s:s + 1].repeat(28, 1, 1, 1, 1), dens[s:s + 1].repeat(28, 1, 1, 1, 1).clamp(max=1.0), R, T,
                            K[None].repeat(28, 1, 1), w, 64, 48, 0.5, 2.0, 1.0, 5, True, False)
        assert (imgs[s].cpu() - ref[0]).abs().max().item() < 1e-4
        assert (masks[s].cpu() - ref[1]).abs().max().item() < 2e-5
        assert (depths[s].cpu() - ref[2]).abs().max().item() < 2e-5


def test_render_360_vs_the_reference_visualize_360(dev, golden):
    """Row f3 against the REFERENCE's own 360-degree NVS: tests/golden/nvs_360.npz = kubric_eval.py:166-232 `visualize_360` on the reference FORGE model
    (oracle/make_golden.py::nvs_goldens; the function's image-writing sink replaced by a recorder) - camera chain from the GT relative poses, rotate, view ordering,
    ConvGRU fusion, both heads, 28 look_at_view_transform cameras used as if they were OpenCV extrinsics, densities clamped to <= 1, depth channel. Here: the same
    stages on the MI355X, the 28 views as ONE ray-marcher launch (forge_amd.nvs.render_360). Tolerances as the full-forward tests against the reference's output:
    max-abs 4e-4 of the image scale, PSNR > 90 dB, masks / depths 2e-4."""
    from forge_amd import geo_utils, nvs
    from forge_amd.model import FORGE
    g = golden("nvs_360")
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), int(g["weight_seed"])))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    sample = {k: v[:, :5].contiguous().to(dev) for k, v in syn.make_sample(1, 10, 256, 1.5, seed=int(g["sample_seed"])).items()}
    with torch.no_grad():
        feats = model.encoder_3d.get_feat3D(sample["images"][0]).reshape(1, 5, 128, 32, 32, 32)
        _, poses, _ = geo_utils.predicted_camera_chain(T(g["poses"]).to(dev), model.encoder_traj.toSE3, ds.get_canonical_pose_cv2(device=dev),
                                                       ds.get_canonical_extrinsics_cv2(device=dev), 1, 5)
        fused = model.encoder_3d.fuse(model.rotate(voxels=feats, camPoses_cv2=poses, grid_size=32, order="distance"))
        feat_mv, dens_mv = model.encoder_3d.heads(fused)
        imgs, masks, depths = nvs.render_360(model, feat_mv, dens_mv, sample["K_cv2"][0, 0], float(g["camera_z"]), n_views=28, render_depth=True)
    imgs, masks, depths = imgs[0].cpu(), masks[0].cpu(), depths[0].cpu()
    assert imgs.shape == (28, 3, 256, 256) and float(T(g["masks_mean"]).mean()) > 0.3            # the object is in view all around the orbit
    assert_forward_close(imgs[:, :, ::8, ::8], T(g["imgs_sub"]), masks[:, :, ::8, ::8], T(g["masks_sub"]), "360 NVS vs reference visualize_360", max_abs=4e-4, psnr=90.0, mask_abs=2e-4)
    assert (depths[:, :, ::8, ::8] - T(g["depths_sub"])).abs().max().item() < 2e-4
    assert (imgs.mean(dim=(1, 2, 3)) - T(g["imgs_mean"])).abs().max().item() < 1e-4
    assert (depths.mean(dim=(1, 2, 3)) - T(g["depths_mean"])).abs().max().item() < 1e-4


def test_conv3x3x3_rows_autograd_vs_torch(dev):
    """forward, data gradient (same GEMM, negated taps, transposed weights) and the wgrad kernel vs torch autograd on CPU."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(17)
    x1 = torch.randn(2, 32, 6, 7, 9, generator=g)
    x2 = torch.randn(2, 128, 6, 7, 9, generator=g)
    w = torch.randn(64, 160, 3, 3, 3, generator=g) / 60
    b = torch.randn(64, generator=g)
    gy = torch.randn(2, 64, 6, 7, 9, generator=g)
    # wgrad needs C1 % 128 == 0 with two inputs -> put the 128-channel tensor first
    a1, a2, aw, ab = x2.clone().requires_grad_(True), x1.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.nn.functional.conv3d(torch.cat([a1, a2], 1), aw, ab, padding=1)
    ref.backward(gy)
    d1 = _rows(x2).to(dev).requires_grad_(True)
    d2 = _rows(x1).to(dev).requires_grad_(True)
    dw, db = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = co.conv3x3x3_rows(d1, d2, dw, db)
    out.backward(_rows(gy).to(dev))
    assert (out.detach().permute(0, 4, 1, 2, 3).cpu() - ref.detach()).abs().max().item() < 5e-5 * ref.abs().max().item()
    for got, exp, name in ((d1.grad.permute(0, 4, 1, 2, 3).cpu(), a1.grad, "dx1"), (d2.grad.permute(0, 4, 1, 2, 3).cpu(), a2.grad, "dx2"),
                           (dw.grad.cpu(), aw.grad, "dw"), (db.grad.cpu(), ab.grad, "db")):
        assert (got - exp).abs().max().item() < 1e-4 * exp.abs().max().item(), name


def test_fuse_autograd_hip_vs_oracle(dev):
    """ConvGRU fusion in train mode (batch-stat BN) through the HIP convs: output and all parameter/input gradients vs autograd
    through the oracle."""
    from forge_amd.fusion import ConvGRU_3D
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=128, hidden_size=128)
    pre = "encoder_3d.fusion_feature."
    w = syn.seeded_state_dict({pre + k: v for k, v in gru.state_dict().items()}, 9)
    gru.load_state_dict({k[len(pre):]: v for k, v in w.items()})
    gru = gru.to(dev).train()
    x = torch.randn(1, 2, 128, 6, 6, 6, generator=torch.Generator().manual_seed(4))
    wr = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in w.items()}
    xr = x.clone().requires_grad_(True)
    ref = fo.fuse(xr, wr, training=True)
    gy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5))
    ref.backward(gy)
    xd = x.to(dev).requires_grad_(True)
    got = gru.fuse_autograd_hip(xd)
    got.backward(gy.to(dev))
    assert (got.detach().cpu() - ref.detach()).abs().max().item() < 2e-4 * max(1.0, ref.abs().max().item())
    assert (xd.grad.cpu() - xr.grad).abs().max().item() < 2e-3 * xr.grad.abs().max().item()
    gscale = max(wr[pre + n_].grad.abs().max().item() for n_, _ in gru.named_parameters())
    for name, p_ in gru.named_parameters():
        e = wr[pre + name].grad          # conv biases in front of a train-mode BN have an analytically zero gradient: absolute floor
        assert (p_.grad.cpu() - e).abs().max().item() < 3e-3 * max(e.abs().max().item(), 1e-3 * gscale), name


def test_heads_autograd_hip_vs_oracle(dev, golden):
    """both heads in train mode (batch-stat BN) with HIP conv / conv-transpose forward, dgrad and wgrad vs autograd through the oracle."""
    from forge_amd.encoder import Encoder3D
    enc = Encoder3D(syn.kubric_config())
    w = syn.seeded_state_dict({"encoder_3d." + k: v for k, v in enc.state_dict().items() if "feature_extraction" not in k}, 0)
    enc.load_state_dict({k[len("encoder_3d."):]: v for k, v in w.items()}, strict=False)
    enc = enc.to(dev).train()
    z = torch.randn(2, 128, 4, 5, 3, generator=torch.Generator().manual_seed(9))
    wr = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in w.items()}
    zr = z.clone().requires_grad_(True)
    rd, rf = fo.density_head(zr, wr, training=True), fo.render_features_head(zr, wr, training=True)
    gd = torch.randn(rd.shape, generator=torch.Generator().manual_seed(1))
    gf = torch.randn(rf.shape, generator=torch.Generator().manual_seed(2))
    ((rd * gd).sum() + (rf * gf).sum()).backward()
    zd = z.to(dev).requires_grad_(True)
    d, f = enc.get_density3D(zd), enc.get_render_features(zd)
    ((d * gd.to(dev)).sum() + (f * gf.to(dev)).sum()).backward()
    assert (d.detach().cpu() - rd.detach()).abs().max().item() < 1e-4 * max(1.0, rd.abs().max().item())
    assert (f.detach().cpu() - rf.detach()).abs().max().item() < 1e-4 * max(1.0, rf.abs().max().item())
    assert (zd.grad.cpu() - zr.grad).abs().max().item() < 2e-3 * zr.grad.abs().max().item()
    names = [n for n, _ in enc.named_parameters() if n.startswith(("density_head", "features_head"))]
    gscale = max(wr["encoder_3d." + n].grad.abs().max().item() for n in names)
    params = dict(enc.named_parameters())
    for n in names:
        e = wr["encoder_3d." + n].grad
        assert (params[n].grad.cpu() - e).abs().max().item() < 3e-3 * max(e.abs().max().item(), 1e-3 * gscale), n


def test_conv2d_rows_strided_autograd_vs_torch(dev):
    """2-D conv autograd on rows incl. the stride-2 data gradient (transposed conv by pixel parity) and strided wgrad."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(23)
    for k, stride, Cin, Cout in ((3, 2, 64, 96), (1, 2, 64, 128), (3, 1, 32, 64), (1, 1, 96, 32)):
        x = torch.randn(2, Cin, 12, 16, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ref = torch.nn.functional.conv2d(xa, wa, None, stride=stride, padding=k // 2)
        gy = torch.randn(ref.shape, generator=g)
        ref.backward(gy)
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
        wd = w.to(dev).requires_grad_(True)
        out = co.conv2d_rows(xd, wd, None, stride=stride)
        out.backward(gy.permute(0, 2, 3, 1).contiguous().to(dev))
        tag = "k%d s%d" % (k, stride)
        assert (out.detach().permute(0, 3, 1, 2).cpu() - ref.detach()).abs().max().item() < 5e-5 * ref.abs().max().item(), tag
        assert (xd.grad.permute(0, 3, 1, 2).cpu() - xa.grad).abs().max().item() < 1e-4 * xa.grad.abs().max().item(), tag
        assert (wd.grad.cpu() - wa.grad).abs().max().item() < 1e-4 * wa.grad.abs().max().item(), tag


def test_conv3d_rows_strided_autograd_vs_torch_float64(dev):
    """convops.conv3d_rows (the 3-D pose estimator's convolutions, models/pose_estimator_3d.py:24-60): Conv3d(k = 3, padding = 1) with stride 1 and
    stride 2, bias, on channels-last rows - forward, data gradient (stride 2: eight parity-phase GEMMs of the transposed convolution), weight
    gradient (strided gather) and bias gradient against torch's float64 CPU convolution; shapes from the estimator's tail (8^3 -> 4^3 -> 2^3 -> 1^3)
    and a ragged one."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(29)
    for stride, Cin, Cout, dims, n in ((2, 64, 96, (8, 12, 6), 2), (2, 128, 64, (2, 2, 2), 3), (1, 64, 32, (5, 4, 6), 2), (2, 32, 64, (4, 4, 4), 1)):
        x = torch.randn(n, Cin, *dims, generator=g, dtype=torch.float64)
        w = torch.randn(Cout, Cin, 3, 3, 3, generator=g, dtype=torch.float64) / (27 * Cin) ** 0.5
        b = torch.randn(Cout, generator=g, dtype=torch.float64)
        xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ref = torch.nn.functional.conv3d(xa, wa, ba, stride=stride, padding=1)
        gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
        ref.backward(gy)
        xd = x.float().permute(0, 2, 3, 4, 1).contiguous().to(dev).requires_grad_(True)
        wd, bd = w.float().to(dev).requires_grad_(True), b.float().to(dev).requires_grad_(True)
        out = co.conv3d_rows(xd, wd, bd, stride=stride)
        out.backward(gy.float().permute(0, 2, 3, 4, 1).contiguous().to(dev))
        tag = "s%d %s" % (stride, dims)
        rel = lambda got, want: (got.double().cpu() - want).abs().max().item() / want.abs().max().item()
        assert out.shape[1:4] == ref.shape[2:], tag
        assert rel(out.detach().permute(0, 4, 1, 2, 3), ref.detach()) < 2e-5, tag
        assert rel(xd.grad.permute(0, 4, 1, 2, 3), xa.grad) < 5e-5, tag
        assert rel(wd.grad, wa.grad) < 5e-5, tag
        assert rel(bd.grad, ba.grad) < 2e-5, tag


def test_conv2d_rows_winograd_2d_training_path_vs_float64(dev):
    """The bottleneck conv2 of ResNet layer3 / layer4 in TRAINING (3x3, stride 1, 256 / 512 channels at 32 x 32): forward, data gradient and
    weight gradient take the 2-D Winograd launches (one depth tap, convops.wino_applies) - against torch's float64 convolution, and against
    the direct kernels (convops.winograd(False)) as the fp32 yard-stick; a narrower layer stays on the direct kernels (same results path)."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(31)
    for C, hw in ((256, 32), (512, 16), (128, 16)):
        x = torch.randn(3, C, hw, hw, generator=g)
        w = torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5
        xa, wa = x.double().requires_grad_(True), w.double().requires_grad_(True)
        ref = torch.nn.functional.conv2d(xa, wa, None, stride=1, padding=1)
        gy = torch.randn(ref.shape, generator=g)
        ref.backward(gy.double())
        assert co.wino_applies(co.TAPS_3x3, 1, 3, 1, hw, hw, C, 0, C) == (C >= co.WINO2D_MIN_C)
        res = {}
        for wino in (True, False):
            with co.winograd(wino):
                xd = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
                wd = w.to(dev).requires_grad_(True)
                out = co.conv2d_rows(xd, wd, None)
                out.backward(gy.permute(0, 2, 3, 1).contiguous().to(dev))
            res[wino] = (out.detach().permute(0, 3, 1, 2).cpu().double(), xd.grad.permute(0, 3, 1, 2).cpu().double(), wd.grad.cpu().double())
        for i, r64 in enumerate((ref.detach(), xa.grad, wa.grad)):
            ew, ed = (res[True][i] - r64).abs().max().item(), (res[False][i] - r64).abs().max().item()
            scale = r64.abs().max().item()
            assert ed < 2e-5 * scale and ew < 6e-5 * scale, (C, i, ew / scale, ed / scale)      # Winograd: <= ~3x the direct kernel's fp32 error


def test_get_feat3D_train_hip_vs_oracle(dev):
    """Encoder (ResNet trunk + lift + conv1) in TRAIN mode through the HIP convs: output and a few gradients vs the oracle autograd."""
    from forge_amd.encoder import Encoder3D
    enc = Encoder3D(syn.kubric_config())
    w = syn.seeded_state_dict({"encoder_3d." + k: v for k, v in enc.state_dict().items()}, 0)
    enc.load_state_dict({k[len("encoder_3d."):]: v for k, v in w.items()})
    enc = enc.to(dev).train()
    img = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(31))
    # the oracle evaluated in float64 is the yardstick: its own fp32 evaluation lands up to 1.6e-2 (of a gradient's max) from it on this
    # input - 53 layers of train-mode BatchNorm over 2 images amplify fp32 reordering noise and a ReLU argument at rounding distance of
    # zero flips whole gradient entries; the HIP path (direct or Winograd kernels) sits in the same band
    # (tools/debug/feat3d_train_noise.py). Output: 5e-5; gradients: 5e-2 of the max.
    wr = {k: (v.double() if v.dtype.is_floating_point else v).clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in w.items()}
    ref = fo.get_feat3D(img.double(), wr, training=True)
    gy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(32))
    ref.backward(gy.double())
    got = enc.get_feat3D(img.to(dev))
    got.backward(gy.to(dev))
    assert (got.detach().cpu().double() - ref.detach()).abs().max().item() < 5e-5 * max(1.0, ref.abs().max().item())
    params = dict(enc.named_parameters())
    for n in ("conv1.0.weight", "feature_extraction.7.2.conv3.weight", "feature_extraction.6.0.conv2.weight", "feature_extraction.5.0.downsample.0.weight",
              "feature_extraction.4.0.conv1.weight", "feature_extraction.0.weight", "feature_extraction.7.0.bn2.weight"):
        e = wr["encoder_3d." + n].grad
        rel = (params[n].grad.cpu().double() - e).abs().max().item() / max(e.abs().max().item(), 1e-12)
        assert rel < 5e-2, (n, rel)


def test_forge_two_scenes_10_views_vs_oracle(dev):
    """b = 2 scenes, 5 input + 5 novel cameras each (the FORGE 10-view layout, models/model.py:117-143): batch strides in the GRU,
    per-scene view ordering, view->volume indexing with b > 1."""
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    w = syn.seeded_state_dict(model.state_dict(), 0)
    model.load_state_dict(w)
    model = model.to(dev).eval()
    sample = syn.make_sample(2, 10, 256, 1.5, seed=11)
    with torch.no_grad():
        imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
        oi, om = fo.forward_hot_path(sample["images"][:, :5], sample["cam_poses_cv2_canonicalized"][:, :5],
                                     sample["cam_extrinsics_cv2_canonicalized"][:, :5], sample["K_cv2"][:, :5], w, cfg,
                                     order_by_distance=True, render_extrinsics=sample["cam_extrinsics_cv2_canonicalized"],
                                     render_K=sample["K_cv2"])
    assert imgs.shape == (20, 3, 256, 256) and masks.shape == (20, 1, 256, 256)
    assert_forward_close(imgs, oi, masks, om, "FORGE 2 scenes x 10 views")


def test_forge_joint_mode_forward_backward(dev):
    """BASELINE config 5 shape of the code path: FORGE with PREDICTED poses (2-D + 3-D pose estimators + pose head, stock torch),
    10 rendered views, 4-tuple return (models/model.py:148); the loss back-propagates through the ray-marcher's camera gradients
    and the rotate op's pose gradients into the pose head, and through the HIP conv backward kernels into the encoder."""
    from forge_amd.model import FORGE
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    sample = syn.make_sample(1, 10, 256, 1.5, seed=12)
    imgs, masks, origin_proj, pose = model(sample, syn.SyntheticDataset(1.5), dev)
    assert imgs.shape == (10, 3, 256, 256) and masks.shape == (10, 1, 256, 256) and origin_proj.shape == (10, 2)
    assert pose["pred"].shape == (4, 7) and pose["gt"].shape == (4, 7) and pose["conf"].shape == (4, 1)
    tgt_i = sample["images"][0].to(dev)
    loss = torch.nn.functional.mse_loss(imgs, tgt_i) + torch.nn.functional.mse_loss(masks, sample["fg_probabilities"][0].to(dev)) \
        + torch.nn.functional.mse_loss(pose["pred"], pose["gt"]) + 0.1 * torch.nn.functional.mse_loss(origin_proj, torch.full_like(origin_proj, 0.5))
    loss.backward()
    for name in ("pose_head.4.weight", "encoder_traj.pose_head_1.3.weight", "encoder_traj_2d.conv.9.weight", "encoder_3d.conv1.0.weight",
                 "encoder_3d.fusion_feature.cells.0.out_gate.weight", "encoder_3d.feature_extraction.4.0.conv1.weight"):
        g = dict(model.named_parameters())[name].grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0, name


def test_omniobject_density_clamp(dev):
    """config.dataset.name == 'omniobject3d' clamps densities to [0,1] before rendering (models/model.py:140-141)."""
    from forge_amd.model import FORGE
    w = None
    outs = []
    for name in ("kubric", "omniobject3d"):
        cfg = syn.kubric_config(dataset_name=name)
        model = FORGE(cfg)
        w = w or syn.seeded_state_dict(model.state_dict(), 0)
        model.load_state_dict(w)
        model = model.to(dev).eval()
        with torch.no_grad():
            outs.append(model(syn.make_sample(1, 5, 256, 1.5, seed=2), syn.SyntheticDataset(1.5), dev)[1].cpu())
    assert not torch.equal(outs[0], outs[1])           # the seeded density head emits values > 1, so the clamp must change the masks
    assert outs[1].max().item() <= 1.0 + 1e-5


def test_attention_vs_float64_and_torch(dev):
    """forge_attention_fwd (ops.attention): softmax(q k^T) v of models/model_utils.py:207-229 (one head of 64 channels, unscaled logits) with the
    N x N matrix kept in registers, against the float64 evaluation of softmax-then-matmul - with torch's fp32 evaluation of the same three ops on
    the GPU as the yardstick (the kernel has to stay within 2x its distance + 1e-6 of max) - on small ragged-tile shapes, with a value table shared
    by the batch (the positional table of the cross attention), with peaky logits (|logit| up to ~60: the running-max rescaling at work) and at the
    pose estimator's size (4 pairs x 4096 tokens). Arguments outside its domain are refused, not approximated."""
    from forge_amd import _lib, ops
    torch.manual_seed(17)
    rel = lambda got, want: (got.double() - want).abs().max().item() / want.abs().max().item()
    for B, Nq, Nk, shared, gain in ((3, 128, 192, False, 1.0), (2, 64, 64, True, 1.0), (2, 192, 128, False, 6.0), (40, 1024, 256, False, 1.0), (4, 4096, 4096, True, 1.0),
                                     (1, 4096, 4096, False, 2.5)):        # both key splits: 2 parts (ragged key counts, many query tiles) and 4 parts (few query tiles)
        q, k = torch.randn(B, Nq, 64, device=dev) * gain * 0.5, torch.randn(B, Nk, 64, device=dev) * 0.5
        v = torch.randn(1 if shared else B, Nk, 64, device=dev)
        with torch.no_grad():
            got = ops.attention(q, k, v)
            t32 = torch.matmul(torch.matmul(q, k.transpose(1, 2)).softmax(dim=-1), v)
            want = torch.matmul(torch.matmul(q.double(), k.double().transpose(1, 2)).softmax(dim=-1), v.double())
        eh, et = rel(got, want), rel(t32, want)
        if os.environ.get("FORGE_TEST_REPORT"):
            print("  attention B=%d Nq=%d Nk=%d shared_v=%s gain %.1f: hip/f64 %.2e torch/f64 %.2e" % (B, Nq, Nk, shared, gain, eh, et))
        assert got.shape == (B, Nq, 64) and eh <= 2.0 * et + 1e-6, (B, Nq, Nk, shared, gain, eh, et)
    q = torch.randn(1, 100, 64, device=dev)
    with torch.no_grad():
        assert not ops.attention_applies(q, q, q)                                  # 100 tokens: not a multiple of 64
        with pytest.raises(RuntimeError, match="multiples of 64"):
            ops.attention(q, q, q)
        assert ops.attention_applies(q[:, :64], q[:, :64], q[:, :64]) and not ops.attention_applies(q[:, :64, :32], q[:, :64, :32], q[:, :64, :32])
    assert not ops.attention_applies(q[:, :64], q[:, :64], q[:, :64])              # autograd on: torch's differentiable ops run instead
    L = _lib.lib()
    out = torch.empty(1, 64, 64, device=dev)
    rc = L.forge_attention_fwd(_lib.ptr(q), _lib.ptr(q), _lib.ptr(q), 64, _lib.ptr(out), 1, 100, 64, 64, _lib.current_stream())
    assert rc != 0 and b"multiples of 64" in L.forge_last_error()
    rc = L.forge_attention_fwd(_lib.ptr(q), _lib.ptr(q), _lib.ptr(q), 64, _lib.ptr(out), 1, 64, 64, 32, _lib.current_stream())
    assert rc != 0 and b"64 channels" in L.forge_last_error()


def test_grad_zero_arena_keeps_one_pool_per_stream(dev):
    """convops.grad_zeros inside a backward pass whose nodes run on two HIP streams (the grouped fusion's weight gradients, FORGE's 2-D pose
    estimator): each stream's requests are carved from a pool that was allocated and zero-filled ON that stream - never from the other stream's,
    whose fill nothing orders them behind - and every slice arrives zeroed."""
    from forge_amd import convops as co
    arena = co._ZeroArena()
    side = torch.cuda.Stream(dev)
    got = []

    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            main = torch.cuda.current_stream(dev)
            a = arena.zeros((1000,), dev)
            z0 = float(a.abs().sum())
            a.add_(1.0)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                b, c = arena.zeros((3, 700), dev), arena.zeros((50,), dev)
                z1 = float(b.abs().sum()) + float(c.abs().sum())
                b.add_(2.0)
                c.add_(3.0)
            main.wait_stream(side)
            got.append((a, b, c, z0, z1))
            return g * 2

    x = torch.ones(4, device=dev, requires_grad=True)
    for _ in range(3):
        Node.apply(x).sum().backward()
    torch.cuda.synchronize()
    assert len(arena.want) == 2 and arena.task == -1
    a, b, c, z0, z1 = got[-1]
    assert z0 == 0.0 and z1 == 0.0 and float(a.sum()) == 1000.0 and float(b.sum()) == 4200.0 and float(c.sum()) == 150.0
    sa, sb, sc = (t.untyped_storage().data_ptr() for t in (a, b, c))
    assert sb == sc and sa != sb and b.data_ptr() != c.data_ptr()                 # b, c share the side stream's pool; a sits in the main stream's
    a1, b1 = got[1][0], got[1][1]
    assert a1.untyped_storage().data_ptr() != sa and b1.untyped_storage().data_ptr() != sb and float(a1.sum()) == 1000.0   # earlier passes' slices untouched


def test_clip_grad_norm_equals_torch_on_mixed_dtype_gradients(dev):
    """train.clip_grad_norm_ (one multi-tensor multiply per dtype group) against torch.nn.utils.clip_grad_norm_ on FORGE's parameter mix - float32
    gradients plus the float64 positional embedding of the 2-D pose estimator, which sends torch's own foreach path to 550 per-tensor launches: total
    norm and every clipped gradient bit for bit, with the clip active (coefficient < 1) and inactive."""
    from forge_amd import train
    torch.manual_seed(21)
    shapes = [(64, 32, 3, 3, 3), (128,), (7, 5), (1, 256, 256), (3,), (33, 17)]
    for scale in (10.0, 1e-3):
        a = [torch.nn.Parameter(torch.randn(sh, device=dev, dtype=torch.float64 if i == 3 else torch.float32)) for i, sh in enumerate(shapes)]
        b = [torch.nn.Parameter(p.detach().clone()) for p in a]
        for p, q in zip(a, b):
            p.grad = torch.randn_like(p) * scale
            q.grad = p.grad.clone()
        a.append(torch.nn.Parameter(torch.zeros(4, device=dev)))              # a parameter without a gradient
        b.append(torch.nn.Parameter(torch.zeros(4, device=dev)))
        t_ref = torch.nn.utils.clip_grad_norm_(b, 10.0, norm_type=2.0)      # torch's default on GPU tensors: multi-tensor norms, then its multiply
        t_got = train.clip_grad_norm_(a, 10.0)
        assert t_got.dtype == t_ref.dtype == torch.float64 and torch.equal(t_got, t_ref)
        assert (t_ref.item() > 10.0) == (scale == 10.0)
        for p, q in zip(a[:-1], b[:-1]):
            assert p.grad.dtype == q.grad.dtype and torch.equal(p.grad, q.grad)
        assert a[-1].grad is None


def test_train_step_harness(dev):
    """row f1: compute_reconstruction_loss + train_step (clip 10, Adam) run on the HIP model; the loss dict equals the formulas of
    scripts/kubric_compute_loss.py:26-35 evaluated separately, and a few steps reduce the loss."""
    from forge_amd import train
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=cfg.train.lr)
    sample = syn.make_sample(1, 5, 256, 1.5, seed=6)
    ds = syn.SyntheticDataset(1.5)
    first = None
    for it in range(4):
        loss, losses = train.train_step(cfg, sample, ds, model, opt, dev, batch_idx=it)
        assert set(losses) == {"recon_img_sv", "recon_mask_sv", "recon_img_mv", "recon_mask_mv"}
        assert abs(sum(losses.values()) - loss.item()) < 1e-4 * max(1.0, loss.item())
        first = first or loss.item()
    assert torch.isfinite(loss) and loss.item() < first


def test_pose_refinement_recovers_perturbed_poses(dev):
    """row f2 end to end: targets are the model's own renderings at the GT poses, the initial poses are perturbed by ~3 degrees /
    2 cm; a short refinement run (all-HIP forward + backward w.r.t. the 7-D poses) must reduce both the loss and the pose error."""
    from forge_amd import geo_utils, refine
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    sample = syn.make_sample(1, 3, 256, 1.5, seed=21)
    with torch.no_grad():
        feats = model.encoder_3d.get_feat3D(sample["images"][0].to(dev)).reshape(1, 3, 128, 32, 32, 32)
        gt7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][0, 1:]).to(dev)
        tgt_i, tgt_m, _, _, _ = refine._render_views(model, cfg, ds, feats, gt7, sample["K_cv2"].to(dev), dev)
    g = torch.Generator().manual_seed(3)
    init = gt7.clone()
    init[:, :4] = torch.nn.functional.normalize(init[:, :4] + 0.03 * torch.randn(2, 4, generator=g).to(dev))
    init[:, 4:] += 0.02 * torch.randn(2, 3, generator=g).to(dev)
    e0 = refine.pose_errors(init, sample["cam_poses_rel_cv2"][0, 1:].to(dev))
    out, hist, dt = refine.refine_poses(model, cfg, ds, feats, init, tgt_i, tgt_m, sample["K_cv2"], dev, iter_num=60, log_every=20)
    e1 = refine.pose_errors(out, sample["cam_poses_rel_cv2"][0, 1:].to(dev))
    assert hist[-1] < hist[0]
    assert e1[0].mean().item() < e0[0].mean().item() and e1[1].mean().item() < e0[1].mean().item()
    assert all(p.requires_grad for p in model.parameters())           # restored
    print("refinement: %.1f ms/iteration (t=3 views), rot err %.2f -> %.2f deg" % (dt * 1e3, e0[0].mean().item(), e1[0].mean().item()))


def test_refinement_pose_gradient_vs_oracle_autograd(dev):
    """End-to-end pin of row f2's objective: d loss / d (quaternion, translation) of the non-reference views through pose algebra ->
    rotate (affine gradient) -> view ordering -> fuse -> heads -> ray-march (camera gradient) -> conv_rgb, against autograd through
    the CPU oracle on the same features and weights. Stated tolerance: 2e-2 of the gradient's max magnitude."""
    from forge_amd import geo_utils, refine
    from forge_amd.model import FORGE, chose_selected, sequence_from_distance
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    w = syn.seeded_state_dict(model.state_dict(), 0)
    model.load_state_dict(w)
    model = model.to(dev).eval()
    for prm in model.parameters():
        prm.requires_grad_(False)
    ds = syn.SyntheticDataset(1.5)
    t = 3
    sample = syn.make_sample(1, t, 256, 1.5, seed=51)
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(1, t, 128, 32, 32, 32, generator=g) * 0.5
    pose7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][0, 1:t])
    pose7[:, :4] = torch.nn.functional.normalize(pose7[:, :4] + 0.02 * torch.randn(t - 1, 4, generator=g))
    tgt_i, tgt_m = torch.rand(t, 3, 256, 256, generator=g), torch.rand(t, 1, 256, 256, generator=g)
    K = sample["K_cv2"][:, :t]
    # HIP path
    ph = pose7.clone().to(dev).requires_grad_(True)
    imgs, masks, _, _, _ = refine._render_views(model, cfg, ds, feats.to(dev), ph, K.to(dev), dev)
    lh = 5.0 * torch.nn.functional.mse_loss(imgs, tgt_i.to(dev)) + torch.nn.functional.mse_loss(masks, tgt_m.to(dev))
    lh.backward()
    # oracle path (same pose algebra in torch on the CPU, then the oracle's stages)
    po = pose7.clone().requires_grad_(True)
    rel = geo_utils.quat2mat(po)
    can_p, can_e = ds.get_canonical_pose_cv2(device="cpu"), ds.get_canonical_extrinsics_cv2(device="cpu")
    poses = can_p.unsqueeze(0) @ rel
    extr = torch.inverse(poses)
    poses = torch.cat([can_p.reshape(1, 1, 4, 4), poses.reshape(1, t - 1, 4, 4)], dim=1)
    extr = torch.cat([can_e.reshape(1, 1, 4, 4), extr.reshape(1, t - 1, 4, 4)], dim=1).reshape(t, 4, 4)
    ft = fo.rotate_world(feats, poses, cfg.render.volume_size)
    ft = chose_selected(ft, sequence_from_distance(poses[:, :, :3, 3]))
    fm = fo.fuse(ft, w)
    dm, rm = fo.density_head(fm, w), fo.render_features_head(fm, w)
    rep = lambda v: v.repeat(t, 1, 1, 1, 1)
    oi, om = fo.vol_render(rep(rm), rep(dm), extr[:, :3, :3], extr[:, :3, 3], K.reshape(t, 3, 3), w, cfg.dataset.img_size,
                           cfg.render.n_pts_per_ray, cfg.render.min_depth, cfg.render.max_depth, cfg.render.volume_size, cfg.render.k_size)[:2]
    lo = 5.0 * torch.nn.functional.mse_loss(oi, tgt_i) + torch.nn.functional.mse_loss(om, tgt_m)
    lo.backward()
    assert abs(lh.item() - lo.item()) < 1e-4 * max(1.0, abs(lo.item()))
    err = (ph.grad.cpu() - po.grad).abs().max().item()
    assert err < 2e-2 * po.grad.abs().max().item(), (err, po.grad.abs().max().item())


def test_refinement_steps_vs_the_reference_do_refinement(dev, golden):
    """Row f2 against the REFERENCE's own loop: tests/golden/refine_steps.npz = kubric_eval.py:412-530 `do_refinement` run for three Adam steps on the reference FORGE
    model (oracle/make_golden.py::refine_goldens; the optimiser's step wrapped to record the gradients it is handed). Here: forge_amd.refine.PoseRefiner on the
    MI355X from the same initial poses.
      (a) per iteration, AT THE REFERENCE'S PARAMETERS of that iteration (torch's Adam replayed on the golden gradients), the gradient of the refinement loss w.r.t. the
          four quaternions and translations - through conv_rgb, the ray-marcher's d(R, T), both heads, the ConvGRU fusion's data gradients, rotate's d(pose), the
          pose chain: 1e-2 of each tensor's max, cosine > 0.9999 (measured <= 5.6e-3 / 1 - cos <= 3e-6);
      (b) free-running for the three steps (PoseRefiner's own Adam): parameters within 1e-4 of the reference's (measured 4.3e-5). The objective is piecewise smooth -
          two trilinear samplers - and its pose gradient is not: 4e-6 of parameter difference at the third iteration moves the gradient by 1.6e-2 of its max, which
          is why (a) pins the gradient at identical parameters."""
    from forge_amd import refine
    from forge_amd.model import FORGE
    g = golden("refine_steps")
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    cfg.loss.recon_rgb, cfg.loss.recon_mask = float(g["recon_rgb"]), float(g["recon_mask"])
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), int(g["weight_seed"])))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    sample = {k: v[:, :5].contiguous().to(dev) for k, v in syn.make_sample(1, 10, 256, 1.5, seed=int(g["sample_seed"])).items()}
    with torch.no_grad():
        feats = model.encoder_3d.get_feat3D(sample["images"][0]).reshape(1, 5, 128, 32, 32, 32)
    args = (model, cfg, ds, feats, T(g["init"]).to(dev), sample["images"][0], sample["fg_probabilities"][0], sample["K_cv2"], dev)
    frozen = refine._frozen(model)
    try:
        # (a) gradients at the reference's parameters
        r = refine.PoseRefiner(*args, use_graph=False)
        ref_rot, ref_tr = T(g["init"])[:, :4].clone().requires_grad_(True), T(g["init"])[:, 4:].clone().requires_grad_(True)
        ref_opt = torch.optim.Adam([{"params": ref_rot, "lr": 1e-3}, {"params": ref_tr, "lr": 5e-4}], lr=1e-3)          # kubric_eval.py:440-449
        for i in range(3):
            with torch.no_grad():
                r.rot.copy_(ref_rot.detach().to(dev))
                r.trans.copy_(ref_tr.detach().to(dev))
            r.eager_step()
            for name, got in (("grad_rot_%d" % i, r.rot.grad), ("grad_trans_%d" % i, r.trans.grad)):
                ref = T(g[name])
                err = (got.cpu() - ref).abs().max().item() / ref.abs().max().item()
                cos = torch.nn.functional.cosine_similarity(got.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
                if os.environ.get("FORGE_TEST_REPORT"):
                    print("  refinement %-14s err/max %.2e  1-cos %.2e" % (name, err, 1 - cos))
                assert err < 1e-2 and cos > 0.9999, (name, err, cos)
            ref_rot.grad, ref_tr.grad = T(g["grad_rot_%d" % i]).clone(), T(g["grad_trans_%d" % i]).clone()
            ref_opt.step()
        assert torch.equal(ref_rot.detach(), T(g["rot_after"])) and torch.equal(ref_tr.detach(), T(g["trans_after"]))    # the replay IS the reference's optimiser
        # (b) free-running
        r = refine.PoseRefiner(*args, use_graph=False)
        for _ in range(3):
            r.eager_step()
        torch.cuda.synchronize()
        assert (r.rot.detach().cpu() - T(g["rot_after"])).abs().max().item() < 1e-4
        assert (r.trans.detach().cpu() - T(g["trans_after"])).abs().max().item() < 1e-4
        ret = T(g["returned_poses"])
        want = torch.cat([torch.nn.functional.normalize(ret[:, :4]), ret[:, 4:]], dim=1)      # the reference returns the raw quaternion; toSE3 normalises it at every use
        assert (r.poses().cpu() - want).abs().max().item() < 1e-4
    finally:
        for p in frozen:
            p.requires_grad_(True)


def test_pose_chain_kernel_vs_torch_algebra(dev):
    """forge_pose_chain_fwd / _bwd (the refinement loop's pose algebra in one launch, Jacobian by forward-mode duals) against the torch algebra it
    replaces - F.normalize, geo_utils.quat2mat, canonical @ rel, inverse_affine, Rotate_world.get_transformation, VolRender._pack_cameras - in
    float64 on the CPU: values to 2e-6, the vector-Jacobian product for random upstream gradients to 1e-5 of its scale; un-normalised
    quaternions (the optimiser's raw parameter) and two scenes."""
    from forge_amd import geo_utils, ops
    ds = syn.SyntheticDataset(1.5)
    g = torch.Generator().manual_seed(9)
    b, t, e = 2, 4, 0.484375
    sample = syn.make_sample(b, t, 256, 1.5, seed=77)
    p7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][:, 1:].reshape(b * (t - 1), 4, 4))
    rot = (p7[:, :4] * (0.5 + torch.rand(b * (t - 1), 1, generator=g)) + 0.05 * torch.randn(b * (t - 1), 4, generator=g))     # NOT unit length
    trans = p7[:, 4:] + 0.02 * torch.randn(b * (t - 1), 3, generator=g)
    K = sample["K_cv2"]
    can_p, can_e = ds.get_canonical_pose_cv2(device="cpu"), ds.get_canonical_extrinsics_cv2(device="cpu")
    gxf, gcam = torch.randn(b * t, 12, generator=g), torch.randn(b * t, 16, generator=g)
    # float64 torch algebra
    r64, t64 = rot.double().requires_grad_(True), trans.double().requires_grad_(True)
    rel = geo_utils.quat2mat(torch.cat([torch.nn.functional.normalize(r64), t64], dim=1))
    poses = (can_p.double().unsqueeze(0) @ rel)
    extr = geo_utils.inverse_affine(poses).reshape(b, t - 1, 4, 4)
    poses_all = torch.cat([can_p.double().reshape(1, 1, 4, 4).repeat(b, 1, 1, 1), poses.reshape(b, t - 1, 4, 4)], dim=1)
    extr_all = torch.cat([can_e.double().reshape(1, 1, 4, 4).repeat(b, 1, 1, 1), extr], dim=1).reshape(b * t, 4, 4)
    T = poses_all[:, 0:1].repeat(1, t - 1, 1, 1).reshape(-1, 4, 4) @ geo_utils.inverse_affine(poses_all[:, 1:].reshape(-1, 4, 4))
    xf_ref = torch.cat([torch.zeros(b, 1, 12, dtype=torch.float64), torch.cat([T[:, :3, :3], T[:, :3, 3:4] / e], dim=-1).reshape(b, t - 1, 12)], dim=1).reshape(b * t, 12)
    Kh = K.double().reshape(b * t, 3, 3) / 2.0
    cam_ref = torch.cat([extr_all[:, :3, :3].reshape(b * t, 9), extr_all[:, :3, 3], Kh[:, 0, 0:1], Kh[:, 1, 1:2], Kh[:, 0, 2:3], Kh[:, 1, 2:3]], dim=1)
    ((xf_ref * gxf.double()).sum() + (cam_ref * gcam.double()).sum()).backward()
    # HIP
    rh, th = rot.to(dev).requires_grad_(True), trans.to(dev).requires_grad_(True)
    xf, cam, mode, slot, poses_h, origin = ops.pose_chain(rh, th, can_p.to(dev), can_e.to(dev), K.to(dev), e, b, t)
    ((xf * gxf.to(dev)).sum() + (cam * gcam.to(dev)).sum()).backward()
    assert (xf.detach().cpu().double() - xf_ref.detach()).abs().max().item() < 2e-6 * max(1.0, xf_ref.abs().max().item())
    assert (cam.detach().cpu().double() - cam_ref.detach()).abs().max().item() < 2e-6 * cam_ref.abs().max().item()
    assert (poses_h.cpu().double() - poses_all.detach()).abs().max().item() < 2e-6 * poses_all.abs().max().item()
    assert mode.cpu().tolist() == ([0] + [1] * (t - 1)) * b
    from forge_amd.model import sequence_from_distance
    order = sequence_from_distance(poses_h[:, :, :3, 3])                                      # out[:, j] = view order[:, j]  <=>  slot[view] = its rank
    want = torch.argsort(order, dim=1) + torch.arange(b, device=dev)[:, None] * t
    assert slot.cpu().tolist() == want.reshape(-1).cpu().tolist()
    org_ref = torch.stack([Kh[:, 0, 0] * extr_all[:, 0, 3] / extr_all[:, 2, 3] + Kh[:, 0, 2], Kh[:, 1, 1] * extr_all[:, 1, 3] / extr_all[:, 2, 3] + Kh[:, 1, 2]], dim=-1)
    assert (origin.cpu().double() - org_ref.detach()).abs().max().item() < 1e-4
    for got, ref in ((rh.grad, r64.grad), (th.grad, t64.grad)):
        assert (got.cpu().double() - ref).abs().max().item() < 1e-5 * ref.abs().max().item(), (got, ref)


def test_adam_small_kernel_follows_torch_adam(dev):
    """forge_adam_small (one launch per tensor, step count on the device) against torch.optim.Adam with the refinement loop's settings
    (kubric_eval.py:440-449: lr 1e-3 / 5e-4, default betas / eps) over 25 steps of random gradients: parameters to 1e-6."""
    from forge_amd import refine
    g = torch.Generator().manual_seed(1)
    p0, q0 = torch.randn(4, 4, generator=g), torch.randn(4, 3, generator=g)
    a, b = p0.clone().to(dev).requires_grad_(True), q0.clone().to(dev).requires_grad_(True)
    c, d = p0.clone().to(dev).requires_grad_(True), q0.clone().to(dev).requires_grad_(True)
    mine = refine._SmallAdam([(a, 1e-3), (b, 5e-4)])
    ref = torch.optim.Adam([{"params": c, "lr": 1e-3}, {"params": d, "lr": 5e-4}], lr=1e-3)
    for _ in range(25):
        ga, gb = torch.randn(4, 4, generator=g).to(dev), (torch.randn(4, 3, generator=g) * 10.0 ** float(torch.randint(-4, 3, (1,), generator=g))).to(dev)
        a.grad, b.grad, c.grad, d.grad = ga.clone(), gb.clone(), ga.clone(), gb.clone()
        mine.step()
        ref.step()
    assert (a - c).abs().max().item() < 1e-6 and (b - d).abs().max().item() < 1e-6
    assert float(mine.state[0][2]) == 25.0


def test_refinement_iteration_fused_pose_chain_equals_torch_pose_algebra(dev):
    """f2: the iteration PoseRefiner runs (ops.pose_chain -> warp affine + packed cameras) against the same iteration with the torch pose algebra
    (refine._render_views): rendered images / masks to 3e-4 of their scale (the two pose algebras differ by fp32 rounding, ~1e-7, which the warp's
    trilinear weights and five GRU steps amplify to ~6e-5), loss to 1e-5, pose gradients to 5e-3 of their max (the ray-march and rotate
    backward use fp32 atomics: two runs of ONE path differ by ~1e-4)."""
    from forge_amd import geo_utils, refine
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    refine._frozen(model)
    ds = syn.SyntheticDataset(1.5)
    t = 4
    sample = syn.make_sample(1, t, 256, 1.5, seed=33)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        feats = model.encoder_3d.get_feat3D(sample["images"][0].to(dev)).reshape(1, t, 128, 32, 32, 32)
        gt7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][0, 1:]).to(dev)
        tgt_i, tgt_m, _, _, _ = refine._render_views(model, cfg, ds, feats, gt7, sample["K_cv2"].to(dev), dev)
    init = gt7.clone()
    init[:, :4] = init[:, :4] * 1.3 + 0.03 * torch.randn(t - 1, 4, generator=g).to(dev)
    init[:, 4:] += 0.02 * torch.randn(t - 1, 3, generator=g).to(dev)
    res = {}
    for fused in (True, False):
        r = refine.PoseRefiner(model, cfg, ds, feats, init, tgt_i, tgt_m, sample["K_cv2"], dev, use_graph=False)
        can = r.canonical
        if fused:
            imgs, masks, _, origin, poses = refine._render_views_fused(model, cfg, ds, r.features, r.rot, r.trans, r.K, dev, can)
        else:
            pose7 = torch.cat([torch.nn.functional.normalize(r.rot), r.trans], dim=1)
            imgs, masks, _, origin, poses = refine._render_views(model, cfg, ds, r.features, pose7, r.K, dev, can)
        loss = r.w_rgb * torch.nn.functional.mse_loss(imgs, tgt_i) + r.w_mask * torch.nn.functional.mse_loss(masks, tgt_m)
        loss.backward()
        res[fused] = (imgs.detach(), masks.detach(), origin.detach(), poses.detach(), float(loss.detach()), r.rot.grad.clone(), r.trans.grad.clone())
    a, c = res[True], res[False]
    for i in range(4):
        assert (a[i] - c[i]).abs().max().item() < (3e-4 if i < 2 else 2e-6) * max(1.0, c[i].abs().max().item()), i
    assert abs(a[4] - c[4]) < 1e-5 * max(1.0, abs(c[4]))
    for i in (5, 6):
        assert (a[i] - c[i]).abs().max().item() < 5e-3 * c[i].abs().max().item(), (i, a[i], c[i])


def test_pose_refinement_graph_replay_matches_eager(dev):
    """f2: the refinement iteration captured into a hipGraph (forward, loss, backward through rotate / fuse / heads / ray-march, Adam)
    follows the same trajectory as the eager loop (atomics in the backward make the two runs differ in the last bits only)."""
    from forge_amd import geo_utils, refine
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    sample = syn.make_sample(1, 3, 256, 1.5, seed=41)
    with torch.no_grad():
        feats = model.encoder_3d.get_feat3D(sample["images"][0].to(dev)).reshape(1, 3, 128, 32, 32, 32)
        gt7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][0, 1:]).to(dev)
        tgt_i, tgt_m, _, _, _ = refine._render_views(model, cfg, ds, feats, gt7, sample["K_cv2"].to(dev), dev)
    g = torch.Generator().manual_seed(9)
    init = gt7.clone()
    init[:, :4] = torch.nn.functional.normalize(init[:, :4] + 0.03 * torch.randn(2, 4, generator=g).to(dev))
    init[:, 4:] += 0.02 * torch.randn(2, 3, generator=g).to(dev)
    runs = [refine.refine_poses(model, cfg, ds, feats, init, tgt_i, tgt_m, sample["K_cv2"], dev, iter_num=12, log_every=4, use_graph=ug)
            for ug in (False, True)]
    (pe, he, _), (pg, hg, _) = runs
    assert len(he) == len(hg) == 4
    # Adam normalises the gradient, so the last-bit noise of the fp32 atomics in the backward kernels can flip a near-zero gradient
    # component's direction: two runs (eager or not) drift apart by a fraction of lr = 1e-3 per step and component
    assert (pe - pg).abs().max().item() < 6e-3 and (pe - init).abs().max().item() > 5e-3
    assert abs(he[0] - hg[0]) < 1e-4 * max(1.0, abs(he[0]))                   # same starting point, same first forward
    for a, b in zip(he, hg):
        assert abs(a - b) < 3e-2 * max(1.0, abs(a))
    assert hg[-1] < hg[0]


def test_graphed_training_step_matches_eager(dev):
    """forge_amd.graph.GraphedStep: forward + loss + backward + gradient clipping + Adam of the GT-pose training step captured into
    one hipGraph; after the same number of optimisation steps the loss of the replayed graph follows the eager run (BatchNorm running
    statistics and Adam state are device tensors updated by the replay)."""
    import torch.nn.functional as F
    from forge_amd.graph import GraphedStep
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    ds = syn.SyntheticDataset(1.5)
    sample = {k: v.to(dev) for k, v in syn.make_sample(1, 5, 256, 1.5, seed=6).items()}
    tgt_i = sample["images"].repeat(1, 2, 1, 1, 1).reshape(-1, 3, 256, 256)
    tgt_m = sample["fg_probabilities"].repeat(1, 2, 1, 1, 1).reshape(-1, 1, 256, 256)

    def make():
        model = FORGE_poseEstimator3D(cfg)
        model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
        model = model.to(dev).train()
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, capturable=True)

        def step():
            imgs, masks = model(sample, ds, dev)
            loss = 5.0 * F.mse_loss(imgs, tgt_i) + F.mse_loss(masks, tgt_m)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
            opt.step()
            return loss.detach()
        return model, opt, step

    _, opt_e, step_e = make()
    eager = []
    for _ in range(4):
        opt_e.zero_grad(set_to_none=True)
        eager.append(step_e().item())
    _, opt_g, step_g = make()
    g = GraphedStep(step_g, opt_g, warmup=2)          # 2 eager steps, then every call replays one captured step
    graphed = [g().item() for _ in range(2)]
    assert eager[1] < eager[0]                                                       # the loss does move
    for a, b in zip(eager[2:], graphed):
        assert abs(a - b) < 5e-3 * abs(a), (eager, graphed)


def test_row_band_render_equals_full_render_rows(dev):
    """per-ray sharding building block: marching rows [h0,h1) with cy shifted by h0 reproduces those rows of the full render bit for bit."""
    from forge_amd import dist as fd
    feat, dens = syn.blob_volumes(1, 32, 16, seed=4)
    _, extr, _ = syn.orbit_cameras(4, 1.5, 15.0)
    Kh = fo.halve_intrinsics(syn.intrinsics(256)[None].repeat(4, 1, 1))
    cam = _cam_pack(extr[:, :3, :3], extr[:, :3, 3], Kh).to(dev)
    v2v = torch.zeros(4, dtype=torch.int32, device=dev)
    h = [fo.grid_half_extent(32, 1.0)] * 3
    full = ops.render_rays(feat.to(dev), dens.to(dev), cam, v2v, 128, 128, 64, 0.5, 2.0, h, True)
    for world in (2, 8):
        for rank in (0, world - 1):
            h0, h1 = fd.ray_band(128, rank, world)
            band = ops.render_rays(feat.to(dev), dens.to(dev), fd.band_cameras(cam, h0), v2v, h1 - h0, 128, 64, 0.5, 2.0, h, True)
            for a, b in zip(band, full):
                assert torch.equal(a, b[:, :, h0:h1])
    got = fd.render_rays_sharded(feat.to(dev), dens.to(dev), cam, v2v, 128, 128, 64, 0.5, 2.0, h, True)      # world size 1 path
    assert all(torch.equal(a, b) for a, b in zip(got, full))


def test_pose_refinement_two_instances_in_flight_match_sequential_runs(dev):
    """f2: refine_poses_many keeps two refinement problems in flight (one hipGraph + HIP stream each, replays issued round-robin); every
    instance follows the trajectory of its own sequential refine_poses run (Adam on atomics-noisy gradients: a fraction of lr per step)
    and both reduce their pose error."""
    from forge_amd import geo_utils, refine
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    problems, gts, inits = [], [], []
    for seed in (21, 22):
        sample = syn.make_sample(1, 3, 256, 1.5, seed=seed)
        with torch.no_grad():
            feats = model.encoder_3d.get_feat3D(sample["images"][0].to(dev)).reshape(1, 3, 128, 32, 32, 32)
            gt7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][0, 1:]).to(dev)
            tgt_i, tgt_m, _, _, _ = refine._render_views(model, cfg, ds, feats, gt7, sample["K_cv2"].to(dev), dev)
        g = torch.Generator().manual_seed(seed)
        init = gt7.clone()
        init[:, :4] = torch.nn.functional.normalize(init[:, :4] + 0.03 * torch.randn(2, 4, generator=g).to(dev))
        init[:, 4:] += 0.02 * torch.randn(2, 3, generator=g).to(dev)
        problems.append((feats, init, tgt_i.clone(), tgt_m.clone(), sample["K_cv2"]))
        gts.append(sample["cam_poses_rel_cv2"][0, 1:].to(dev))
        inits.append(init)
    n = 24
    many, dt = refine.refine_poses_many(model, cfg, ds, problems, dev, iter_num=n, depth=2)
    assert all(p.requires_grad for p in model.parameters())
    for pr, got, gt, init in zip(problems, many, gts, inits):
        seq, _, _ = refine.refine_poses(model, cfg, ds, *pr, dev, iter_num=n, use_graph=True)     # both entry points run iter_num + 1 optimiser steps (kubric_eval.py:450)
        assert (got - seq).abs().max().item() < 8e-3 and (got - init).abs().max().item() > 5e-3
        e0, e1 = refine.pose_errors(init, gt), refine.pose_errors(got, gt)
        assert e1[0].mean().item() < e0[0].mean().item()
    print("refinement, 2 instances in flight: %.2f ms per iteration and instance (t = 3 views)" % (dt * 1e3))


def test_loss_functions_match_reference_golden(dev):
    """f1: forge_amd.train's four loss functions against the values the REFERENCE's scripts/kubric_compute_loss.py produced on the same
    tensors through a stub model, on the MI355X: the MSE terms are csrc/loss.hip launches (train.grouped_mse) (tests/golden/loss_terms.npz, generated by oracle/make_golden.py)."""
    import types
    import numpy as np
    from forge_amd import train as tr
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_terms.npz"))
    T = lambda k: torch.from_numpy(gold[k]).to(dev)
    sample10 = {"images": T("images"), "fg_probabilities": T("fg")}
    sample5 = {k: v[:, :5].contiguous() for k, v in sample10.items()}
    pose = {"pred": T("pose_pred"), "gt": T("pose_gt")}
    cfg = types.SimpleNamespace(loss=types.SimpleNamespace(recon_rgb=float(gold["recon_rgb"]), recon_mask=float(gold["recon_mask"]),
                                                           perceptual_img=0.0, regu_origin_proj=float(gold["regu_origin_proj"])))
    cases = {
        "recon": (tr.compute_reconstruction_loss, sample5, lambda s, d, dev: (T("r_img"), T("r_msk"))),
        "pose": (tr.compute_pose_loss, sample5, lambda s, d, dev: (pose, T("origin"))),
        "all": (tr.compute_all_loss, sample5, lambda s, d, dev: (T("r_img"), T("r_msk"), T("origin"), pose)),
        "all_nvs": (tr.compute_all_loss_nvs, sample10, lambda s, d, dev: (T("r_img"), T("r_msk"), T("origin"), pose)),
    }
    for name, (fn, smp, model) in cases.items():
        loss, terms, _, _ = fn(cfg, 0, smp, None, model, {}, dev, None)
        assert abs(float(loss) - float(gold["total_" + name])) < 1e-5 * max(1.0, abs(float(gold["total_" + name]))), name
        ref_terms = {k.split("__", 1)[1]: float(gold[k]) for k in gold.files if k.startswith(name + "__")}
        assert set(terms) == set(ref_terms), (name, sorted(terms), sorted(ref_terms))
        for k, v in ref_terms.items():
            assert abs(terms[k] - v) < 1e-5 * max(1.0, abs(v)), (name, k)
    # a joint sample with another number of novel views (5 input + 3 novel): the same kernel, one group per call, against torch's own MSE
    import torch.nn.functional as Fn
    s8 = {k: v[:, :8].contiguous() for k, v in sample10.items()}
    nb = s8["images"].shape[0]
    r_img, r_msk = T("r_img").reshape(nb, 10, 3, *T("r_img").shape[-2:])[:, :8], T("r_msk").reshape(nb, 10, 1, *T("r_msk").shape[-2:])[:, :8]
    model8 = lambda s, d, dv: (r_img.reshape(nb * 8, 3, *r_img.shape[-2:]), r_msk.reshape(nb * 8, 1, *r_msk.shape[-2:]), T("origin"), pose)
    _, terms8, _, _ = tr.compute_all_loss_nvs(cfg, 0, s8, None, model8, {}, dev, None)
    want = {"recon_img": cfg.loss.recon_rgb * Fn.mse_loss(r_img[:, :5], s8["images"][:, :5]), "recon_img_nvs": cfg.loss.recon_rgb * Fn.mse_loss(r_img[:, 5:], s8["images"][:, 5:]),
            "recon_mask": cfg.loss.recon_mask * Fn.mse_loss(r_msk[:, :5], s8["fg_probabilities"][:, :5]),
            "recon_mask_nvs": cfg.loss.recon_mask * Fn.mse_loss(r_msk[:, 5:], s8["fg_probabilities"][:, 5:])}
    for k, v in want.items():
        assert abs(terms8[k] - float(v)) < 1e-5 * max(1.0, abs(float(v))), k
