"""GPU (-m gpu), round 2: the BASELINE configurations round 1 left unexercised, the analytic renderer KATs, the reference's
predicted-pose forward, checkpoint round trips and the ADVICE r1 regressions — all through the C-ABI.

  configs[2]  full HIP path, batch = 8 scenes, 64^3 render grid                   test_config2_batch8_*
  configs[3]  training step on 128^3-voxel scenes (64^3 feature grid)            test_config3_*
  configs[4]  joint 2D3D (predicted poses) + 128^3 voxel                          test_forge_joint_forward_vs_reference_golden, test_config4_*
"""
import os

import numpy as np
import pytest
import torch

import forge_oracle as fo
import kat_render
import stock_pose
from forge_amd import geo_utils, ops, synthetic as syn
from test_gpu_parity import assert_forward_close

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from forge_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _model(cls, dev, cfg=None, seed=0, train=False):
    cfg = cfg or syn.kubric_config()
    model = cls(cfg)
    w = syn.seeded_state_dict(model.state_dict(), seed)
    model.load_state_dict(w)
    model = model.to(dev)
    return (model.train() if train else model.eval()), w, cfg


# ------------------------------------------------------------------------------------------------------------- a6 analytic KATs
def test_render_analytic_kats_hip(dev):
    """forge_render_fwd against the analytic known answers of tests/kat_render.py (derived from the documented PyTorch3D contracts,
    not from the oracle or its shims): uniform slabs on cubic / anisotropic grids (x<->W, y<->H), single-voxel impulses under a
    rotated camera with fx != fy, cx != cy (hit pixel = OpenCV projection of the voxel centre), a depth sample exactly on a voxel."""
    for case in kat_render.cases():
        cam = case["cam"]
        D, H, W = case["dims"]
        s = case["vol"] / D
        half = (0.5 * (W - 1) * s, 0.5 * (H - 1) * s, 0.5 * (D - 1) * s)
        cam16 = torch.tensor(list(cam["R"].reshape(9)) + list(cam["T"]) + [cam["fx"], cam["fy"], cam["cx"], cam["cy"]], dtype=torch.float32)[None]
        feat = torch.from_numpy(case["feat"]).float()[None].to(dev)
        dens = torch.from_numpy(case["dens"]).float()[None, None].to(dev)
        of, oo, od = ops.render_rays(feat, dens, cam16.to(dev), torch.zeros(1, dtype=torch.int32, device=dev), case["Hr"], case["Wr"],
                                     case["S"], case["zmin"], case["zmax"], half, True)
        got = torch.cat([of, oo, od], dim=1)[0].permute(1, 2, 0).cpu().numpy()
        kat_render.check(case, got)


# ------------------------------------------------------------------------------------------------------------- a8 predicted poses
def test_forge_joint_forward_vs_reference_golden(dev, golden):
    """models/model.py:42-148 with use_gt_pose=False, eval mode: the REFERENCE's own output (tests/golden/forward_joint.npz) vs
    forge_amd.model.FORGE on the MI355X — pins pose_estimator_{2d,3d}.py, the pose head, the predicted-camera chain, the ordering by
    predicted translations and the HIP path behind them. Stated tolerance: poses 5e-4; images max-abs 5e-3 / PSNR > 55 dB (pose noise
    of 1e-4 moves the warp / the cameras by a fraction of a voxel on top of the usual ~70-layer fp32 noise)."""
    from forge_amd.model import FORGE
    g = golden("forward_joint")
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    model, _, _ = _model(FORGE, dev, cfg, int(g["weight_seed"]))
    sample = syn.make_sample(1, 10, 256, 1.5, seed=int(g["sample_seed"]))
    with torch.no_grad():
        imgs, masks, oproj, pose = model(sample, syn.SyntheticDataset(1.5), dev)
    assert (pose["pred"].cpu() - T(g["joint__pose_pred"])).abs().max().item() < 5e-4
    assert (pose["conf"].cpu() - T(g["joint__conf"])).abs().max().item() < 5e-4
    assert (pose["gt"].cpu() - T(g["joint__pose_gt"])).abs().max().item() < 1e-5
    assert (oproj.cpu() - T(g["joint__origin_proj"])).abs().max().item() < 2e-3
    ref_i, ref_m = T(g["joint__imgs_sub"]), T(g["joint__masks_sub"])
    assert (imgs.cpu()[:, :, ::4, ::4] - ref_i).abs().max().item() < 5e-3 and fo.psnr(imgs.cpu()[:, :, ::4, ::4], ref_i) > 55.0
    assert (masks.cpu()[:, :, ::4, ::4] - ref_m).abs().max().item() < 5e-3
    assert (imgs.cpu().mean(dim=(1, 2, 3)) - T(g["joint__imgs_mean"])).abs().max().item() < 2e-4
    # pose-only mode (models/model.py:98-114)
    model.config.train.parameter = "pose"
    with torch.no_grad():
        pose2, oproj2 = model(sample, syn.SyntheticDataset(1.5), dev)
    assert (pose2["pred"].cpu() - T(g["joint_pose__pose_pred"])).abs().max().item() < 5e-4
    assert (oproj2.cpu() - T(g["joint_pose__origin_proj"])).abs().max().item() < 2e-3


def test_pose3d_predicted_pose_forward_vs_reference_golden(dev, golden):
    """models/model_single_pose_estimator.py:26-138 with use_gt_pose=False (3-D pose estimator alone), eval mode, vs the reference."""
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    g = golden("forward_joint")
    model, _, _ = _model(FORGE_poseEstimator3D, dev, syn.kubric_config(use_gt_pose=False), int(g["pose3d_weight_seed"]))
    assert float(T(g["pose3d__masks_mean"]).mean()) > 0.1            # the golden scene is NOT empty: fuse -> heads -> render are exercised
    sample = {k: v[:, :5].contiguous() for k, v in syn.make_sample(1, 10, 256, 1.5, seed=int(g["sample_seed"])).items()}
    with torch.no_grad():
        imgs, masks, oproj, pose = model(sample, syn.SyntheticDataset(1.5), dev)
    assert (pose["pred"].cpu() - T(g["pose3d__pose_pred"])).abs().max().item() < 5e-4
    assert (pose["conf"].cpu() - T(g["pose3d__conf"])).abs().max().item() < 5e-4
    assert (oproj.cpu() - T(g["pose3d__origin_proj"])).abs().max().item() < 2e-3
    # seed-3 weights render intensities up to 3.7 (conv_rgb's ReLU is unbounded above): bounds relative to the image scale - max-abs 5e-3,
    # 99.9 % of the sub-sampled pixels within 2e-3 (measured: 2.8e-3 / 9e-4 of the scale, 70.9 dB; predicted poses agree to 1e-5)
    ref_i, ref_m = T(g["pose3d__imgs_sub"]), T(g["pose3d__masks_sub"])
    scale = max(1.0, ref_i.abs().max().item())
    di, dm = (imgs.cpu()[:, :, ::4, ::4] - ref_i).abs(), (masks.cpu()[:, :, ::4, ::4] - ref_m).abs()
    stats = (di.max().item(), torch.quantile(di.flatten(), 0.999).item(), fo.psnr(imgs.cpu()[:, :, ::4, ::4], ref_i), dm.max().item(), scale)
    assert stats[0] < 5e-3 * scale and stats[1] < 2e-3 * scale and stats[2] > 60.0 and stats[3] < 5e-3, stats
    assert (imgs.cpu().mean(dim=(1, 2, 3)) - T(g["pose3d__imgs_mean"])).abs().max().item() < 2e-4 * scale, stats


# ------------------------------------------------------------------------------------------------------------- configs[4] training step
def joint_training_step(dev, cfg=None, weight_seed=0, sample_seed=12, features_recon=None):
    """One joint 2D3D fine-tune iteration up to the gradients (kubric_train_joint.py:111-141 -> compute_all_loss_nvs -> backward): FORGE with
    predicted poses in train mode, BatchNorm on running statistics and Dropout off as in the golden, the stock-torch pose networks pinned to
    their deterministic backward algorithms (tests/test_gpu_ddp.py::_joint_step explains why). Returns (loss, terms, model, imgs, masks)."""
    from forge_amd import train
    from forge_amd.model import FORGE
    cfg = cfg or syn.kubric_config(use_gt_pose=False, parameter="joint")
    det = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        model = FORGE(cfg)
        model.load_state_dict(syn.seeded_state_dict(model.state_dict(), weight_seed))
        model = model.to(dev).train()
        for m in model.modules():
            if isinstance(m, (torch.nn.modules.batchnorm._BatchNorm, torch.nn.Dropout)):
                m.eval()
        sample = {k: v.to(dev) for k, v in syn.make_sample(1, 10, 256, 1.5, seed=sample_seed).items()}
        if features_recon is not None:
            sample["features_recon"] = features_recon                      # rides in the sample (what a DDP-wrapped model can be given)
        loss, terms, imgs, masks = train.compute_all_loss_nvs(cfg, 0, sample, syn.SyntheticDataset(1.5), model, {}, dev)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det
    return loss.detach(), terms, model, imgs.detach(), masks.detach()


class _StageView:
    """One stage of tests/golden/train_stages.npz as a fixture of its own: `files` / item access with the stage prefix stripped."""

    def __init__(self, g, stage):
        self.g, self.pre = g, stage + "__"
        self.files = [k[len(self.pre):] for k in g.files if k.startswith(self.pre)]

    def __getitem__(self, k):
        return self.g[self.pre + k]


@pytest.mark.parametrize("stage", ["pose3d_joint", "pose3d_pose", "joint_pose"])
def test_remaining_training_stages_vs_reference_golden(dev, golden, stage):
    """The reference trains in five stages; the GT-pose stage and the joint 2D3D stage are pinned by train_pose3d.npz / train_joint.npz, these are the other
    three, each = the reference's OWN loss function on its own model class + backward (tests/golden/train_stages.npz, oracle/make_golden.py::stage_goldens;
    fp32 and float64; BatchNorm on running statistics, Dropout off):
      pose3d_joint  compute_all_loss  on FORGE_poseEstimator3D(use_gt_pose=False, 'joint')  (joint_pose_3d.yaml; kubric_train_pose_3D.py:95-96): 2t views rendered
                    from the 3-D estimator's predicted cameras, four reconstruction terms + pose + translation + origin regulariser
      pose3d_pose   compute_pose_loss on the same model in 'pose' mode (pred_pose_3d.yaml): pose + translation MSE, nothing rendered
      joint_pose    compute_pose_loss on FORGE(use_gt_pose=False, 'pose') (pred_pose_2d3d.yaml / pretrain_pose_2d3d.yaml): both estimators + pose head
    Loss terms to 2e-5 of their float64 value; gradients against the float64 evaluation within 3x the reference's own fp32 distance + 1e-3 of each tensor's max (the
    pose-only stages are so well conditioned that the reference's fp32 run sits 1e-6 from float64 - there the floor is the bound: fp32 convolution chains of two
    ResNet-50s and the 3-D estimator, Winograd launches included, agree with float64 to 1e-4 .. 6e-4)."""
    from forge_amd import train
    from forge_amd.model import FORGE
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    allg = golden("train_stages")
    g = _StageView(allg, stage)
    cls, parameter, loss_fn, views, wseed = {"pose3d_joint": (FORGE_poseEstimator3D, "joint", train.compute_all_loss, 5, int(allg["pose3d_weight_seed"])),
                                             "pose3d_pose": (FORGE_poseEstimator3D, "pose", train.compute_pose_loss, 5, int(allg["pose3d_weight_seed"])),
                                             "joint_pose": (FORGE, "pose", train.compute_pose_loss, 10, int(allg["joint_weight_seed"]))}[stage]
    cfg = syn.kubric_config(use_gt_pose=False, parameter=parameter)
    cfg.loss.recon_rgb, cfg.loss.recon_mask, cfg.loss.regu_origin_proj = float(allg["recon_rgb"]), float(allg["recon_mask"]), float(allg["regu_origin_proj"])
    det = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        model = cls(cfg)
        model.load_state_dict(syn.seeded_state_dict(model.state_dict(), wseed))
        model = model.to(dev).train()
        for m in model.modules():
            if isinstance(m, (torch.nn.modules.batchnorm._BatchNorm, torch.nn.Dropout)):
                m.eval()
        sample = {k: v[:, :views].contiguous().to(dev) for k, v in syn.make_sample(1, 10, 256, 1.5, seed=int(allg["sample_seed"])).items()}
        loss, terms, _, _ = loss_fn(cfg, 0, sample, syn.SyntheticDataset(1.5), model, {}, dev)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det
    assert abs(loss.item() - float(g["loss64"])) < 2e-5 * abs(float(g["loss64"])), (loss.item(), float(g["loss64"]), float(g["loss"]))
    tkeys = [k[len("term64__"):] for k in g.files if k.startswith("term64__")]
    assert sorted(terms) == sorted(tkeys), (sorted(terms), sorted(tkeys))
    for k in tkeys:
        ref = float(g["term64__" + k])
        assert abs(terms[k] - ref) < 2e-5 * max(abs(ref), 0.1), (k, terms[k], ref)
    # floor: 1e-3 of each tensor's max; 3e-3 for the FORGE pose stage, whose loss reaches the encoder only through the 3-D estimator's d input - a max-abs
    # metric over two ReLU / LeakyReLU chains (ResNet trunk, estimator): single mask flips at pre-activations within fp32 noise of zero put isolated
    # per-channel outliers of 1-2.5e-3 on the BatchNorm-weight gradients there (1 - cos stays < 1e-6), with any fp32 implementation whose forward is not
    # bit-identical to the reference's (round 6 A/B of the eval-mode BatchNorm kernels against the torch module: profiles/r06_eval_bn_ab.txt)
    n = check_gradients_vs_float64_golden(g, dict(model.named_parameters()), factor=3.0, floor=3e-3 if stage == "joint_pose" else 1e-3)
    assert n == len([k for k in g.files if k.startswith("g64err__")]) >= 9


def test_config4_joint_step_on_the_128_cube_grid_end_to_end(dev):
    """BASELINE configs[4] END TO END at its 128^3-voxel grid (until round 5 only the pieces ran at that size): the joint 2D3D
    fine-tune iteration with 5 synthetic [128, 64^3] feature volumes entering rotate(D = 64) -> ConvGRU fusion at M = 262144 -> heads -> a 128^3 x 17
    volume -> 10 ray-marched views, pose networks on their native inputs, compute_all_loss_nvs, backward through the pose chain. Checked: the 128^3
    volume really is what is rendered (the heads' output shape), every sub-network receives a finite, non-zero gradient, the gradient reaching the
    synthetic feature volumes is non-zero for all five views, and a second evaluation reproduces the step to 2e-5 (relative L2; the weight
    gradients' fp32 atomics are the only run-to-run difference)."""
    seen = {}
    from forge_amd.encoder import Encoder3D
    orig = Encoder3D.heads

    def spy(self, z):
        out = orig(self, z)
        seen["z"], seen["feat"], seen["dens"] = tuple(z.shape), tuple(out[0].shape), tuple(out[1].shape)
        return out
    keys = ["pose_head.4.weight", "encoder_traj.pose_head_1.3.weight", "encoder_traj_2d.conv.9.weight", "encoder_3d.fusion_feature.cells.0.out_gate.weight",
            "encoder_3d.features_head.0.weight", "encoder_3d.density_head.6.weight", "render.conv_rgb.6.weight"]
    runs = []
    Encoder3D.heads = spy
    try:
        for _ in range(2):
            gen = torch.Generator(device=dev).manual_seed(79)
            f64 = torch.randn(1, 5, 128, 64, 64, 64, device=dev, generator=gen).mul_(0.5).permute(0, 1, 3, 4, 5, 2).contiguous().permute(0, 1, 5, 2, 3, 4).requires_grad_(True)
            loss, terms, model, imgs, masks = joint_training_step(dev, features_recon=f64)
            named = dict(model.named_parameters())
            runs.append((loss.item(), {k: named[k].grad.detach().clone() for k in keys}, f64.grad.detach().clone()))
            del model
    finally:
        Encoder3D.heads = orig
    assert seen == {"z": (1, 128, 64, 64, 64), "feat": (1, 16, 128, 128, 128), "dens": (1, 1, 128, 128, 128)}, seen
    assert imgs.shape == (1, 10, 3, 256, 256) and masks.shape == (1, 10, 1, 256, 256)
    (la, ga, fa), (lb, gb, fb) = runs
    assert torch.isfinite(torch.tensor(la)) and abs(la - lb) <= 1e-6 * abs(la)
    for k in keys:
        assert torch.isfinite(ga[k]).all() and ga[k].abs().max().item() > 0, k
        assert ((ga[k] - gb[k]).norm() / ga[k].norm()).item() < 2e-5, k
    per_view = fa.abs().amax(dim=(0, 2, 3, 4, 5))
    assert torch.isfinite(fa).all() and (per_view > 0).all(), per_view          # the pose chain AND the reconstruction reach every view's volume
    assert ((fa - fb).norm() / fa.norm()).item() < 2e-5


def grad_distance(got, ref):
    """(max |got - ref| / max |ref|, 1 - cos) of two gradient tensors, in float64."""
    a, b = got.double().flatten(), ref.double().flatten()
    cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item() if a.numel() > 1 else 1.0
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300), 1.0 - cos


def check_gradients_vs_float64_golden(g, named, factor, floor=3e-4, report=None):
    """The float64-referenced gradient bound. The fixtures carry, per key, the REFERENCE's float64 gradient (grad64__ /
    gsub64__: the same graph evaluated in double by oracle/make_golden.py) and how far the reference's own fp32 gradient sits from it
    (g64err__ / g64cos__, on the stored sample g64suberr__ / g64subcos__). Asserted per key:
        err(HIP, f64) <= factor * err(ref fp32, f64) + floor          (both as max-abs / max |g64|)
        1 - cos(HIP, f64) <= factor^2 * (1 - cos(ref fp32, f64)) + 1e-6
    `floor`: 3e-4 of the tensor's max - bias / BatchNorm-weight gradients are sums of 1e5..1e6 fp32 terms, where a different summation order
    alone moves the result by 1e-4 (40x below the 1e-2 band this bound replaces). Keys whose float64 gradient is exactly cancellation
    (|g64| < 1e-6 of the largest gradient: biases in front of a train-mode BatchNorm) are skipped."""
    keys = [k[len("g64err__"):] for k in g.files if k.startswith("g64err__")]
    scale = max(float(np.abs(g["grad64__" + k] if "grad64__" + k in g.files else g["gsub64__" + k]).max()) for k in keys)
    bad, rows = [], []
    for k in keys:
        got = named[k].grad
        assert got is not None, k
        flat = got.detach().flatten().cpu()
        if "gsub64__" + k in g.files:
            flat, ref64 = flat[::int(g["gstride__" + k])], T(g["gsub64__" + k])
            e32, c32 = float(g["g64suberr__" + k]), float(g["g64subcos__" + k])
        else:
            ref64 = T(g["grad64__" + k]).flatten()
            e32, c32 = float(g["g64err__" + k]), float(g["g64cos__" + k])
        if float(ref64.abs().max()) < 1e-6 * scale:
            continue
        e, c = grad_distance(flat, ref64)
        rows.append((k, e, c, e32, c32))
        if not (e <= factor * e32 + floor and c <= factor * factor * c32 + 1e-6):
            bad.append((k, e, e32, c, c32))
    if report is not None:
        report.extend(rows)
    if os.environ.get("FORGE_TEST_REPORT"):
        for k, e, c, e32, c32 in rows:
            print("  %-64s hip/f64 %.2e (1-cos %.1e)  ref32/f64 %.2e (1-cos %.1e)  ratio %.2f" % (k[-64:], e, c, e32, c32, e / max(e32, 1e-12)))
    assert not bad, bad
    return len(rows)


def test_joint_training_step_vs_reference_golden(dev, golden):
    """BASELINE configs[4] / VERDICT r4 item 1: the joint fine-tune iteration against the REFERENCE's own run of it
    (tests/golden/train_joint.npz = scripts/kubric_compute_loss.py:121-172 `compute_all_loss_nvs` on models/model.py:18-148 `FORGE` with predicted
    poses + backward, made in the build container by oracle/make_golden.py::train_joint_goldens, in fp32 AND in float64): the seven loss terms,
    the rendered maps, and the gradients of the pose head, both pose estimators (stock torch, fed by rotate's d(pose) and the ray-marcher's
    d(R, T) through toSE3), the trunk, conv1, both GRU gates, both heads and conv_rgb.
    Bounds: loss / terms 2e-5 relative to the float64 value (the reference's fp32 loss is 8e-7 from it); gradients against the float64
    evaluation within 3x the distance of the reference's own fp32 run (measured <= 2.2x, most keys < 1.3x: tools/debug/train_grad_margins.py),
    and within 2e-2 of each tensor's max of the reference's fp32 gradients (two fp32 evaluations of the pose chain sit 0.5-1.5e-2 from float64
    each: the unscaled 4096-token attention of the 3-D pose estimator amplifies rounding)."""
    g = golden("train_joint")
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    cfg.loss.recon_rgb, cfg.loss.recon_mask, cfg.loss.regu_origin_proj = float(g["recon_rgb"]), float(g["recon_mask"]), float(g["regu_origin_proj"])
    loss, terms, model, imgs, masks = joint_training_step(dev, cfg, int(g["weight_seed"]), int(g["sample_seed"]))
    assert float(T(g["masks_mean"]).mean()) > 0.1                      # the scene is in view of the predicted cameras: every stage carries gradient
    assert abs(loss.item() - float(g["loss64"])) < 2e-5 * abs(float(g["loss64"])), (loss.item(), float(g["loss64"]), float(g["loss"]))
    for k in ("recon_img", "recon_mask", "recon_img_nvs", "recon_mask_nvs", "pose", "trans", "regu_origin"):
        ref = float(g["term64__" + k])
        assert abs(terms[k] - ref) < 2e-5 * max(abs(ref), 0.1), (k, terms[k], ref, float(g["term__" + k]))
    assert (imgs[0, :, :, ::16, ::16].cpu() - T(g["imgs_sub"])).abs().max().item() < 2e-3
    assert (masks[0, :, :, ::16, ::16].cpu() - T(g["masks_sub"])).abs().max().item() < 2e-3
    named = dict(model.named_parameters())
    assert check_gradients_vs_float64_golden(g, named, factor=3.0) >= 29
    for k in [k[len("gnorm__"):] for k in g.files if k.startswith("gnorm__")]:
        flat = named[k].grad.detach().flatten().cpu()
        if "grad__" + k in g.files:
            ref = T(g["grad__" + k]).flatten()
        else:                                                          # the whole tensor through its norm, the stored sample element-wise
            assert abs(float(flat.double().norm()) - float(g["gnorm__" + k])) < 1e-2 * float(g["gnorm__" + k]), (k, float(flat.double().norm()), float(g["gnorm__" + k]))
            ref, flat = T(g["gsub__" + k]), flat[::int(g["gstride__" + k])]
        assert (flat - ref).abs().max().item() < 2e-2 * float(g["gmax__" + k]), k
    # parameters the reference's joint step leaves without a gradient stay without one here (find_unused_parameters=True territory)
    for k in ("encoder_traj.out.0.weight", "encoder_traj_2d.out.0.weight", "rotate.conv3d_1.weight"):
        assert named[k].grad is None or float(named[k].grad.abs().max()) == 0.0, k


def test_pose_estimators_hip_convolutions_vs_float64_and_stock_torch(dev):
    """Round 5: on the MI355X the 3-D pose estimator's eight 3x3x3 convolutions (+ BatchNorm + LeakyReLU) and the 2-D pose estimator's four stride-2
    convolutions run on libforge_hip.so instead of MIOpen's naive fp32 kernels (164 + 21 ms of the 256 ms joint step). Both modules, train mode
    (BatchNorm batch statistics) and eval mode, forward features + gradients of the input and of a parameter from every block, against the SAME
    module evaluated in float64 on the CPU - and, as the yardstick, the stock-torch path on the GPU against the same float64 result
    (tools/stock_pose.py): the HIP path has to stay within 3x the stock path's distance (+ 2e-5 of max) in eval mode and within 4x (+ 1e-3) in train
    mode, where the last BatchNorm layers normalise over 2-16 values per channel and amplify any rounding difference chaotically (both paths
    sit 0.3-2e-2 from float64 there). Round 6: eval-mode gradients take the train-mode form of the bound too (single activation-mask flips, see below;
    MIOpen's per-process solver choice moves the stock yardstick itself between 3e-5 and 1e-3 on the same key). The stock distance is the MEDIAN of
    STOCK_RUNS evaluations: in train mode one stock evaluation differs from the next in the same process (MIOpen's kernels do not round
    reproducibly, and the chaotic BatchNorm layers amplify that) - PoseEstimator2D's conv.1.weight gradient drew 2.2e-3 in one process and
    6.0e-3 .. 1.3e-2 in ten evaluations of two others, while the HIP path sat at 9.9e-3 from float64 in every one."""
    import copy
    import statistics
    from forge_amd.pose_estimator_2d import PoseEstimator2D
    from forge_amd.pose_estimator_3d import PoseEstimator3D
    STOCK_RUNS = 5
    torch.manual_seed(3)
    rel = lambda got, want: (got.detach().double().cpu() - want.detach()).abs().max().item() / max(want.detach().abs().max().item(), 1e-30)

    def run(mod, x, keys, stock=False):
        x = x.clone().requires_grad_(True)
        out = (stock_pose.stock_forward(mod) if stock else mod)(x, return_features=True)
        out.square().sum().backward()
        named = dict(mod.named_parameters())
        res = [out.detach(), x.grad] + [named[k].grad for k in keys]
        for p in mod.parameters():
            p.grad = None
        return res

    cases = [
        (PoseEstimator3D(syn.kubric_config()), (torch.randn(1, 3, 128, 32, 32, 32) * 0.5),
         ["conv3d_1.0.weight", "conv3d_1.3.bias", "conv3d_2.3.weight", "conv3d_3.1.weight", "conv3d_3.3.weight", "pose_head_1.0.weight", "pose_head_1.3.weight",
          "pose_transformer.self_transformer.mlp.fc1.weight"]),
        (PoseEstimator2D(), torch.rand(1, 3, 3, 256, 256), ["conv.0.weight", "conv.1.weight", "conv.3.weight", "conv.6.bias", "conv.9.weight",
                                                            "self_attn_blks.2.mlp.mlp.1.weight", "backbone.layer4.0.0.conv2.weight"]),
    ]
    for mod, x, keys in cases:
        sd = syn.seeded_state_dict({"m." + k: v for k, v in mod.state_dict().items()}, 11)
        mod.load_state_dict({k[2:]: v for k, v in sd.items()})
        for train in (True, False):
            mod.train(train)
            for m in mod.modules():                                        # Dropout off: three evaluations must be comparable
                if isinstance(m, torch.nn.Dropout):
                    m.eval()
            ref_mod = copy.deepcopy(mod).double()
            for m in ref_mod.modules():
                for k, v in list(vars(m).items()):
                    if torch.is_tensor(v) and v.is_floating_point():
                        setattr(m, k, v.double())
            ref = run(ref_mod, x.double(), keys, stock=True)
            g = copy.deepcopy(mod).to(dev)
            hip = run(g, x.to(dev), keys)
            stocks = [run(copy.deepcopy(mod).to(dev), x.to(dev), keys, stock=True) for _ in range(STOCK_RUNS)]
            for i, (name, a, r) in enumerate(zip(["features", "d input"] + keys, hip, ref)):
                if a is None and name == "d input" and isinstance(mod, PoseEstimator2D):
                    continue                                               # the HIP stem gathers its patches from the detached image: no d(image), as in the encoder's trunk
                eh, es = rel(a, r), statistics.median(rel(st[i], r) for st in stocks)
                if os.environ.get("FORGE_TEST_REPORT"):
                    print("  %-16s %-5s %-52s hip/f64 %.2e  stock/f64 %.2e" % (type(mod).__name__, "train" if train else "eval", name, eh, es))
                # features: the tight eval bound. Gradients: max-abs of a chain with LeakyReLU / ReLU masks - ONE pre-activation within fp32 noise of zero
                # flips its mask and moves a localised gradient entry by its full value, whichever fp32 implementation runs (round 6: the same module, the
                # same weights, another input: HIP and torch BatchNorm paths both 5e-3 from float64 on d input; stock torch itself sits 1.3e-3 away here,
                # profiles/r06_eval_bn_ab.txt) - so both modes get the stock distance x 4 + 1e-3 of the tensor's max
                bound = 3.0 * es + 2e-5 if (name == "features" and not train) else 4.0 * es + 1e-3
                assert eh <= bound, (type(mod).__name__, train, name, eh, es)


def test_pose_estimators_inference_schedule_vs_float64_stock_torch_and_autograd_path(dev):
    """forge_amd/frozen.py: under torch.no_grad() in eval mode (kubric_eval.py predict_initial, demo.py) both pose estimators launch every
    convolution once with bias + folded BatchNorm + residual + LeakyReLU in the GEMM epilogue. Features against the same module in float64 on the
    CPU with the stock-torch GPU path as the yardstick (within 3x its distance + 2e-5 of max), against the autograd path of the same weights (a
    different summation order only), and: a BatchNorm left in train mode keeps the autograd path's launches and batch statistics; an in-place parameter update
    (an optimizer step's version bump) is seen by the cached launch arguments."""
    import copy
    from forge_amd import frozen as fz
    from forge_amd.pose_estimator_2d import PoseEstimator2D
    from forge_amd.pose_estimator_3d import PoseEstimator3D
    torch.manual_seed(5)
    rel = lambda got, want: (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item() / max(want.detach().abs().max().item(), 1e-30)
    cases = [(PoseEstimator3D(syn.kubric_config()), torch.randn(2, 3, 128, 32, 32, 32) * 0.5, "conv3d_2"),
             (PoseEstimator2D(), torch.rand(1, 4, 3, 256, 256), "conv")]
    for mod, x, blk in cases:
        sd = syn.seeded_state_dict({"m." + k: v for k, v in mod.state_dict().items()}, 13)
        mod.load_state_dict({k[2:]: v for k, v in sd.items()})
        mod.eval()
        ref_mod = copy.deepcopy(mod).double()
        for m in ref_mod.modules():
            for k, v in list(vars(m).items()):
                if torch.is_tensor(v) and v.is_floating_point():
                    setattr(m, k, v.double())
        with torch.no_grad():
            ref = stock_pose.stock_forward(ref_mod)(x.double(), return_features=True)
        g = copy.deepcopy(mod).to(dev)
        xd = x.to(dev)
        assert fz.frozen_ok(xd, g) is False                                  # autograd on: not the inference schedule
        with torch.no_grad():
            assert fz.frozen_ok(xd, g)
            fro = g(xd, return_features=True)
        auto = g(xd, return_features=True)                                   # grad mode: convops.conv*_rows + bn_act_rows
        g2 = copy.deepcopy(mod).to(dev)
        with torch.no_grad():
            stock = stock_pose.stock_forward(g2)(xd, return_features=True)
        ef, es, ea = rel(fro, ref), rel(stock, ref), rel(fro, auto)
        if os.environ.get("FORGE_TEST_REPORT"):
            print("  %-16s inference schedule/f64 %.2e  stock/f64 %.2e  schedule/autograd path %.2e" % (type(mod).__name__, ef, es, ea))
        assert ef <= 3.0 * es + 2e-5, (type(mod).__name__, ef, es)
        assert ea <= 2e-4, (type(mod).__name__, ea)
        # cached launch arguments follow an in-place parameter update
        with torch.no_grad():
            first = [p for n_, p in g.named_parameters() if n_.startswith(blk) and p.dim() > 1][0]
            first.mul_(1.5)
            fro2, = [g(xd, return_features=True)]
        auto2 = g(xd, return_features=True)
        assert rel(fro2, auto2) <= 2e-4 and rel(fro2, fro) > 1e-3, (type(mod).__name__, rel(fro2, auto2), rel(fro2, fro))
        # one BatchNorm in train mode: batch statistics, i.e. the autograd path's launches
        bn = [m for m in getattr(g, blk).modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)][0]
        bn.train()
        bn.momentum = 0.0                                                    # running statistics untouched between the two evaluations
        with torch.no_grad():
            assert not fz.frozen_ok(xd, g)
            mixed = g(xd, return_features=True)
        assert rel(mixed, g(xd, return_features=True)) <= 2e-5 and rel(mixed, fro2) > 1e-3


# ------------------------------------------------------------------------------------------------------------- configs[2]
def test_config2_batch8_vs_oracle_and_per_scene_bit_equality(dev, monkeypatch):
    """BASELINE configs[2]: full HIP path, batch = 8 scenes, 64^3 render grid, 1 GPU. Scenes 2 and 5 of the batch against the CPU
    oracle; every scene of the batch equals the same scene run alone (b = 1) up to fp32 summation order under the default launch
    plan (the plan model may pick another tile / split-K factor for another M), and BIT FOR BIT when both runs are pinned to one
    plan (convops.force_plan): the batch only changes M, never the per-row arithmetic."""
    from forge_amd.model import FORGE
    model, w, cfg = _model(FORGE, dev)
    ds = syn.SyntheticDataset(1.5)
    sample = syn.make_sample(8, 5, 256, 1.5, seed=31)
    with torch.no_grad():
        imgs, masks = model(sample, ds, dev)
    assert imgs.shape == (40, 3, 256, 256) and masks.shape == (40, 1, 256, 256)
    imgs, masks = imgs.cpu().reshape(8, 5, 3, 256, 256), masks.cpu().reshape(8, 5, 1, 256, 256)
    for s in (2, 5):
        one = {k: v[s:s + 1] for k, v in sample.items()}
        with torch.no_grad():
            oi, om = fo.forward_hot_path(one["images"], one["cam_poses_cv2_canonicalized"], one["cam_extrinsics_cv2_canonicalized"],
                                         one["K_cv2"], w, cfg, order_by_distance=True)
        assert_forward_close(imgs[s], oi, masks[s], om, "configs[2] scene %d of 8" % s)
    worst = 0.0
    for s in range(8):
        one = {k: v[s:s + 1].contiguous() for k, v in sample.items()}
        with torch.no_grad():
            i1, m1 = model(one, ds, dev)
        worst = max(worst, (i1.cpu() - imgs[s]).abs().max().item(), (m1.cpu() - masks[s]).abs().max().item())
    # different M -> possibly different tile / split-K plans -> different fp32 summation orders: equality up to rounding, stated
    assert worst < 2e-4, worst
    from forge_amd import convops as co_
    monkeypatch.setattr(co_.STATE, "plan_override", ("D", 1))
    with torch.no_grad():
        pi, pm = model(sample, ds, dev)
        pi, pm = pi.reshape(8, 5, 3, 256, 256).clone(), pm.reshape(8, 5, 1, 256, 256).clone()
        for s in range(8):
            i1, m1 = model({k: v[s:s + 1].contiguous() for k, v in sample.items()}, ds, dev)
            assert torch.equal(i1, pi[s]) and torch.equal(m1, pm[s]), s


def test_config2_batch8_graph_replay_equals_eager(dev):
    """The bench's launch mode at b = 8: hipGraph replay == eager launch, bit for bit."""
    from forge_amd.graph import GraphedForward
    from forge_amd.model import FORGE
    model, _, _ = _model(FORGE, dev)
    ds = syn.SyntheticDataset(1.5)
    sample = {k: v.to(dev) for k, v in syn.make_sample(8, 5, 256, 1.5, seed=32).items()}
    with torch.no_grad():
        ei, em = model(sample, ds, dev)
    g = GraphedForward(model, sample, ds, dev)
    gi, gm = g(sample)
    assert torch.equal(ei, gi) and torch.equal(em, gm)


# ------------------------------------------------------------------------------------------------------------- 128^3-voxel configs
def _grid64_inputs(t, seed, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(1, t, 128, 64, 64, 64, generator=g) * scale
    jit = (torch.rand(10, 2, generator=g) - 0.5) * 0.3
    poses, extr, _ = syn.orbit_cameras(10, 1.5, 12.0, jit)
    return feats, poses, extr


def test_config4_grid64_stages_vs_oracle_crops(dev):
    """128^3-voxel path (models/rotate.py:115-117: 64^3 feature grid -> heads -> 128^3 render volume) stage by stage on synthetic
    [1,3,128,64^3] feature volumes: rotate(D=64) vs the oracle on a channel slice; ConvGRU fusion at M = 262144 vs the oracle on a
    40^3 crop (interior 16^3 is outside the crop's 12-voxel boundary influence: 2 + 2t conv layers); heads to 128^3 vs the oracle on a
    32^3 crop; ray-march of the 128^3 x 17 volume (142.6 MB) vs the oracle; reconstruct() end to end equals the staged pieces."""
    from forge_amd.model import FORGE, chose_selected, sequence_from_distance
    model, w, cfg = _model(FORGE, dev)
    t = 3
    feats, poses, extr = _grid64_inputs(t, 5)
    P = poses[None, :t].contiguous()
    fd = feats.to(dev)
    with torch.no_grad():
        ft = model.rotate(voxels=fd, camPoses_cv2=P.to(dev), grid_size=64)
        ref_rot = fo.rotate_world(feats[:, :, :8], P, 1.0)
        assert (ft[:, :, :8].cpu() - ref_rot).abs().max().item() < 2e-5 * max(1.0, ref_rot.abs().max().item())
        idx = sequence_from_distance(P[:, :, :3, 3])
        ft = chose_selected(ft, idx)
        fused = model.encoder_3d.fuse(ft)
        assert fused.shape == (1, 128, 64, 64, 64)
        crop = ft[:, :, :, 8:48, 8:48, 8:48].cpu().contiguous()
        ref_f = fo.fuse(crop, w)[:, :, 12:28, 12:28, 12:28]
        got_f = fused[:, :, 20:36, 20:36, 20:36].cpu()
        assert (got_f - ref_f).abs().max().item() < 2e-4 * max(1.0, ref_f.abs().max().item())
        feat3, dens3 = model.encoder_3d.heads(fused)
        assert feat3.shape == (1, 16, 128, 128, 128) and dens3.shape == (1, 1, 128, 128, 128)
        zc = fused[:, :, 16:48, 16:48, 16:48].cpu().contiguous()
        ref_d, ref_r = fo.density_head(zc, w)[..., 8:56, 8:56, 8:56], fo.render_features_head(zc, w)[..., 8:56, 8:56, 8:56]
        assert (dens3[..., 40:88, 40:88, 40:88].cpu() - ref_d).abs().max().item() < 1e-4 * max(1.0, ref_d.abs().max().item())
        assert (feat3[..., 40:88, 40:88, 40:88].cpu() - ref_r).abs().max().item() < 1e-4 * max(1.0, ref_r.abs().max().item())
        # ray-march the 128^3 volume: two cameras, 128^2 rays x 64 samples
        E = extr[[1, 7]]
        K = syn.intrinsics(256)[None].repeat(2, 1, 1)
        Kh = fo.halve_intrinsics(K)
        ref_raw = fo.render_rays(feat3.cpu().repeat(2, 1, 1, 1, 1), dens3.cpu().repeat(2, 1, 1, 1, 1), E[:, :3, :3], E[:, :3, 3], Kh,
                                 128, 128, 64, 0.5, 2.0, 1.0, False)
        cam = torch.cat([E[:, :3, :3].reshape(2, 9), E[:, :3, 3], Kh[:, 0, 0:1], Kh[:, 1, 1:2], Kh[:, 0, 2:3], Kh[:, 1, 2:3]], dim=1).to(dev)
        h = fo.grid_half_extent(128, 1.0)
        of, oo = ops.render_rays(feat3, dens3, cam, torch.zeros(2, dtype=torch.int32, device=dev), 128, 128, 64, 0.5, 2.0, (h, h, h), False)
        got_raw = torch.cat([of, oo], dim=1).permute(0, 2, 3, 1).cpu()
        assert (got_raw - ref_raw).abs().max().item() < 3e-5 * max(1.0, ref_raw.abs().max().item())
        # end to end through reconstruct(): identical kernels, identical results
        cams = geo_utils.camera_dict(E[None].to(dev), K[None].to(dev))
        imgs, masks, _ = model.reconstruct(fd, P.to(dev), cams)
        rgb_ref = model.render._conv_rgb_hip(of)
        assert (imgs - rgb_ref).abs().max().item() < 1e-6 and torch.isfinite(imgs).all() and imgs.shape == (2, 3, 256, 256)


def test_config4_grid64_batch_equals_single_scene(dev):
    """Full-size property at the 64^3 feature grid: fuse + heads of a 2-scene batch (operands of 805 MB / 1.07 GB: batch-strided
    addressing close to the kernels' 2 GiB buffer range, and chunked when MAX_OPERAND_BYTES is lowered) equal each scene run alone
    up to fp32 summation order; the chunked launch equals the unchunked one bit for bit."""
    from forge_amd import convops as co
    from forge_amd.model import FORGE
    model, _, _ = _model(FORGE, dev)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, 2, 128, 64, 64, 64, generator=g) * 0.5).to(dev)
    with torch.no_grad():
        both = model.encoder_3d.fuse(x)
        f_b, d_b = model.encoder_3d.heads(both)
        for s in range(2):
            one = model.encoder_3d.fuse(x[s:s + 1])
            assert (one - both[s:s + 1]).abs().max().item() < 2e-4 * max(1.0, both.abs().max().item())
            f1, d1 = model.encoder_3d.heads(both[s:s + 1])
            assert (f1 - f_b[s:s + 1]).abs().max().item() < 1e-4 * max(1.0, f_b.abs().max().item())
            assert (d1 - d_b[s:s + 1]).abs().max().item() < 1e-4 * max(1.0, d_b.abs().max().item())
        old = co.MAX_OPERAND_BYTES
        try:
            co.MAX_OPERAND_BYTES = 700 << 20                     # forces one scene per launch for the [b,t,...] input and the heads' up tensor
            chunked = model.encoder_3d.fuse(x)
            f_c, d_c = model.encoder_3d.heads(both)
        finally:
            co.MAX_OPERAND_BYTES = old
        assert torch.equal(chunked, both) and torch.equal(f_c, f_b) and torch.equal(d_c, d_b)


def test_config3_grid64_training_step_vs_oracle_autograd(dev):
    """BASELINE configs[3] shape of the TRAINING path at the 128^3-voxel grid: rotate -> fuse -> heads -> ray-march -> conv_rgb in
    train mode (BatchNorm batch statistics) on a synthetic [1,2,128,64^3] feature volume, loss = 5 MSE(rgb) + MSE(mask), backward through
    every HIP backward kernel at full size (rotate gather-adjoint at 64^3, ConvGRU dgrad/wgrad at M = 262144, transposed-conv and
    narrow-layer backward at 128^3, ray-march backward into a 142.6 MB volume) vs autograd through the CPU oracle: loss and the
    gradients of the input features and of parameters from every stage. Tolerance: 1e-2 of max(|g|max, 0.1 x the largest |g|max among
    the checked tensors): a bias gradient here is a sum of 262144 sign-alternating terms (|sum| ~ 1e-3 of sum |terms|), so per-term fp32
    noise of 1e-5 is amplified ~400x in its relative error (measured 1.6e-2 on conv_gate.bias with the loss equal to 1e-6)."""
    from forge_amd.model import FORGE
    model, w, cfg = _model(FORGE, dev, train=True)
    t = 2
    feats, poses, extr = _grid64_inputs(t, 13)
    P = poses[None, :t].contiguous()
    E = extr[None, [0, 3]].contiguous()
    K = syn.intrinsics(256)[None, None].repeat(1, 2, 1, 1)
    g = torch.Generator().manual_seed(3)
    tgt_i, tgt_m = torch.rand(2, 3, 256, 256, generator=g), torch.rand(2, 1, 256, 256, generator=g)
    fd = feats.to(dev).requires_grad_(True)
    imgs, masks, _ = model.reconstruct(fd, P.to(dev), geo_utils.camera_dict(E.to(dev), K.to(dev)))
    loss = 5.0 * torch.nn.functional.mse_loss(imgs, tgt_i.to(dev)) + torch.nn.functional.mse_loss(masks, tgt_m.to(dev))
    loss.backward()
    keys = ["encoder_3d.fusion_feature.cells.0.conv_gate.bias", "encoder_3d.fusion_feature.cells.0.out_gate.bias",
            "encoder_3d.fusion_feature.fusion_conv.4.weight", "encoder_3d.fusion_feature.fusion_norm.weight", "encoder_3d.features_head.3.bias",
            "encoder_3d.density_head.6.weight", "render.conv_rgb.3.weight"]
    wo = {k: (v.clone().requires_grad_(True) if k in keys else v.clone()) for k, v in w.items()}
    fr = feats.clone().requires_grad_(True)
    oi, om = fo.reconstruct_from_features(fr, P, E, K, wo, cfg, training=True, order_by_distance=True)
    lo = 5.0 * torch.nn.functional.mse_loss(oi, tgt_i) + torch.nn.functional.mse_loss(om, tgt_m)
    lo.backward()
    assert abs(loss.item() - lo.item()) < 1e-4 * max(1.0, abs(lo.item())), (loss.item(), lo.item())
    named = dict(model.named_parameters())
    gscale = max(wo[k].grad.abs().max().item() for k in keys)
    for k in keys:
        ref = wo[k].grad
        err = (named[k].grad.cpu() - ref).abs().max().item()
        assert err < 1e-2 * max(ref.abs().max().item(), 1e-1 * gscale), (k, err, ref.abs().max().item())
    # input-feature gradient: relative L2 (a max-norm bound is meaningless here - where a LeakyReLU pre-activation sits within fp32
    # noise of 0 the two implementations pick different slopes (1 vs 0.01) and the gradient of a few isolated voxels differs by O(1)).
    # This quantity is ill-conditioned in fp32 at this size (train-mode BatchNorm over 262144 voxels): tools/debug/config3_f64.py measured
    # fp32 oracle vs float64 oracle 1.0e-2, HIP vs float64 oracle 1.4e-2, HIP vs fp32 oracle 1.0e-2 - the bound is 3 x the oracle's own error.
    gf = fd.grad.cpu()
    l2 = (gf - fr.grad).norm().item() / fr.grad.norm().item()
    frac = ((gf - fr.grad).abs() > 1e-2 * fr.grad.abs().max()).float().mean().item()
    per_view = [((gf[:, v] - fr.grad[:, v]).norm() / fr.grad[:, v].norm().clamp_min(1e-30)).item() for v in range(t)]
    assert l2 < 3e-2 and frac < 3e-4, (l2, frac, per_view)


def test_config3_per_gpu_shape_b4_grid64_training_step_equals_its_four_scenes(dev):
    """BASELINE configs[3] PER-GPU shape: FORGE_poseEstimator3D training step at 4 scenes x 5 views on the 128^3-voxel grid (synthetic
    [4,5,128,64^3] feature volumes, 3 fusions, heads to 128^3, 40 ray-marched views, loss, backward) - ~60 GB live, the > 2 GiB batch
    chunking of the forward / data-gradient / weight-gradient launchers active. The CPU oracle cannot run this size, so the bar is a
    size-independent property: with BatchNorm on its running statistics the scenes of a batch are independent, hence loss and parameter
    gradients of the 4-scene step equal the mean over the same four scenes run ONE AT A TIME (b = 1: no chunking, other launch plans) - the
    b = 1 step itself is pinned against the oracle's autograd by test_config3_grid64_training_step_vs_oracle_autograd."""
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    model, w, cfg = _model(FORGE_poseEstimator3D, dev, train=True)
    for m_ in model.modules():
        if isinstance(m_, torch.nn.modules.batchnorm._BatchNorm):
            m_.eval()
    b, t = 4, 5
    g = torch.Generator(device=dev).manual_seed(41)
    feats = (torch.randn(b, t, 128, 64, 64, 64, device=dev, generator=g) * 0.5).permute(0, 1, 3, 4, 5, 2).contiguous().permute(0, 1, 5, 2, 3, 4)
    gc = torch.Generator().manual_seed(42)
    P, E = [], []
    for s_ in range(b):
        jit = (torch.rand(10, 2, generator=gc) - 0.5) * 0.3
        poses, extr, _ = syn.orbit_cameras(10, 1.5, 12.0, jit)
        P.append(poses[:t])
        E.append(extr[:t].repeat(2, 1, 1))
    P, E = torch.stack(P).to(dev), torch.stack(E).to(dev)
    K = syn.intrinsics(256)[None, None].repeat(b, 2 * t, 1, 1).to(dev)
    tgt_i, tgt_m = torch.rand(b, 2 * t, 3, 256, 256, generator=gc).to(dev), torch.rand(b, 2 * t, 1, 256, 256, generator=gc).to(dev)
    keys = ["encoder_3d.fusion_feature.cells.0.conv_gate.weight", "encoder_3d.fusion_feature.cells.0.out_gate.bias", "encoder_3d.fusion_feature.fusion_conv.3.weight",
            "encoder_3d.features_head.0.weight", "encoder_3d.features_head.3.weight", "encoder_3d.density_head.6.weight", "render.conv_rgb.0.weight",
            "render.conv_rgb.6.bias"]
    named = dict(model.named_parameters())

    def run(sl):
        model.zero_grad(set_to_none=True)
        n = sl.stop - sl.start
        imgs, masks, _ = model.reconstruct(feats[sl], P[sl], geo_utils.camera_dict(E[sl], K[sl]))
        loss = 5.0 * torch.nn.functional.mse_loss(imgs.reshape(n, 2 * t, 3, 256, 256), tgt_i[sl]) + \
            torch.nn.functional.mse_loss(masks.reshape(n, 2 * t, 1, 256, 256), tgt_m[sl])
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), {k: named[k].grad.detach().double().clone() for k in keys}
    l4, g4 = run(slice(0, b))
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30
    singles = [run(slice(i, i + 1)) for i in range(b)]
    l1 = sum(x[0] for x in singles) / b
    assert abs(l4 - l1) < 1e-5 * max(1.0, abs(l1)), (l4, l1)
    for k in keys:
        ref = sum(x[1][k] for x in singles) / b
        rel = ((g4[k] - ref).norm() / ref.norm().clamp_min(1e-30)).item()
        cos = torch.nn.functional.cosine_similarity(g4[k].flatten(), ref.flatten(), dim=0).item()
        assert rel < 2e-3 and cos > 0.99999, (k, rel, cos)
    assert peak_gb > 20.0, peak_gb                                   # the per-GPU shape really was resident (61.7 GB measured in round 2)


# ------------------------------------------------------------------------------------------------------------- f4
def test_checkpoint_round_trip_reference_layout(dev, golden, tmp_path):
    """f4: a checkpoint written in the reference's layout (utils/train_utils.py:167: {'epoch','state_dict' with DDP's `module.`
    prefix,'optimizer','best_psnr'}) is read back with strict=True by resume_training (utils/exp_utils.py:152-182) and reproduces the
    reference model's golden forward; load_encoder_pretrained (utils/exp_utils.py:185-216) hands the encoder_3d/rotate/render
    sub-trees over to a joint FORGE model (strict per sub-module) which then renders the same views. The sample arrives as HOST
    tensors: one pinned staging copy (forge_amd/staging.py)."""
    from forge_amd import checkpoint as ck
    from forge_amd.model import FORGE
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    g = golden("forward_pose3d")
    src, w, cfg = _model(FORGE_poseEstimator3D, dev, seed=int(g["weight_seed"]))
    opt = torch.optim.Adam(src.parameters(), lr=cfg.train.lr)
    ck.save_checkpoint({"epoch": 7, "state_dict": {"module." + k: v for k, v in src.state_dict().items()}, "optimizer": opt.state_dict(),
                        "best_psnr": 21.5}, str(tmp_path), "cpt_last.pth.tar")
    fresh = FORGE_poseEstimator3D(cfg).to(dev).eval()
    with torch.no_grad():
        sample = syn.make_sample(1, 5, 256, 1.5, seed=int(g["sample_seed"]))
        stale = fresh(sample, syn.SyntheticDataset(1.5), dev)[0].clone()          # populates the packed-weight caches with the random init
    opt2 = torch.optim.Adam(fresh.parameters(), lr=cfg.train.lr)
    fresh, opt2, epoch, best_psnr, best_rot = ck.resume_training(fresh, opt2, str(tmp_path), strict=True, device=dev)
    assert epoch == 7 and best_psnr == 21.5 and best_rot == float("inf")
    with torch.no_grad():
        imgs, masks = fresh(sample, syn.SyntheticDataset(1.5), dev)               # host sample -> staged copy; caches must have been dropped
    assert not torch.equal(imgs, stale)
    assert_forward_close(imgs[:, :, ::4, ::4], T(g["imgs_sub"]), masks[:, :, ::4, ::4], T(g["masks_sub"]), "resumed checkpoint vs reference golden",
                         max_abs=4e-4, psnr=90.0, mask_abs=2e-4)
    # stage hand-over into the joint model
    joint = FORGE(syn.kubric_config()).to(dev).eval()
    ck.load_encoder_pretrained(joint, str(tmp_path), strict=True, device=dev)
    for name in ("encoder_3d", "rotate", "render"):
        for (k, a), (_, b) in zip(getattr(joint, name).state_dict().items(), getattr(src, name).state_dict().items()):
            assert torch.equal(a, b), (name, k)
    with pytest.raises(RuntimeError):
        ck.resume_training(joint, None, str(tmp_path), strict=True, device=dev)    # pose networks are missing from the GT-pose checkpoint


def test_staged_sample_equals_device_resident_sample(dev):
    """One pinned host->device copy per forward (f4): results identical to the device-resident sample; tensors of an earlier forward
    are not overwritten by the next staging."""
    from forge_amd.model import FORGE
    from forge_amd.staging import stage_sample
    model, _, _ = _model(FORGE, dev)
    ds = syn.SyntheticDataset(1.5)
    host = syn.make_sample(2, 5, 256, 1.5, seed=44)
    st1 = stage_sample(host, dev)
    keep = st1["images"].clone()
    host2 = syn.make_sample(2, 5, 256, 1.5, seed=45)
    st2 = stage_sample(host2, dev)
    assert torch.equal(st1["images"], keep) and torch.equal(st1["images"].cpu(), host["images"])
    assert st2["K_cv2"].data_ptr() % 256 == 0 and torch.equal(st2["cam_poses_rel_cv2"].cpu(), host2["cam_poses_rel_cv2"])
    with torch.no_grad():
        a = model(host, ds, dev)
        b = model({k: v.to(dev) for k, v in host.items()}, ds, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------- ADVICE r1 regressions
def test_inference_mode_and_data_edit_invalidation(dev):
    """(i) forward under torch.inference_mode() (inference tensors have no version counter: the old heads memo crashed);
    (ii) a `.data` edit + forge_amd.invalidate_packed() changes the fused inference output exactly as it changes the autograd path."""
    import forge_amd
    from forge_amd.model import FORGE
    model, _, _ = _model(FORGE, dev)
    ds = syn.SyntheticDataset(1.5)
    sample = {k: v.to(dev) for k, v in syn.make_sample(1, 5, 256, 1.5, seed=8).items()}
    with torch.no_grad():
        base = model(sample, ds, dev)[0].clone()
    with torch.inference_mode():
        inf = model(sample, ds, dev)[0]
        assert torch.equal(inf, base)
    p = model.encoder_3d.features_head[3].weight
    p.data.mul_(1.5)
    forge_amd.invalidate_packed(model)
    with torch.no_grad():
        edited = model(sample, ds, dev)[0]
    assert not torch.equal(edited, base)
    model.eval()                                                       # mode switches drop the caches too
    p.data.div_(1.5)
    model.eval()
    with torch.no_grad():
        back = model(sample, ds, dev)[0]
    assert (back - base).abs().max().item() < 1e-5


def test_single_head_getters_equal_merged_heads(dev):
    """get_density3D / get_render_features (each head alone, N = 32 transposed conv) == heads() (merged N = 64 launch)."""
    from forge_amd.encoder import Encoder3D
    enc = Encoder3D(syn.kubric_config())
    enc.load_state_dict({k[len("encoder_3d."):]: v for k, v in
                         syn.seeded_state_dict({"encoder_3d." + k: v for k, v in enc.state_dict().items()}, 0).items()})
    enc = enc.to(dev).eval()
    z = torch.randn(2, 128, 8, 8, 8, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        f, d = enc.heads(z)
        assert (enc.get_render_features(z) - f).abs().max().item() < 1e-5 and (enc.get_density3D(z) - d).abs().max().item() < 1e-5


def test_frozen_eval_paths_equal_autograd_paths(dev):
    """Row f2 (pose refinement, frozen weights): the fused-forward / hand-written-backward paths (_FuseFrozen, _HeadsFrozen,
    _ConvRgbFrozen - taken when no parameter requires grad) give the same outputs and the same input gradients as the generic
    autograd paths on the same module (taken when a parameter requires grad). Outputs: 2e-4 of the max. Gradients: relative L2 1e-3 and
    at most 1e-4 of the elements off by more than 1 % of the max - NOT a max-norm bound: the two paths sum in different orders, so a
    LeakyReLU pre-activation within fp32 noise of 0 takes slope 1 in one and 0.01 in the other and isolated gradient elements differ
    (tools/debug/heads_bwd_full.py: every stage agrees to 1e-6 with torch except at those sign flips; the float64 oracle comparison is
    test_refinement_pose_gradient_vs_oracle_autograd)."""
    from forge_amd.model import FORGE
    model, _, _ = _model(FORGE, dev)
    g = torch.Generator().manual_seed(17)
    x0 = (torch.randn(1, 3, 128, 16, 16, 16, generator=g) * 0.5).to(dev)
    r0 = torch.randn(2, 16, 24, 24, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)

    def run(frozen):
        for p in model.parameters():
            p.requires_grad_(not frozen)
        x = x0.clone().requires_grad_(True)
        fused = model.encoder_3d.fuse(x)
        feat, dens = model.encoder_3d.heads(fused)
        wf, wd = torch.linspace(-1, 1, feat.numel(), device=dev).reshape(feat.shape), torch.linspace(1, -1, dens.numel(), device=dev).reshape(dens.shape)
        ((feat * wf).sum() + (dens * wd).sum() + fused.square().sum() * 1e-3).backward()
        r = r0.clone().requires_grad_(True)
        if frozen:
            from forge_amd.volume_render import _ConvRgbFrozen
            rgb = _ConvRgbFrozen.apply(r, model.render)
        else:
            rgb = model.render._conv_rgb_autograd_hip(r)
        (rgb * torch.linspace(-1, 1, rgb.numel(), device=dev).reshape(rgb.shape)).sum().backward()
        return [t.detach().clone() for t in (fused, feat, dens, x.grad, rgb, r.grad)]
    a, b = run(True), run(False)
    for p in model.parameters():
        p.requires_grad_(True)
    for name, u, v in zip(("fused", "feat", "dens", "dx", "rgb", "dr"), a, b):
        if name in ("dx", "dr"):
            assert (u - v).norm().item() < 1e-3 * v.norm().item(), (name, (u - v).norm().item() / v.norm().item())
            assert ((u - v).abs() > 1e-2 * v.abs().max()).float().mean().item() < 1e-4, name
        else:
            assert rel(u, v) < 2e-4, (name, rel(u, v))


def test_grouped_mse_equals_four_mse_losses(dev):
    """f1: the fused squared-error pass (csrc/loss.hip) == the reference's four F.mse_loss terms (scripts/kubric_compute_loss.py:26-29),
    values and gradients, for the channels-last rgb layout conv_rgb produces and the plain-NCHW mask layout; both view-group mappings
    (GT-pose model: 2t rendered views vs t targets; joint model: t + t rendered vs t + t targets)."""
    import torch.nn.functional as F
    from forge_amd.train import grouped_mse
    g = torch.Generator().manual_seed(12)
    b, t, h, w = 2, 5, 24, 40
    for c, cl in ((3, True), (1, False)):
        for Vt in (t, 2 * t):
            base = torch.rand(b * 2 * t, c, h, w, generator=g).to(dev)
            if cl:
                base = base.contiguous(memory_format=torch.channels_last)
            tgt = torch.rand(b, Vt, c, h, w, generator=g).to(dev)
            p1 = base.clone(memory_format=torch.preserve_format).requires_grad_(True)
            p2 = base.clone(memory_format=torch.preserve_format).requires_grad_(True)
            m = grouped_mse(p1.reshape(b, 2 * t, c, h, w), tgt, t)
            r = p2.reshape(b, 2 * t, c, h, w)
            ref = torch.stack([F.mse_loss(r[:, :t], tgt[:, :t]), F.mse_loss(r[:, t:], tgt[:, :t] if Vt == t else tgt[:, t:])])
            assert (m - ref).abs().max().item() < 1e-6 * max(1.0, ref.abs().max().item())
            (5.0 * m[0] + 0.3 * m[1]).backward()
            (5.0 * ref[0] + 0.3 * ref[1]).backward()
            assert (p1.grad - p2.grad).abs().max().item() < 1e-6 * p2.grad.abs().max().item() + 1e-9


def test_fuse_groups_inference_shares_input_halves(dev):
    """FORGE_poseEstimator3D's three fusions in INFERENCE with the input halves of the GRU convolutions computed once per view
    (ConvGRU_3D.fuse_groups_hip: residual operand of the fused GRU epilogues) against three independent fuse_hip calls and the oracle:
    2e-4 of the max (fp32 summation order: conv(x, W_x) + conv(h, W_h) vs conv([x, h], W))."""
    from forge_amd.model import FORGE
    model, w, _ = _model(FORGE, dev)
    x = (torch.randn(2, 5, 128, 8, 8, 8, generator=torch.Generator().manual_seed(21)) * 0.5)
    groups = [[0, 1, 2], [3, 4], [0, 1, 2, 3, 4]]
    with torch.no_grad():
        shared = model.encoder_3d.fuse_groups(x.to(dev), groups)
        for g, s in zip(groups, shared):
            sep = model.encoder_3d.fuse(x[:, g].to(dev))
            ref = fo.fuse(x[:, g], w)
            scale = max(1.0, ref.abs().max().item())
            assert (s - sep).abs().max().item() < 2e-4 * scale and (s.cpu() - ref).abs().max().item() < 2e-4 * scale


@pytest.mark.parametrize("C", [64, 128])
def test_fuse_groups_inference_8_plane_form_equals_separate_fusions(dev, C):
    """test_fuse_groups_inference_shares_input_halves at 2 scenes = 2048 tile rows per GRU step, where the point products take the 8-plane form
    (convops.wino_half_applies): at C = 64 the gates' (2 C columns) but not the state's (C columns), so the shared input-half products of the two
    GRU convolutions come in different forms. ConvGRU_3D.fuse_groups_hip against independent fuse_hip calls, the same bound."""
    from forge_amd import convops as co
    from forge_amd.fusion import ConvGRU_3D
    R = 2 * 16 * 8 * 8
    assert co.wino_half_applies(R, 2 * C, C) and co.wino_half_applies(R, C, C) == (C > 64)
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=C, hidden_size=C)
    gru.load_state_dict(syn.seeded_state_dict(gru.state_dict(), 3))
    gru = gru.to(dev).eval()
    x = (torch.randn(2, 5, C, 16, 16, 16, generator=torch.Generator().manual_seed(21)) * 0.5).to(dev)
    groups = [[0, 1, 2], [3, 4], [0, 1, 2, 3, 4]]
    with torch.no_grad():
        shared = gru.fuse_groups_hip(x, groups)
        for g, s in zip(groups, shared):
            sep = gru.fuse_hip(x[:, g])
            assert (s - sep).abs().max().item() < 2e-4 * max(1.0, sep.abs().max().item()), g


def test_conv_wgrad_batch_chunking(dev, monkeypatch):
    """convops.conv_wgrad accumulates batches whose operands exceed the kernel's 2 GiB buffer range in batch chunks (needed by the
    128^3-voxel training step at 4 scenes per GPU): with the limit lowered so that 5 volumes split 2 + 2 + 1, the weight gradient equals
    the single launch (fp32 atomics: 1e-5 of the max) - two-input form with a batch-strided first operand."""
    from forge_amd import convops as co
    g = torch.Generator().manual_seed(6)
    n, D, C = 5, 8, 128
    xs = torch.randn(n, 2, D, D, D, C, generator=g).to(dev)                    # views stacked: x1 = xs[:, 1] has a batch stride
    x1, h = xs[:, 1], torch.randn(n, D, D, D, C, generator=g).to(dev)
    dy = torch.randn(n, D, D, D, 2 * C, generator=g).to(dev)
    bs1 = co._batch_stride_rows(x1)

    def run():
        dw = torch.zeros(27, 2 * C, 2 * C, device=dev)
        co.conv_wgrad(dy, x1, C, h, C, dw, (n, D, D, D), (D, D, D), 2 * C, co.TAPS_3x3x3, bs1=bs1)
        return dw
    ref = run()
    monkeypatch.setattr(co, "MAX_OPERAND_BYTES", 2 * D ** 3 * 2 * C * 4 + 1)     # two volumes of dy per launch
    got = run()
    assert (got - ref).abs().max().item() < 1e-5 * ref.abs().max().item()
    want = torch.nn.grad.conv3d_weight(torch.cat([x1, h], dim=-1).permute(0, 4, 1, 2, 3).contiguous(), (2 * C, 2 * C, 3, 3, 3),
                                       dy.permute(0, 4, 1, 2, 3).contiguous(), padding=1)
    assert (got.permute(1, 2, 0).reshape(2 * C, 2 * C, 3, 3, 3) - want).abs().max().item() < 1e-3 * want.abs().max().item()


def test_rotate_fused_view_order_equals_gather(dev):
    """The view ordering of models/model.py:127-128 fused into the warp's store (forge_rotate_fwd_slots; ranks computed by the pose kernel
    for order="distance") == warp followed by sequence_from_distance + chose_selected, bit for bit; explicit index orders and a tie
    (two views at the same distance: lower view index first, as torch.sort's stable result on equal keys) included."""
    from forge_amd.model import chose_selected, sequence_from_distance
    from forge_amd.rotate import Rotate_world
    rot = Rotate_world(syn.kubric_config()).to(dev)
    g = torch.Generator().manual_seed(33)
    jit = (torch.rand(10, 2, generator=g) - 0.5) * 0.4
    p1, _, _ = syn.orbit_cameras(10, 1.5, 20.0, jit)
    p2, _, _ = syn.orbit_cameras(10, 1.5, 5.0)
    P = torch.stack([p1[[0, 4, 2, 7, 1]], p2[[0, 3, 3, 9, 6]]]).to(dev)          # scene 1: views 1 and 2 share a pose (tie)
    vox = torch.randn(2, 5, 8, 16, 16, 16, generator=g).to(dev)
    with torch.no_grad():
        plain = rot(vox, P, grid_size=16)
        idx = sequence_from_distance(P[:, :, :3, 3])
        want = chose_selected(plain, idx)
        assert torch.equal(rot(vox, P, grid_size=16, order="distance"), want)
        assert torch.equal(rot(vox, P, grid_size=16, order=idx), want)
        perm = torch.tensor([[4, 0, 3, 1, 2], [2, 1, 0, 4, 3]], device=dev)
        assert torch.equal(rot(vox, P, grid_size=16, order=perm), chose_selected(plain, perm))
    vg = vox.clone().requires_grad_(True)                                        # autograd path: gather on the result
    assert torch.equal(rot(vg, P, grid_size=16, order="distance").detach(), want)
