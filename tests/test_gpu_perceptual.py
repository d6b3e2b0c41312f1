"""GPU (-m gpu): the VGG-16 perceptual loss (forge_amd/perceptual.py) against the float64 reference class (tests/golden/perceptual_vgg.npz,
tools/make_golden_perceptual.py), its kernels against torch autograd, determinism, and the training-step integration (eager, captured, DDP)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from forge_amd import _lib, synthetic as syn
from forge_amd import perceptual as fp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "perceptual_vgg.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def modules(gold, dev):
    seed = int(gold["seed"])
    return {r: fp.VGGPerceptualLoss(resize=r, pretrained=False, seed=seed).to(dev) for r in (True, False)}


@pytest.mark.parametrize("case", list("abcde"))
def test_golden_case_loss_and_input_gradient(gold, modules, dev, case):
    from make_golden_perceptual import images, to_float
    pairs, C, H, W, resize, deepest = (int(v) for v in gold[case + "_meta"])
    inp, tgt = images(case, pairs, C, H, W)
    assert [int(inp.astype(np.int64).sum()), int(tgt.astype(np.int64).sum())] == gold[case + "_codesum"].tolist()
    x = to_float(inp).to(dev).requires_grad_(True)
    y = to_float(tgt).to(dev)
    loss = modules[bool(resize)](x, y, only_deepest=bool(deepest))
    loss.backward()
    # the golden holds rows 0, s, 2s, ... of the gradient (s = rowstep) as float16 of grad / gscale
    ref_l = float(gold[case + "_loss"])
    ref_g = torch.from_numpy(gold[case + "_grad"].astype(np.float64)) * float(gold[case + "_gscale"])
    g = x.grad.double().cpu()[:, :, ::int(gold[case + "_rowstep"])]
    rel_loss = abs(loss.item() - ref_l) / abs(ref_l)
    rel_l2 = ((g - ref_g).norm() / ref_g.norm()).item()
    cos = (g.flatten() @ ref_g.flatten() / (g.norm() * ref_g.norm())).item()
    print("perceptual golden %s: loss rel %.3g grad rel L2 %.3g cos %.8f" % (case, rel_loss, rel_l2, cos))
    # gradient: relative L2 <= 2e-2. ReLU masks and sign(x - y) flip on near-zero elements between fp32 and float64, each flip a full-size
    # change of one element; the measured 2e-4 .. 8.4e-3 is the same with every convolution on the direct GEMM instead of Winograd
    # (DESIGN.md "VGG-16 perceptual loss": accuracy). The cosine bound is what catches a wrong gradient.
    assert rel_loss <= 1e-4 and rel_l2 <= 2e-2 and cos >= 0.9999, (rel_loss, rel_l2, cos)


def _tap_bwd(x, y, g_next, coef):
    N, H, W, C = x.shape
    d = torch.empty_like(x)
    _lib.check(_lib.lib().forge_vgg_tap_bwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(g_next), _lib.ptr(coef), _lib.ptr(d), N, H, W, C,
                                            _lib.current_stream()), "forge_vgg_tap_bwd")
    return d


@pytest.mark.parametrize("with_next,with_l1", [(True, True), (False, True), (True, False)])
def test_tap_boundary_backward_is_torch_autograd_bitwise(dev, with_next, with_l1):
    g = torch.Generator().manual_seed(7)
    N, H, W, C = 2, 12, 10, 16
    pre = torch.randn(N, H, W, C, generator=g)
    pre[:, 0::2, 0::2] = pre[:, 1::2, 1::2]                         # tied maxima inside many windows (first in row-major order must win)
    pre[0, 4:6, 4:6, :] = 0.7                                       # a window of four equal values
    pre = pre.to(dev).requires_grad_(True)
    y = torch.relu(torch.randn(N, H, W, C, generator=g)).to(dev)
    y[0, 0, 0] = torch.relu(pre.detach()[0, 0, 0])                  # x == y: sign 0
    gn = torch.randn(N, H // 2, W // 2, C, generator=g).to(dev)
    w = torch.tensor(0.37, device=dev)
    x = torch.relu(pre)
    loss = 0
    if with_next:
        loss = loss + (F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2) * gn.permute(0, 3, 1, 2)).sum()
    if with_l1:
        loss = loss + w * F.l1_loss(x, y)
    (ref,) = torch.autograd.grad(loss, pre)
    coef = (w / x.numel()).reshape(1) if with_l1 else None
    got = _tap_bwd(x.detach().contiguous(), y, gn if with_next else None, coef)
    assert torch.equal(got, ref)


def _prep_rows(x, t, mean, std, resize):
    N, C, Hi, Wi = x.shape
    Ho, Wo = (224, 224) if resize else (Hi, Wi)
    rows = torch.empty(2 * N * Ho * Wo, 32, device=x.device)
    st = lambda v: [int(s) for s in v.stride()]
    _lib.check(_lib.lib().forge_vgg_prep_fwd(_lib.ptr(x), *st(x), _lib.ptr(t), *st(t), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(rows), N, C, Hi, Wi,
                                             Ho, Wo, int(resize), _lib.current_stream()), "forge_vgg_prep_fwd")
    return rows.view(2 * N, Ho, Wo, 32)


@pytest.mark.parametrize("C,layout,resize", [(3, "channels_last", True), (3, "contiguous", True), (1, "contiguous", True), (3, "contiguous", False)])
def test_preparation_and_adjoint_match_torch(dev, C, layout, resize):
    g = torch.Generator().manual_seed(11)
    N, Hi, Wi = 2, 40, 56 if resize else 48
    if not resize:
        Hi = 32
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
    x = torch.rand(N, C, Hi, Wi, generator=g).to(dev)
    t = torch.rand(N, C, Hi, Wi, generator=g).to(dev)
    if layout == "channels_last":
        x, t = x.contiguous(memory_format=torch.channels_last), t.contiguous(memory_format=torch.channels_last)
    xr = x.clone().requires_grad_(True)

    def ref_prep(v):
        v = v.repeat(1, 3, 1, 1) if C == 1 else v
        v = (v - mean) / std
        return F.interpolate(v, mode="bilinear", size=(224, 224), align_corners=False) if resize else v
    ri, rt = ref_prep(xr), ref_prep(t)
    rows = _prep_rows(x, t, mean, std, resize)
    Ho, Wo = rows.shape[1:3]
    # the centre tap (ky = kx = 1) of the patch rows is the prepared image itself
    got = rows[..., 12:15].permute(0, 3, 1, 2)
    ref = torch.cat([ri, rt]).detach()
    assert (got - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())
    assert torch.equal(rows[:, 0, :, 0:9], torch.zeros_like(rows[:, 0, :, 0:9]))          # the row above the image is padding
    assert torch.equal(rows[..., 27:], torch.zeros_like(rows[..., 27:]))
    # adjoint
    gy = torch.randn(N, 3, Ho, Wo, generator=g).to(dev)
    (rg,) = torch.autograd.grad(ri, xr, gy)
    g4 = F.pad(gy.permute(0, 2, 3, 1), (0, 1)).contiguous()
    din = torch.empty_like(x)
    st = [int(s) for s in din.stride()]
    _lib.check(_lib.lib().forge_vgg_prep_bwd(_lib.ptr(g4), 4, _lib.ptr(std), _lib.ptr(din), *st, N, C, Hi, Wi, Ho, Wo, int(resize),
                                             _lib.current_stream()), "forge_vgg_prep_bwd")
    assert din.stride() == x.stride()
    assert (din - rg).abs().max().item() <= 1e-5 * max(1.0, rg.abs().max().item())


def test_two_calls_are_bitwise_identical(modules, dev):
    g = torch.Generator().manual_seed(3)
    x0 = torch.rand(3, 3, 96, 128, generator=g).to(dev)
    y = torch.rand(3, 3, 96, 128, generator=g).to(dev)
    out = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        loss = modules[True](x, y)
        loss.backward()
        out.append((loss.detach(), x.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    with torch.no_grad():
        assert torch.equal(modules[True](x0, y), out[0][0])
    with pytest.raises(ValueError):
        modules[True](x0.requires_grad_(True), y.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        modules[False](torch.rand(1, 3, 40, 40, device=dev), torch.rand(1, 3, 40, 40, device=dev))


def _gt_pose_setup(dev, seed=5):
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    sample = {k: v.to(dev) for k, v in syn.make_sample(1, 5, 256, 1.5, seed=seed).items()}
    return cfg, model, sample


def test_training_loss_term_and_gradients(dev):
    from forge_amd import train
    cfg, model, sample = _gt_pose_setup(dev)
    ds = syn.SyntheticDataset(1.5)
    pl = fp.VGGPerceptualLoss(pretrained=False).to(dev)
    grads = {}
    for w in (0.0, 0.02):
        cfg.loss.perceptual_img = w
        model.zero_grad(set_to_none=True)
        loss, losses, imgs, _ = train.compute_reconstruction_loss(cfg, 0, sample, ds, model, {}, dev, perceptual_loss=pl)
        loss.backward()
        grads[w] = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        if w > 0:
            b, t, c, h, wd = sample["images"].shape
            tgt = sample["images"].reshape(b, t, c, h, wd).repeat(1, 2, 1, 1, 1).reshape(-1, c, h, wd)
            with torch.no_grad():
                ref = 0.02 * pl(imgs.reshape(-1, c, h, wd), tgt)
            assert abs(float(losses["perceptual_img"]) - ref.item()) <= 1e-6 * abs(ref.item())
            mse = sum(float(v) for k, v in losses.items() if k != "perceptual_img")
            assert abs(loss.item() - (mse + float(losses["perceptual_img"]))) <= 1e-5 * abs(loss.item())
    assert all(torch.isfinite(g).all() for g in grads[0.02].values())
    assert any(not torch.equal(grads[0.0][k], grads[0.02][k]) for k in grads[0.0])


def test_graphed_training_step_with_perceptual_term(dev):
    from forge_amd import train
    from forge_amd.graph import GraphedStep
    ds = syn.SyntheticDataset(1.5)

    def make():
        cfg, model, sample = _gt_pose_setup(dev, seed=6)
        cfg.loss.perceptual_img = 0.02
        pl = fp.VGGPerceptualLoss(pretrained=False).to(dev)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, capturable=True)

        def step():
            loss, _, _, _ = train.compute_reconstruction_loss(cfg, 0, sample, ds, model, {}, dev, perceptual_loss=pl)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
            opt.step()
            return loss.detach()
        return opt, step

    opt_e, step_e = make()
    eager = []
    for _ in range(4):
        opt_e.zero_grad(set_to_none=True)
        eager.append(step_e().item())
    opt_g, step_g = make()
    g = GraphedStep(step_g, opt_g, warmup=2)
    graphed = [g().item() for _ in range(2)]
    for a, b in zip(eager[2:], graphed):
        assert abs(a - b) < 5e-3 * abs(a), (eager, graphed)


def test_ddp_wrap_like_the_reference(dev):
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        pl = fp.VGGPerceptualLoss(pretrained=False).to(dev)
        ddp = torch.nn.parallel.DistributedDataParallel(pl, device_ids=[dev.index], find_unused_parameters=True)
        x = torch.rand(2, 3, 64, 64, device=dev, requires_grad=True)
        y = torch.rand(2, 3, 64, 64, device=dev)
        for _ in range(2):
            loss = ddp(x, y).mean()
            loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
        assert all(p.grad is None or not p.grad.any() for p in (pl.mean, pl.std))          # not inputs of the graph: no gradient
    finally:
        dist.destroy_process_group()
