"""Deterministic mode on the MI355X: the _det entry points (include/forge_hip.h, "Deterministic mode") per kernel family, and bitwise-reproducible
GT-pose training steps, joint-step gradients and pose refinement with forge_amd.deterministic(True)."""
import ctypes

import pytest
import torch

import forge_amd
from forge_amd import _lib, convops as co, synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def _ws(nbytes, dev):
    assert nbytes >= 0, nbytes
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _check_family(dev, run_det, run_atomic, shape, ref=None, noise=2e-5):
    """run_det(out, accumulate) launches the _det entry into out; run_atomic(out) the default entry into a zero-filled out.
    (a) accumulate = 0 over NaN: finite, within noise * max|ref| of the float64 reference; (b) accumulate = 1 on a random prior equals
    prior + (a) bitwise; (c) 20 launches interleaved with other work are bitwise identical; (d) within reorder noise of the atomic path."""
    first = torch.full(shape, float("nan"), device=dev)
    run_det(first, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(first).all()
    atomic = torch.zeros(shape, device=dev)
    run_atomic(atomic)
    torch.cuda.synchronize()
    scale = (ref if ref is not None else atomic.double()).abs().max().item()
    assert scale > 0
    if ref is not None:
        err = (first.double() - ref).abs().max().item()
        assert err <= noise * scale, (err, scale)
    assert (first - atomic).abs().max().item() <= noise * scale                                          # (d)
    prior = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    acc = prior.clone()
    run_det(acc, 1)
    assert torch.equal(acc, prior + first)                                                                # (b)
    scratch = torch.empty(1 << 20, device=dev)
    for i in range(20):                                                                                   # (c)
        scratch.normal_()                                                                                 # other launches on the stream
        again = torch.full(shape, float("nan") if i % 2 else 7.0, device=dev)
        run_det(again, 0)
        scratch.mul_(0.5)
        assert torch.equal(again, first), i


def _ref_wgrad(dy, x, taps, ist, D):
    """float64 dW[t] = dY^T X_t with torch slices and matmuls (as tests/test_gpu_parity.py's tap-grouped tiles test)."""
    n, _, H, W, Cy = dy.shape
    Cx = x.shape[-1]
    pad = 4
    xp = torch.nn.functional.pad(x.double(), (0, 0, pad, pad, pad, pad, pad if D > 1 else 0, pad if D > 1 else 0))
    dyf = dy.double().reshape(-1, Cy)
    ref = torch.empty(len(taps), Cy, Cx, dtype=torch.float64, device=dy.device)
    for t, (dz, dy_, dx) in enumerate(taps):
        z0 = (dz + pad) if D > 1 else 0
        xs = xp[:, z0:z0 + (D - 1) * ist + 1:ist, dy_ + pad:dy_ + pad + (H - 1) * ist + 1:ist, dx + pad:dx + pad + (W - 1) * ist + 1:ist]
        ref[t] = dyf.t() @ xs.reshape(-1, Cx)
    return ref


T27 = [tuple(t) for t in co.TAPS_3x3x3]
WGRAD_CASES = {   # name: (n, D, H, W, Cout, C1, C2, ist, taps) - the kernel each shape selects (conv_wgrad.hip's dispatch)
    "tiles_ciw128_two_inputs": (1, 8, 16, 16, 64, 128, 64, 1, T27),
    "tiles_ciw64": (1, 8, 16, 16, 128, 64, 0, 1, T27),
    "tiles_ciw32": (1, 8, 16, 24, 64, 32, 0, 1, T27),
    "tiles_ciw64_tg2": (2, 8, 96, 90, 96, 64, 0, 1, [(0, 0, 0), (1, 0, -1)]),
    "tiles_ciw32_tg4": (3, 1, 256, 200, 64, 32, 0, 1, [(0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]),
    "lines": (1, 8, 16, 40, 32, 32, 0, 1, T27),
    "lines16_cin16": (2, 8, 16, 40, 16, 16, 0, 1, T27),
    "lines16_cin32": (2, 8, 16, 40, 16, 32, 0, 1, T27),
    "lines16_stride2": (2, 1, 24, 40, 16, 16, 0, 2, [(0, ky - 2, kx - 2) for ky in range(6) for kx in range(6)]),
    "small": (2, 6, 10, 20, 8, 8, 0, 1, [(0, 0, -4), (0, 0, 4), (1, 1, 0), (0, 0, 0), (-1, 0, 2)]),
}


@pytest.mark.parametrize("case", sorted(WGRAD_CASES))
def test_conv_wgrad_det_families(dev, case):
    n, D, H, W, Cout, C1, C2, ist, taps = WGRAD_CASES[case]
    Di, Hi, Wi = (D * ist if D > 1 else 1), H * ist, W * ist
    g = torch.Generator().manual_seed(len(case))
    dy = torch.randn(n, D, H, W, Cout, generator=g).to(dev)
    x = torch.randn(n, Di, Hi, Wi, C1 + C2, generator=g).to(dev)
    x1 = x[..., :C1].contiguous()
    x2 = x[..., C1:].contiguous() if C2 else None
    ref = _ref_wgrad(dy, x, taps, ist, D)
    L = _lib.lib()
    ta = (ctypes.c_int * (3 * len(taps)))(*[v for t in taps for v in t])
    nbytes = L.forge_conv_wgrad_det_ws_bytes(C1, C2, n, D, H, W, ist, Di, Hi, Wi, Cout, ta, len(taps))
    assert nbytes > 0
    ws = _ws(nbytes, dev)
    common = lambda out: (_lib.ptr(dy), Cout, _lib.ptr(x1), C1, C1, 0, _lib.ptr(x2), C2, max(C2, 0), 0, _lib.ptr(out), n, D, H, W, ist, Di, Hi, Wi,
                          Cout, ta, len(taps))

    def det(out, accumulate):
        _lib.check(L.forge_conv_wgrad_det(*common(out), accumulate, _lib.ptr(ws), nbytes, _lib.current_stream()), "forge_conv_wgrad_det")

    def atomic(out):
        _lib.check(L.forge_conv_wgrad(*common(out), _lib.current_stream()), "forge_conv_wgrad")
    _check_family(dev, det, atomic, (len(taps), Cout, C1 + C2), ref)
    # the workspace is checked, not trusted
    out = torch.zeros(len(taps), Cout, C1 + C2, device=dev)
    assert L.forge_conv_wgrad_det(*common(out), 0, _lib.ptr(ws), nbytes - 4, _lib.current_stream()) == -1


@pytest.mark.parametrize("kd", [1, 3])
def test_wino_wgrad_det(dev, kd):
    n, D, Ht, Wt, Cout, C1 = 2, 4, 8, 8, 64, 128
    R = n * D * Ht * Wt
    g = torch.Generator().manual_seed(kd)
    dM = torch.randn(16, R, Cout, generator=g).to(dev)
    V = torch.randn(16, R, C1, generator=g).to(dev)
    Vg = V.double().reshape(16, n, D, Ht, Wt, C1)
    ref = torch.empty(16, kd, Cout, C1, dtype=torch.float64, device=dev)
    for k in range(kd):
        dz = k - 1 if kd == 3 else 0
        sh = torch.zeros_like(Vg)
        if dz == 0:
            sh = Vg
        elif dz > 0:
            sh[:, :, :D - dz] = Vg[:, :, dz:]
        else:
            sh[:, :, -dz:] = Vg[:, :, :D + dz]
        ref[:, k] = torch.einsum("prc,prd->pcd", dM.double(), sh.reshape(16, R, C1))
    L = _lib.lib()
    nbytes = L.forge_wino_wgrad_det_ws_bytes(C1, 0, n, D, Ht, Wt, Cout, kd)
    ws = _ws(nbytes, dev)
    common = lambda out: (_lib.ptr(dM), _lib.ptr(V), C1, 0, 0, None, 0, 0, 0, _lib.ptr(out), n, D, Ht, Wt, Cout, kd)

    def det(out, accumulate):
        _lib.check(L.forge_wino_wgrad_det(*common(out), accumulate, _lib.ptr(ws), nbytes, _lib.current_stream()), "forge_wino_wgrad_det")

    def atomic(out):
        _lib.check(L.forge_wino_wgrad(*common(out), _lib.current_stream()), "forge_wino_wgrad")
    _check_family(dev, det, atomic, (16, kd, Cout, C1), ref)


def test_conv_direct_wgrad_det(dev):
    n, D, H, W, Cin, Cout = 2, 12, 20, 24, 8, 3
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(n, D, H, W, Cout, generator=g).to(dev)
    x = torch.randn(n, D, H, W, Cin, generator=g).to(dev)
    ref = _ref_wgrad(dy, x, T27, 1, D)
    L = _lib.lib()
    ta = co._taps_array(T27)
    nbytes = L.forge_conv_direct_wgrad_det_ws_bytes(n, D, H, W, Cin, Cout, 27)
    ws = _ws(nbytes, dev)
    common = lambda out: (_lib.ptr(dy), Cout, _lib.ptr(x), Cin, _lib.ptr(out), n, D, H, W, Cin, Cout, ta, 27)

    def det(out, accumulate):
        _lib.check(L.forge_conv_direct_wgrad_det(*common(out), accumulate, _lib.ptr(ws), nbytes, _lib.current_stream()), "forge_conv_direct_wgrad_det")

    def atomic(out):
        _lib.check(L.forge_conv_direct_wgrad(*common(out), _lib.current_stream()), "forge_conv_direct_wgrad")
    _check_family(dev, det, atomic, (27, Cout, Cin), ref)


@pytest.mark.parametrize("slots", [False, True])
def test_rotate_bwd_det(dev, slots):
    n, C, D, H, W = 6, 32, 16, 16, 16
    g = torch.Generator().manual_seed(11)
    vox = torch.randn(n, D, H, W, C, generator=g).to(dev)
    dout = torch.randn(n, D, H, W, C, generator=g).to(dev)
    ang = torch.rand(n, generator=g) * 0.6
    xf = torch.zeros(n, 3, 4)
    xf[:, 0, 0], xf[:, 0, 1], xf[:, 1, 0], xf[:, 1, 1], xf[:, 2, 2] = ang.cos(), -ang.sin(), ang.sin(), ang.cos(), 1.0
    xf[:, :, 3] = torch.randn(n, 3, generator=g) * 0.1
    xf = xf.reshape(n, 12).to(dev)
    mode = torch.tensor([0, 1, 1, 1, 0, 1], dtype=torch.int32, device=dev)
    slot = torch.tensor([1, 0, 3, 2, 5, 4], dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = (L.forge_rotate_bwd_slots_det_ws_bytes if slots else L.forge_rotate_bwd_det_ws_bytes)(n, C, D, H, W)
    ws = _ws(nbytes, dev)
    head = (_lib.ptr(dout), _lib.ptr(vox), _lib.ptr(xf), _lib.ptr(mode)) + ((_lib.ptr(slot),) if slots else ())

    def det(out, accumulate):
        fn = L.forge_rotate_bwd_slots_det if slots else L.forge_rotate_bwd_det
        _lib.check(fn(*head, None, _lib.ptr(out), n, C, D, H, W, accumulate, _lib.ptr(ws), nbytes, _lib.current_stream()), "forge_rotate_bwd_det")

    def atomic(out):
        fn = L.forge_rotate_bwd_slots if slots else L.forge_rotate_bwd
        _lib.check(fn(*head, None, _lib.ptr(out), n, C, D, H, W, _lib.current_stream()), "forge_rotate_bwd")
    _check_family(dev, det, atomic, (n, 12), None, noise=1e-5)
    out = torch.full((n, 12), float("nan"), device=dev)
    det(out, 0)
    assert (out[mode == 0] == 0).all()                                                        # mode-0 volumes: written as zeros
    # the volume gradient of the _det entry is the default gather's, bitwise
    dv_a, dv_b = torch.empty_like(vox), torch.empty_like(vox)
    fn_d = L.forge_rotate_bwd_slots_det if slots else L.forge_rotate_bwd_det
    fn_a = L.forge_rotate_bwd_slots if slots else L.forge_rotate_bwd
    _lib.check(fn_d(*head, _lib.ptr(dv_a), None, n, C, D, H, W, 0, None, 0, _lib.current_stream()), "forge_rotate_bwd_det")
    _lib.check(fn_a(*head, _lib.ptr(dv_b), None, n, C, D, H, W, _lib.current_stream()), "forge_rotate_bwd")
    assert torch.equal(dv_a, dv_b)


# ------------------------------------------------------------------------------------------------------------- end to end
def _gt_pose_steps(dev, steps=3):
    """Three GT-pose training steps of FORGE_poseEstimator3D (fwd + bwd + clip + Adam) from a seeded state on a seeded synthetic sample;
    returns (losses, parameters)."""
    from forge_amd import train
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    sample = {k: v.to(dev) for k, v in syn.make_sample(1, 5, 256, 1.5, seed=3).items()}
    ds = syn.SyntheticDataset(1.5)
    losses = []
    for _ in range(steps):
        imgs, masks = model(sample, ds, dev)[:2]
        mi = train.grouped_mse(imgs.reshape(1, 10, 3, 256, 256), sample["images"], 5)
        mm = train.grouped_mse(masks.reshape(1, 10, 1, 256, 256), sample["fg_probabilities"], 5)
        loss = 5.0 * (mi[0] + mi[1]) + mm[0] + mm[1]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        train.clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return torch.stack(losses), {k: v.detach().clone() for k, v in model.named_parameters()}


def _assert_same_run(a, b):
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    diff = [k for k in a[1] if not torch.equal(a[1][k], b[1][k])]
    assert not diff, diff[:8]


def test_gt_pose_training_steps_bitwise_reproducible(dev):
    with forge_amd.deterministic(True):
        assert forge_amd.is_deterministic()
        a = _gt_pose_steps(dev)
        b = _gt_pose_steps(dev)
    _assert_same_run(a, b)
    assert torch.isfinite(a[0]).all()


def test_gt_pose_training_steps_follow_torch_flag(dev):
    forge_amd.set_deterministic(None)
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert forge_amd.is_deterministic()
        a = _gt_pose_steps(dev)
        b = _gt_pose_steps(dev)
    finally:
        torch.use_deterministic_algorithms(False)
    _assert_same_run(a, b)


def test_joint_step_gradients_bitwise_reproducible(dev):
    """The joint configs[4] step (tests/test_gpu_configs.py::joint_training_step: torch's flag on, so the deterministic path) run twice gives
    bitwise-identical gradients for every parameter and the same loss."""
    from test_gpu_configs import joint_training_step
    runs = []
    for _ in range(2):
        loss, _, model, _, _ = joint_training_step(dev)
        runs.append((loss.clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
        del model
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys() and len(runs[0][1]) > 0
    diff = [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
    assert not diff, diff[:8]


def test_refine_poses_bitwise_reproducible(dev):
    """refine_poses (the graph-replayed default path) twice with t = 5 views for 20 iterations in deterministic mode: identical poses and losses.
    (The graph is captured inside the block, so it replays the _det launches.)"""
    from forge_amd import geo_utils, refine
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    t = 5
    sample = syn.make_sample(1, t, 256, 1.5, seed=41)
    with torch.no_grad():
        feats = model.encoder_3d.get_feat3D(sample["images"][0].to(dev)).reshape(1, t, 128, 32, 32, 32)
        gt7 = geo_utils.mat2quat(sample["cam_poses_rel_cv2"][0, 1:]).to(dev)
        tgt_i, tgt_m, _, _, _ = refine._render_views(model, cfg, ds, feats, gt7, sample["K_cv2"].to(dev), dev)
    g = torch.Generator().manual_seed(9)
    init = gt7.clone()
    init[:, :4] = torch.nn.functional.normalize(init[:, :4] + 0.03 * torch.randn(t - 1, 4, generator=g).to(dev))
    init[:, 4:] += 0.02 * torch.randn(t - 1, 3, generator=g).to(dev)
    with forge_amd.deterministic(True):
        runs = [refine.refine_poses(model, cfg, ds, feats, init.clone(), tgt_i, tgt_m, sample["K_cv2"], dev, iter_num=20, log_every=5)
                for _ in range(2)]
    (pa, ha, _), (pb, hb, _) = runs
    assert torch.isfinite(pa).all() and (pa - init).abs().max().item() > 0
    assert torch.equal(pa, pb)
    assert ha == hb
