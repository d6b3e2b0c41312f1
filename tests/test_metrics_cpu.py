"""CPU: the image metrics' surface (forge_amd/metrics.py) - the LPIPS state_dict layout, both lin-weight spellings, the no-download weight lookup,
the argument checks of the Python API and of the new C entries - and the float64 restatements of SSIM and LPIPS that tests/test_gpu_metrics.py
measures the kernels against, pinned by known answers (neither skimage nor lpips is importable here)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from forge_amd import _lib
from forge_amd import metrics as fm
from forge_amd import perceptual as fp

K1, K2 = 0.01, 0.03
TAP_ENDS = (3, 8, 15, 22, 29)                      # features index of relu1_2, relu2_2, relu3_3, relu4_3, relu5_3


# -------------------------------------------------------------------------------------------------------------------- float64 restatements
def psnr_ref(a, b, data_range=1.0):
    """skimage.metrics.peak_signal_noise_ratio on [C, H, W] arrays, in float64."""
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return np.inf if mse == 0 else 10.0 * np.log10(data_range ** 2 / mse)


def ssim_ref(a, b, data_range=1.0):
    """skimage.metrics.structural_similarity(multichannel=True, data_range) with the defaults (7x7 uniform window, sample covariance) on
    [C, H, W] arrays, in float64: the mean of the SSIM map over every valid 7x7 window (skimage's crop of 3 pixels) and over channels."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    win = np.lib.stride_tricks.sliding_window_view
    vals = []
    for x, y in zip(a, b):
        wx, wy = win(x, (7, 7)), win(y, (7, 7))                    # [H - 6, W - 6, 7, 7]: every valid window
        ux, uy = wx.mean(axis=(2, 3)), wy.mean(axis=(2, 3))
        vx = (wx * wx).mean(axis=(2, 3)) - ux * ux
        vy = (wy * wy).mean(axis=(2, 3)) - uy * uy
        vxy = (wx * wy).mean(axis=(2, 3)) - ux * uy
        vx, vy, vxy = (49.0 / 48.0) * vx, (49.0 / 48.0) * vy, (49.0 / 48.0) * vxy
        s = (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        vals.append(s.mean())
    return float(np.mean(vals))


def lpips_ref(state_dict, in0, in1, normalize=False):
    """lpips.LPIPS(net='vgg', version='0.1') forward in float64 on the CPU from an LPIPS state_dict: [N] values."""
    sd = {k: v.detach().double().cpu() for k, v in state_dict.items()}
    feats = fp.vgg16_features()[:30].double()
    fsd = {}
    for k, v in sd.items():
        if k.startswith("net.slice"):
            _, _, n, leaf = k.split(".")
            fsd["%s.%s" % (n, leaf)] = v
    feats.load_state_dict(fsd, strict=True)
    x0, x1 = in0.double().cpu(), in1.double().cpu()
    if normalize:
        x0, x1 = 2 * x0 - 1, 2 * x1 - 1
    shift, scale = sd["scaling_layer.shift"], sd["scaling_layer.scale"]
    h0, h1 = (x0 - shift) / scale, (x1 - shift) / scale
    total = torch.zeros(x0.shape[0], dtype=torch.float64)
    k = 0
    with torch.no_grad():
        for i, layer in enumerate(feats):
            h0, h1 = layer(h0), layer(h1)
            if i in TAP_ENDS:
                n0 = h0 / (h0.square().sum(1, keepdim=True).sqrt() + 1e-10)
                n1 = h1 / (h1.square().sum(1, keepdim=True).sqrt() + 1e-10)
                d = F.conv2d((n0 - n1).square(), sd["lin%d.model.1.weight" % k])
                total += d.mean(dim=(1, 2, 3))
                k += 1
    return total


# -------------------------------------------------------------------------------------------------------------------- restatements' known answers
def test_ssim_ref_of_constant_images():
    for a, b in ((0.2, 0.7), (0.0, 1.0), (0.5, 0.5)):
        x, y = np.full((3, 12, 9), a), np.full((3, 12, 9), b)
        c1 = K1 ** 2
        assert abs(ssim_ref(x, y) - (2 * a * b + c1) / (a * a + b * b + c1)) < 1e-12


def test_ssim_ref_of_one_window_by_hand():
    rng = np.random.default_rng(3)
    x, y = rng.random((1, 7, 7)), rng.random((1, 7, 7))
    xs, ys = x.ravel().tolist(), y.ravel().tolist()
    mx, my = sum(xs) / 49, sum(ys) / 49
    vx = sum((u - mx) ** 2 for u in xs) / 48
    vy = sum((v - my) ** 2 for v in ys) / 48
    cxy = sum((u - mx) * (v - my) for u, v in zip(xs, ys)) / 48
    c1, c2 = K1 ** 2, K2 ** 2
    want = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    assert abs(ssim_ref(x, y) - want) < 1e-12


def test_ssim_ref_of_an_image_with_itself_is_one():
    x = np.random.default_rng(0).random((3, 20, 31))
    assert abs(ssim_ref(x, x) - 1.0) < 1e-12


def test_psnr_ref_of_a_known_mse():
    x = np.random.default_rng(1).random((3, 16, 16)) * 0.5
    assert abs(psnr_ref(x, x + 0.1) - 20.0) < 1e-9                 # mse 0.01
    assert abs(psnr_ref(x, x + 0.1, data_range=2.0) - 10 * np.log10(400.0)) < 1e-9
    assert psnr_ref(x, x) == np.inf


def test_lpips_ref_of_an_image_with_itself_is_zero():
    m = fm.LPIPS(pretrained=False, seed=1)
    x = torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(0))
    assert torch.equal(lpips_ref(m.state_dict(), x, x), torch.zeros(2, dtype=torch.float64))


def test_lpips_ref_with_one_lin_weight_is_that_taps_mean():
    m = fm.LPIPS(pretrained=False, seed=2)
    sd = m.state_dict()
    for k in range(5):
        sd["lin%d.model.1.weight" % k].zero_()
    sd["lin1.model.1.weight"][0, 5] = 2.0                          # relu2_2, channel 5
    g = torch.Generator().manual_seed(1)
    x0, x1 = torch.rand(1, 3, 32, 32, generator=g), torch.rand(1, 3, 32, 32, generator=g)
    w = {k: v.double() for k, v in sd.items()}

    def relu2_2(x):
        h = (x.double() - w["scaling_layer.shift"]) / w["scaling_layer.scale"]
        for i in (0, 2):
            h = F.relu(F.conv2d(h, w["net.slice1.%d.weight" % i], w["net.slice1.%d.bias" % i], padding=1))
        h = F.max_pool2d(h, 2)
        for i in (5, 7):
            h = F.relu(F.conv2d(h, w["net.slice2.%d.weight" % i], w["net.slice2.%d.bias" % i], padding=1))
        return h[0]                                                # [128, 16, 16]
    f0, f1 = relu2_2(x0), relu2_2(x1)
    n0, n1 = f0.norm(dim=0) + 1e-10, f1.norm(dim=0) + 1e-10
    want = (2.0 * (f0[5] / n0 - f1[5] / n1) ** 2).mean().item()
    got = lpips_ref(sd, x0, x1).item()
    assert want > 0 and abs(got - want) <= 1e-12 * want


# -------------------------------------------------------------------------------------------------------------------- LPIPS module surface
def test_lpips_state_dict_keys_and_shapes():
    m = fm.LPIPS(pretrained=False)
    want = [("scaling_layer.shift", (1, 3, 1, 1)), ("scaling_layer.scale", (1, 3, 1, 1))]
    idx, cin, s = 0, 3, 1
    for v in fp.VGG16_CFG[:17]:
        if v == "M":
            idx += 1
            s += 1
            continue
        want += [("net.slice%d.%d.weight" % (s, idx), (v, cin, 3, 3)), ("net.slice%d.%d.bias" % (s, idx), (v,))]
        cin, idx = v, idx + 2
    want += [("lin%d.model.1.weight" % k, (1, c, 1, 1)) for k, c in enumerate((64, 128, 256, 512, 512))]
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert torch.allclose(m.scaling_layer.shift.view(3), torch.tensor([-0.030, -0.088, -0.188]))
    assert torch.allclose(m.scaling_layer.scale.view(3), torch.tensor([0.458, 0.448, 0.450]))
    assert not any(p.requires_grad for p in m.parameters()) and not m.training


def test_vgg_weights_are_the_perceptual_modules():
    a = fm.LPIPS(pretrained=False, seed=4)
    tv = fp.seeded_vgg16_state_dict(4)
    for k, v in a.state_dict().items():
        if k.startswith("net."):
            _, s, n, leaf = k.split(".")
            assert torch.equal(v, tv["features.%s.%s" % (n, leaf)]), k
    b = fm.LPIPS(pretrained=False, seed=9, vgg_weights=tv)
    assert torch.equal(getattr(b.net.slice5, "28").weight, tv["features.28.weight"])
    with pytest.raises(KeyError):
        fm.LPIPS(pretrained=False, vgg_weights={k: v for k, v in tv.items() if k != "features.26.bias"})


def test_both_lin_key_spellings_load_identically(tmp_path):
    lins = fm.seeded_lin_state_dict(7)
    alt = {k.replace("lin", "lins.", 1): v for k, v in lins.items()}
    a = fm.LPIPS(pretrained=False, model_path=lins)
    b = fm.LPIPS(pretrained=False, model_path=alt)
    p = tmp_path / "vgg.pth"
    torch.save(alt, str(p))
    c = fm.LPIPS(pretrained=False, model_path=str(p))
    d = fm.LPIPS(pretrained=False, seed=1)
    d.load_state_dict(dict(a.state_dict(), **{k.replace("lin", "lins.", 1): v for k, v in lins.items() if k.startswith("lin")}), strict=True)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) and torch.equal(v, c.state_dict()[k]) and torch.equal(v, d.state_dict()[k]), k
    assert all((v >= 0).all() for v in lins.values())


def test_lin_weights_from_the_environment(tmp_path, monkeypatch):
    p = tmp_path / "lin.pth"
    torch.save(fm.seeded_lin_state_dict(3), str(p))
    monkeypatch.setenv("FORGE_LPIPS_WEIGHTS", str(p))
    assert fm.default_lin_path() == str(p)
    m = fm.LPIPS(vgg_weights=fp.seeded_vgg16_state_dict(0))
    assert torch.equal(m.lin3.model[1].weight, fm.seeded_lin_state_dict(3)["lin3.model.1.weight"])


def test_weight_lookup_never_downloads(tmp_path, monkeypatch):
    import socket
    monkeypatch.delenv("FORGE_LPIPS_WEIGHTS", raising=False)
    monkeypatch.delenv("FORGE_VGG16_WEIGHTS", raising=False)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    monkeypatch.setattr("importlib.util.find_spec", lambda name, *a: None)

    def no_net(*a, **kw):
        raise AssertionError("LPIPS tried to open a network connection")
    monkeypatch.setattr(socket, "create_connection", no_net)
    monkeypatch.setattr(socket.socket, "connect", no_net)
    with pytest.raises(FileNotFoundError) as e:
        fm.LPIPS(vgg_weights=fp.seeded_vgg16_state_dict(0))
    assert "FORGE_LPIPS_WEIGHTS" in str(e.value) and "model_path" in str(e.value) and "lpips" in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        fm.LPIPS(model_path=fm.seeded_lin_state_dict(0))               # the VGG weights: perceptual.py's lookup
    assert "FORGE_VGG16_WEIGHTS" in str(e.value)


@pytest.mark.parametrize("kw", [{"net": "alex"}, {"net": "squeeze"}, {"version": "0.0"}, {"lpips": False}, {"spatial": True}])
def test_unsupported_options_raise(kw):
    with pytest.raises(ValueError):
        fm.LPIPS(pretrained=False, **kw)


# -------------------------------------------------------------------------------------------------------------------- argument checks
def test_host_tensors_raise():
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.psnr(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.ssim(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.LPIPS(pretrained=False)(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.image_metrics(x, x)


def test_shape_checks_come_before_any_launch(monkeypatch):
    """ValueError cases: mismatched shapes / channels, SSIM below 7 pixels, LPIPS extents not divisible by 16, LPIPS on C != 3. The checks are
    exercised with meta tensors posing as device tensors: they must raise before anything touches a device."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    m = fm.LPIPS(pretrained=False)
    m.scaling_layer.shift = torch.empty(1, 3, 1, 1, device="meta")
    meta = lambda *s: torch.empty(*s, device="meta")                      # noqa: E731
    with pytest.raises(ValueError):
        fm.psnr(meta(2, 3, 16, 16), meta(2, 3, 16, 17))
    with pytest.raises(ValueError):
        fm.ssim(meta(2, 3, 16, 16), meta(2, 1, 16, 16))
    with pytest.raises(ValueError):
        fm.psnr(meta(3, 16, 16), meta(3, 16, 16))
    with pytest.raises(ValueError, match="7x7"):
        fm.ssim(meta(1, 3, 6, 40), meta(1, 3, 6, 40))
    with pytest.raises(ValueError, match="7x7"):
        fm.ssim(meta(1, 3, 40, 5), meta(1, 3, 40, 5))
    with pytest.raises(ValueError, match="multiples of 16"):
        m(meta(1, 3, 40, 48), meta(1, 3, 40, 48))
    with pytest.raises(ValueError, match="multiples of 16"):
        m(meta(1, 3, 48, 72), meta(1, 3, 48, 72))
    with pytest.raises(ValueError, match="3-channel"):
        m(meta(1, 1, 32, 32), meta(1, 1, 32, 32))
    with pytest.raises(ValueError):
        m(meta(2, 3, 32, 32), meta(1, 3, 32, 32))
    with pytest.raises(TypeError):
        fm.psnr(meta(1, 3, 8, 8).double(), meta(1, 3, 8, 8).double())


def test_compute_img_metric_checks_its_arrays():
    with pytest.raises(ValueError):
        fm.compute_img_metric(np.zeros((8, 8, 3), np.float32), np.zeros((8, 9, 3), np.float32))
    with pytest.raises(ValueError):
        fm.compute_img_metric(np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float32))


def test_c_entries_check_their_arguments(built_lib):
    l = _lib.lib()
    fake = 0x1000                                    # never dereferenced: argument checks run before any launch
    odd = 0x1004                                     # not 16-byte aligned
    nb = l.forge_metric_blocks()
    assert nb > 0 and l.forge_ssim_tiles(256, 256) > 0 and l.forge_ssim_tiles(6, 256) == -1 and l.forge_ssim_tiles(256, 6) == -1
    s = (1, 1, 1, 1)
    assert l.forge_psnr(None, *s, fake, *s, 1, 3, 8, 8, 1.0, fake, fake, None) == -1
    assert l.forge_psnr(fake, *s, fake, *s, 0, 3, 8, 8, 1.0, fake, fake, None) == -1
    assert l.forge_psnr(fake, *s, fake, *s, 1, 3, 8, 8, 0.0, fake, fake, None) == -1
    assert b"forge_psnr" in l.forge_last_error()
    assert l.forge_ssim(fake, *s, fake, *s, 1, 3, 6, 8, 1.0, fake, fake, None) == -2
    assert b"7x7" in l.forge_last_error()
    assert l.forge_ssim(fake, *s, None, *s, 1, 3, 8, 8, 1.0, fake, fake, None) == -1
    assert l.forge_ssim(fake, *s, fake, *s, 1, 3, 8, -1, 1.0, fake, fake, None) == -1
    assert l.forge_lpips_tap(fake, 1, 16, 96, fake, fake, None) == -2
    assert l.forge_lpips_tap(odd, 1, 16, 64, fake, fake, None) == -2
    assert l.forge_lpips_tap(fake, 1, 16, 64, odd, fake, None) == -2
    assert l.forge_lpips_tap(fake, 0, 16, 64, fake, fake, None) == -1
    assert l.forge_lpips_tap(fake, 1, 16, 64, fake, None, None) == -1
    assert l.forge_lpips_finalize(fake, 1, 1, 1, 1, 0, 1, fake, None) == -1
    assert l.forge_lpips_finalize(None, 1, 1, 1, 1, 1, 1, fake, None) == -1
    with pytest.raises(RuntimeError, match="forge_lpips_tap"):
        _lib.check(l.forge_lpips_tap(fake, 1, 16, 96, fake, fake, None), "forge_lpips_tap")
