"""GPU (-m gpu): the image metrics (forge_amd/metrics.py) against the float64 restatements of tests/test_metrics_cpu.py, on random, smooth and
render-like images (flat background plus an object: the cancellation case of SSIM's variances); determinism, batch independence, hipGraph
capture, the compute_img_metric drop-in, and the perceptual loss through the shared VGG trunk."""
import numpy as np
import pytest
import torch

from forge_amd import metrics as fm
from forge_amd import perceptual as fp
from test_metrics_cpu import lpips_ref, psnr_ref, ssim_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lp(dev):
    return fm.LPIPS(pretrained=False, seed=0).to(dev)


def images(kind, n, H, W, seed=0):
    """A pair of float32 [n, 3, H, W] batches in [0, 1] (CPU): 'random' (independent uniform), 'smooth' (low-frequency sinusoids, the second a
    perturbed copy) or 'render' (a flat 0.9 background shared by both images, a textured disc that differs between them)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.rand(n, 3, H, W, generator=g), torch.rand(n, 3, H, W, generator=g)
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ph = torch.rand(n, 3, 4, generator=g) * 6.283

    def wave(f, k):
        return torch.sin(f * 6.283 * yy + ph[:, :, k, None, None]) * torch.cos(f * 4.0 * xx + ph[:, :, k + 1, None, None])
    if kind == "smooth":
        a = 0.5 + 0.35 * wave(1.5, 0)
        return a.contiguous(), (a + 0.05 * wave(3.0, 2)).clamp(0, 1).contiguous()
    assert kind == "render"
    disc = (((yy - 0.5) ** 2 + (xx - 0.45) ** 2) < 0.08).float()
    tex = 0.45 + 0.3 * wave(4.0, 0)
    a = 0.9 * (1 - disc) + disc * tex
    b = 0.9 * (1 - disc) + disc * (tex + 0.04 * torch.randn(n, 3, H, W, generator=g)).clamp(0, 1)
    return a.contiguous(), b.contiguous()


STAT_CASES = [("random", 3, 256, 256), ("smooth", 2, 256, 256), ("render", 5, 256, 256), ("random", 1, 37, 53), ("smooth", 2, 37, 53),
              ("render", 4, 37, 53)]


@pytest.mark.parametrize("kind,n,H,W", STAT_CASES)
def test_psnr_and_ssim_against_float64(dev, kind, n, H, W):
    a, b = images(kind, n, H, W, seed=n + H)
    ad, bd = a.to(dev), b.to(dev).contiguous(memory_format=torch.channels_last)        # one operand strided
    p, s = fm.psnr(ad, bd), fm.ssim(ad, bd)
    assert p.dtype == torch.float64 and s.dtype == torch.float64 and p.shape == (n,) and s.shape == (n,) and p.device == ad.device
    for i in range(n):
        x, y = a[i].numpy(), b[i].numpy()
        assert np.mean((x.astype(np.float64) - y) ** 2) >= 1e-8
        assert abs(p[i].item() - psnr_ref(x, y)) < 1e-4, (kind, i)
        assert abs(s[i].item() - ssim_ref(x, y)) < 1e-5, (kind, i)


def test_identical_images(dev, lp):
    a, _ = images("render", 2, 64, 48)
    ad = a.to(dev)
    assert torch.isinf(fm.psnr(ad, ad.clone())).all() and (fm.psnr(ad, ad.clone()) > 0).all()
    assert torch.allclose(fm.ssim(ad, ad.clone()), torch.ones(2, dtype=torch.float64, device=dev), rtol=0, atol=1e-12)
    assert torch.equal(lp(ad, ad.clone()), torch.zeros(2, 1, 1, 1, device=dev))


@pytest.mark.parametrize("kind,n,H,W,normalize", [("render", 1, 256, 256, False), ("smooth", 2, 64, 96, False), ("random", 3, 48, 80, False),
                                                  ("render", 2, 48, 80, True)])
def test_lpips_against_float64(dev, lp, kind, n, H, W, normalize):
    a, b = images(kind, n, H, W, seed=7 * n + W)
    got = lp(a.to(dev), b.to(dev), normalize=normalize)
    assert got.shape == (n, 1, 1, 1) and got.dtype == torch.float32
    want = lpips_ref(lp.state_dict(), a, b, normalize=normalize)
    rel = ((got.view(-1).double().cpu() - want).abs() / want).max().item()
    assert rel < 1e-4, (kind, rel, got.view(-1).tolist(), want.tolist())


def test_lpips_never_requires_grad(dev, lp):
    a, b = images("random", 1, 32, 32)
    x = a.to(dev).requires_grad_(True)
    out = lp(x, b.to(dev))
    assert not out.requires_grad and out.grad_fn is None
    assert not fm.image_metrics(x, b.to(dev), lp)["lpips"].requires_grad


def test_two_calls_are_bitwise_equal(dev, lp):
    a, b = (t.to(dev) for t in images("render", 5, 256, 256, seed=3))
    r1, r2 = fm.image_metrics(a, b, lp), fm.image_metrics(a, b, lp)
    for k in ("psnr", "ssim", "lpips"):
        assert torch.equal(r1[k], r2[k]), k


def test_each_pair_of_a_batch_equals_its_single_call(dev, lp):
    a, b = (t.to(dev) for t in images("smooth", 5, 256, 256, seed=5))
    batch = fm.image_metrics(a, b, lp)
    for i in range(5):
        one = fm.image_metrics(a[i:i + 1], b[i:i + 1], lp)
        for k in ("psnr", "ssim", "lpips"):
            assert torch.equal(batch[k][i:i + 1], one[k]), (k, i)


def test_graph_capture_replays_to_the_eager_result(dev, lp):
    a, b = (t.to(dev) for t in images("render", 5, 256, 256, seed=11))
    eager = fm.image_metrics(a, b, lp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fm.image_metrics(a, b, lp)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fm.image_metrics(a, b, lp)
    g.replay()
    torch.cuda.synchronize()
    for k in ("psnr", "ssim", "lpips"):
        assert torch.equal(out[k], eager[k]), k


def test_compute_img_metric_is_the_drop_in(dev):
    a, b = images("render", 1, 64, 80, seed=2)
    rgb, gt = a[0].permute(1, 2, 0).numpy(), b[0].permute(1, 2, 0).numpy()       # HWC, as kubric_eval.py passes them
    p, s = fm.compute_img_metric(rgb, gt)
    assert isinstance(p, float) and isinstance(s, float)
    assert p == fm.psnr(a.to(dev), b.to(dev))[0].item() and s == fm.ssim(a.to(dev), b.to(dev))[0].item()
    assert abs(p - psnr_ref(gt.transpose(2, 0, 1), rgb.transpose(2, 0, 1))) < 1e-4
    assert abs(s - ssim_ref(gt.transpose(2, 0, 1), rgb.transpose(2, 0, 1))) < 1e-5


# The perceptual loss of the parent commit (before the VGG trunk was shared with LPIPS) on these inputs, as float32 bits: the shared trunk must
# leave it bitwise unchanged.
PERCEPTUAL_BITS = {True: 0x3E53C952, False: 0x3E56436D}


@pytest.mark.parametrize("resize", [True, False])
def test_perceptual_loss_is_unchanged_by_the_shared_trunk(dev, resize):
    m = fp.VGGPerceptualLoss(resize=resize, pretrained=False, seed=0).to(dev)
    a, b = images("smooth", 2, 64, 96, seed=1)
    loss = m(a.to(dev), b.to(dev))
    bits = int(np.array([loss.item()], np.float32).view(np.uint32)[0])
    assert bits == PERCEPTUAL_BITS[resize], hex(bits)
