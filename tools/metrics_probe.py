"""Accuracy and timing of the image metrics (forge_amd/metrics.py) on the MI355X.

  1. accuracy: the largest errors of psnr / ssim / LPIPS against the float64 restatements of tests/test_metrics_cpu.py on the test suite's
     image families (random, smooth, render-like) at 256^2 and non-square sizes;
  2. conv5 plan A/B: conv5_1 .. conv5_3 forward at H/16 of 256^2 inputs (2P images) on Winograd F(2x2, 3x3) and on the 9-tap direct GEMM,
     then the LPIPS module with each conv5 plan, at 5 and 40 pairs;
  3. image_metrics (PSNR + SSIM + LPIPS) with device events after a warm-up at 5 pairs of 256^2 (one scene's novel views) and 40 pairs, with
     PSNR + SSIM alone and LPIPS alone, and LPIPS against the floor of its direct-convolution FLOPs (40.1 GFLOP per 256^2 image) at the
     fp32 peak (157.3 TF).

    python tools/metrics_probe.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from forge_amd import convops as co  # noqa: E402
from forge_amd import metrics as fm  # noqa: E402
from forge_amd import perceptual as fp  # noqa: E402

PEAK_TF = 157.3
CONV5 = ("conv5_1", "conv5_2", "conv5_3")


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def lpips_gflop_per_image(H=256, W=256):
    """Direct-convolution FLOPs of VGG-16 features[:30] on one H x W image."""
    f, cin, h, w = 0, 3, H, W
    for v in fp.VGG16_CFG[:17]:
        if v == "M":
            h, w = h // 2, w // 2
            continue
        f += 2 * h * w * cin * v * 9
        cin = v
    return f / 1e9


def accuracy(dev):
    from test_gpu_metrics import STAT_CASES, images
    from test_metrics_cpu import lpips_ref, psnr_ref, ssim_ref
    worst = {"psnr_db": 0.0, "ssim_abs": 0.0, "lpips_rel": 0.0}
    for kind, n, H, W in STAT_CASES:
        a, b = images(kind, n, H, W, seed=n + H)
        p, s = fm.psnr(a.to(dev), b.to(dev)).cpu(), fm.ssim(a.to(dev), b.to(dev)).cpu()
        for i in range(n):
            x, y = a[i].numpy(), b[i].numpy()
            e_p, e_s = abs(p[i].item() - psnr_ref(x, y)), abs(s[i].item() - ssim_ref(x, y))
            worst["psnr_db"], worst["ssim_abs"] = max(worst["psnr_db"], e_p), max(worst["ssim_abs"], e_s)
        print("accuracy %-6s %d x %dx%d  psnr err %.2e dB  ssim err %.2e" % (kind, n, H, W, worst["psnr_db"], worst["ssim_abs"]), flush=True)
    lp = fm.LPIPS(pretrained=False).to(dev)
    for kind, n, H, W, norm in (("render", 1, 256, 256, False), ("smooth", 2, 64, 96, False), ("random", 3, 48, 80, False), ("render", 2, 48, 80, True),
                                ("random", 1, 256, 256, False)):
        a, b = images(kind, n, H, W, seed=7 * n + W)
        got = lp(a.to(dev), b.to(dev), normalize=norm).view(-1).double().cpu()
        want = lpips_ref(lp.state_dict(), a, b, normalize=norm)
        rel = ((got - want).abs() / want).max().item()
        worst["lpips_rel"] = max(worst["lpips_rel"], rel)
        print("accuracy lpips %-6s %d x %dx%d normalize=%d  rel err %.2e  (values %s)" % (kind, n, H, W, norm, rel, [round(v, 5) for v in want.tolist()]),
              flush=True)
    return worst


def conv5_ab(pairs, reps, dev):
    hw, c = 16, 512
    w = torch.randn(c, c, 3, 3, device=dev) * (2.0 / (9 * c)) ** 0.5
    wp, _ = co.pack_conv2d_weight(w)
    x = torch.rand(2 * pairs, hw, hw, c, device=dev)
    y = torch.empty(2 * pairs, hw, hw, c, device=dev)
    row = {"pairs": pairs, "H": hw}
    for mode in ("wino", "direct"):
        L = {"cin": c, "cout": c, "bias": torch.zeros(c, device=dev), "one": torch.ones(c, device=dev), "zero": torch.zeros(c, device=dev),
             "wp": wp, "U": co.wino_pack_packed(wp) if mode == "wino" else None}
        row["layer_" + mode + "_ms"] = timed(lambda: fp._conv(L, x, 2 * pairs, hw, hw, y), reps)
    print("conv5 A/B %d pairs (one 512->512 layer at 16^2, %d images): wino %.4f ms  direct %.4f ms" % (pairs, 2 * pairs, row["layer_wino_ms"],
                                                                                                      row["layer_direct_ms"]), flush=True)
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(pairs, 3, 256, 256, generator=g).to(dev), torch.rand(pairs, 3, 256, 256, generator=g).to(dev)
    for mode in ("wino", "direct"):
        lp = fm.LPIPS(pretrained=False).to(dev)
        for n in CONV5:
            lp.plan[n] = (mode, None)
        row["lpips_" + mode + "_ms"] = timed(lambda: lp(a, b), reps)
    print("conv5 A/B %d pairs: LPIPS with conv5 on wino %.3f ms, on direct %.3f ms" % (pairs, row["lpips_wino_ms"], row["lpips_direct_ms"]), flush=True)
    return row


def protocol(pairs, reps, dev):
    g = torch.Generator().manual_seed(1)
    a, b = torch.rand(pairs, 3, 256, 256, generator=g).to(dev), torch.rand(pairs, 3, 256, 256, generator=g).to(dev)
    lp = fm.LPIPS(pretrained=False).to(dev)
    r = {"pairs": pairs}
    r["image_metrics_ms"] = timed(lambda: fm.image_metrics(a, b, lp), reps)
    r["psnr_ssim_ms"] = timed(lambda: fm.image_metrics(a, b), reps)
    r["lpips_ms"] = timed(lambda: lp(a, b), reps)
    r["lpips_floor_ms"] = lpips_gflop_per_image() * 2 * pairs / PEAK_TF
    r["lpips_frac_of_floor"] = r["lpips_floor_ms"] / r["lpips_ms"]
    print("image_metrics %d pairs of 256^2: %.3f ms (PSNR + SSIM %.3f ms, LPIPS %.3f ms = %.3f of its %.3f ms floor)" % (
        pairs, r["image_metrics_ms"], r["psnr_ssim_ms"], r["lpips_ms"], r["lpips_frac_of_floor"], r["lpips_floor_ms"]), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-accuracy", action="store_true")
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "lpips_gflop_per_image": lpips_gflop_per_image(),
           "conv5_plan": {n: fp.LAYER_PLAN[n][0] for n in CONV5}}
    print("LPIPS VGG-16 features[:30] at 256^2: %.2f GFLOP per image (direct convolution)" % res["lpips_gflop_per_image"], flush=True)
    if not a.skip_accuracy:
        res["accuracy_max"] = accuracy(dev)
    if not a.skip_ab:
        res["conv5_ab"] = [conv5_ab(5, a.reps, dev), conv5_ab(40, a.reps, dev)]
    res["protocol"] = [protocol(5, a.reps, dev), protocol(40, a.reps, dev)]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
