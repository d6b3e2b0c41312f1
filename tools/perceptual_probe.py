"""Timing of the VGG-16 perceptual loss (forge_amd/perceptual.py) on the MI355X.

  1. per-layer A/B: each of conv1_2 .. conv4_3, forward (ReLU epilogue) and data gradient, on Winograd F(2x2, 3x3) (one depth tap) and on the
     9-tap direct GEMM, at the shapes of `--pairs` pairs (2P images forward, P images backward);
  2. the module's forward + backward with device events after a warm-up, at 10 pairs (one GT-pose scene: b 2t = 10 views of 256^2) and 40
     pairs (four scenes), with the executed GFLOP from shapes, the fraction of the fp32-MFMA floor (157.3 TF) and the peak memory;
  3. train_step of the GT-pose model (b = 1) with and without the term (perceptual_img 0.02 / 0).

    python tools/perceptual_probe.py [--reps 10] [--skip-ab] [--skip-train]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from forge_amd import convops as co  # noqa: E402
from forge_amd import perceptual as fp  # noqa: E402

PEAK_TF = 157.3
SHAPES = [(224, 64, 64), (112, 64, 128), (112, 128, 128), (56, 128, 256), (56, 256, 256), (56, 256, 256), (28, 256, 512), (28, 512, 512),
          (28, 512, 512)]                                  # (H = W, Cin, Cout) of conv1_2 .. conv4_3


def timed(fn, reps, warm=2):
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


def executed_gflop(pairs, plan):
    """fp32 FLOPs the kernels execute per forward + backward: 2P images forward, P images data gradient; Winograd layers at 1/2.25 of direct."""
    f = 2 * 224 * 224 * 64 * 32 * (2 * pairs)                      # conv1_1 on the 32-wide patch rows
    f += 2 * 224 * 224 * 4 * 64 * 9 * pairs                          # conv1_1 data gradient (Cout 4)
    for name, (hw, cin, cout) in zip(fp.LAYER_NAMES[1:], SHAPES):
        d = 2 * hw * hw * cin * cout * 9
        fw, bw = plan[name]
        f += d * 2 * pairs / (2.25 if fw == "wino" else 1.0) + d * pairs / (2.25 if bw == "wino" else 1.0)
    return f / 1e9


def layer_ab(pairs, reps):
    dev = torch.device("cuda:0")
    out = []
    for name, (hw, cin, cout) in zip(fp.LAYER_NAMES[1:], SHAPES):
        w = torch.randn(cout, cin, 3, 3, device=dev) * (2.0 / (9 * cin)) ** 0.5
        row = {"layer": name, "H": hw, "Cin": cin, "Cout": cout}
        for mode in ("wino", "direct"):
            wp, _ = co.pack_conv2d_weight(w)
            L = {"cin": cin, "cout": cout, "bias": torch.zeros(cout, device=dev), "one": torch.ones(cout, device=dev), "zero": torch.zeros(cout, device=dev),
                 "wp": wp, "wT": wp.transpose(1, 2).contiguous(), "U": co.wino_pack_packed(wp) if mode == "wino" else None,
                 "UT": co.wino_pack_packed(wp, transpose=True) if mode == "wino" else None}
            x = torch.rand(2 * pairs, hw, hw, cin, device=dev)
            y = torch.empty(2 * pairs, hw, hw, cout, device=dev)
            d = torch.randn(pairs, hw, hw, cout, device=dev)
            row["fwd_" + mode] = timed(lambda: fp._conv(L, x, 2 * pairs, hw, hw, y), reps)
            row["dgrad_" + mode] = timed(lambda: fp._dgrad(L, d, pairs, hw, hw), reps)
            del x, y, d
        row["fwd_pick"] = "wino" if row["fwd_wino"] < row["fwd_direct"] else "direct"
        row["dgrad_pick"] = "wino" if row["dgrad_wino"] < row["dgrad_direct"] else "direct"
        print("A/B %d pairs %-8s H=%3d %3d->%3d  fwd wino %.3f direct %.3f ms | dgrad wino %.3f direct %.3f ms" % (
            pairs, name, hw, cin, cout, row["fwd_wino"], row["fwd_direct"], row["dgrad_wino"], row["dgrad_direct"]), flush=True)
        out.append(row)
    return out


def module_timing(pairs, reps, plan=None):
    dev = torch.device("cuda:0")
    m = fp.VGGPerceptualLoss(pretrained=False).to(dev)
    if plan is not None:
        m.plan = dict(plan)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(pairs, 3, 256, 256, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = torch.rand(pairs, 3, 256, 256, generator=g).to(dev)

    def fwd_bwd():
        x.grad = None
        m(x, y).backward()

    def fwd():
        with torch.no_grad():
            m(x, y)
    fwd_bwd()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t_fb = timed(fwd_bwd, reps)
    peak = torch.cuda.max_memory_allocated() - base
    t_f = timed(fwd, reps)
    gf = executed_gflop(pairs, m.plan)
    floor = gf / PEAK_TF                                          # GFLOP / (TFLOP/s) = ms
    wfloor = 38.0 * pairs / PEAK_TF                                # the all-Winograd-from-conv1_2 estimate (38 GFLOP per pair)
    r = {"pairs": pairs, "fwd_bwd_ms": t_fb, "fwd_only_ms": t_f, "executed_gflop": gf, "floor_ms": floor, "frac_of_floor": floor / t_fb,
         "wino_floor_ms": wfloor, "frac_of_wino_floor": wfloor / t_fb, "direct_equiv_gflop": 3 * 27.9 * pairs, "peak_mem_gb": peak / 1e9}
    print("module %d pairs: fwd+bwd %.3f ms (fwd %.3f ms), executed %.1f GFLOP, floor %.3f ms -> %.3f of floor (%.3f of the 38 GFLOP/pair floor "
          "%.3f ms), peak %.2f GB" % (pairs, t_fb, t_f, gf, floor, floor / t_fb, wfloor / t_fb, wfloor, peak / 1e9), flush=True)
    return r


def train_timing(reps):
    from forge_amd import synthetic as syn, train
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    dev = torch.device("cuda:0")
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    ds = syn.SyntheticDataset(1.5)
    sample = {k: v.to(dev) for k, v in syn.make_sample(1, 5, 256, 1.5, seed=0).items()}
    pl = fp.VGGPerceptualLoss(pretrained=False).to(dev)
    out = {}
    for w in (0.0, 0.02):
        cfg.loss.perceptual_img = w
        out["train_step_ms_perceptual_%g" % w] = timed(lambda: train.train_step(cfg, sample, ds, model, opt, dev, perceptual_loss=pl), reps)
    print("train_step b=1: %.2f ms without the term, %.2f ms with it" % (out["train_step_ms_perceptual_0"], out["train_step_ms_perceptual_0.02"]),
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "plan": fp.LAYER_PLAN}
    if not a.skip_ab:
        res["ab_10"] = layer_ab(10, a.reps)
        res["ab_40"] = layer_ab(40, a.reps)
    res["module"] = [module_timing(10, a.reps), module_timing(40, a.reps)]
    if not a.skip_ab:
        best = {r["layer"]: (r["fwd_pick"], r["dgrad_pick"]) for r in res["ab_40"]}
        res["module_ab40_plan"] = {"plan": best, "timing": [module_timing(10, a.reps, best), module_timing(40, a.reps, best)]}
    if not a.skip_train:
        res["train"] = train_timing(a.reps)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
