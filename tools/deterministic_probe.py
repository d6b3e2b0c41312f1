#!/usr/bin/env python
"""Cost of the deterministic mode (forge_amd.deterministic): default vs deterministic step time, alternating in one process.

    python tools/deterministic_probe.py [--repeats R] [--steps K] [--out profiles/det_probe.json]
    DET_PROBE_ONLY=gt4 DET_PROBE_MODE=det python tools/deterministic_probe.py --repeats 1 --steps 3     # one workload in one mode (rocprofv3 pass)

Workloads: the GT-pose training step (FORGE_poseEstimator3D, fwd + bwd + clip + Adam; tools/train_step_probe.py) at 1 and 4 scenes and the
joint 2D3D step (FORGE, predicted poses; tools/joint_step_probe.py) at 4 scenes. Each repeat times K steps in default mode, then K in
deterministic mode (after one warm-up step in each), device-synchronised; the table reports the median ms per step and the ratio."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import forge_amd  # noqa: E402
from forge_amd import synthetic as syn, train  # noqa: E402


def gt_pose(b, dev):
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, fused=True)
    sample = {k: v.to(dev) for k, v in syn.make_sample(b, 5, 256, 1.5, seed=3).items()}
    ds = syn.SyntheticDataset(1.5)

    def step():
        imgs, masks = model(sample, ds, dev)[:2]
        mi = train.grouped_mse(imgs.reshape(b, 10, 3, 256, 256), sample["images"], 5)
        mm = train.grouped_mse(masks.reshape(b, 10, 1, 256, 256), sample["fg_probabilities"], 5)
        loss = 5.0 * (mi[0] + mi[1]) + mm[0] + mm[1]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        train.clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        return loss
    return step


def joint(b, dev):
    from forge_amd.model import FORGE
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    cfg.loss.regu_origin_proj = 1.0
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    params = [p for m in (model.encoder_traj, model.pose_head, model.encoder_3d.fusion_feature, model.encoder_3d.density_head, model.render)
              for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=1e-4, fused=True)
    sample = {k: v.to(dev) for k, v in syn.make_sample(b, 10, 256, 1.5, seed=12).items()}
    ds = syn.SyntheticDataset(1.5)

    def step():
        loss, _, _, _ = train.compute_all_loss_nvs(cfg, 0, sample, ds, model, {}, dev)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        train.clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        return loss
    return step


WORKLOADS = {"gt1": ("GT-pose step, 1 scene", gt_pose, 1), "gt4": ("GT-pose step, 4 scenes", gt_pose, 4), "joint4": ("joint step, 4 scenes", joint, 4)}


def timed(step, mode, k):
    with forge_amd.deterministic(mode):
        step()                                            # warm-up in this mode (workspace sizes, kernel loads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            step()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    only = os.environ.get("DET_PROBE_ONLY")
    force = os.environ.get("DET_PROBE_MODE")              # "det" / "default": one mode only (profiling passes)
    rows = []
    for key, (name, make, b) in WORKLOADS.items():
        if only and key != only:
            continue
        step = make(b, dev)
        step()
        torch.cuda.synchronize()
        if force:
            ms = timed(step, force == "det", a.steps)
            print("%-24s %s: %.2f ms/step" % (name, force, ms), flush=True)
            continue
        base, det = [], []
        for _ in range(a.repeats):                        # alternate: default, deterministic, default, ...
            base.append(timed(step, False, a.steps))
            det.append(timed(step, True, a.steps))
        mb, md = statistics.median(base), statistics.median(det)
        rows.append({"workload": name, "key": key, "default_ms": base, "det_ms": det, "default_median_ms": mb, "det_median_ms": md, "ratio": md / mb})
        print("%-24s default %8.2f ms  deterministic %8.2f ms  ratio %.3f   (medians of %d x %d steps; default %s, det %s)"
              % (name, mb, md, md / mb, a.repeats, a.steps, ["%.2f" % v for v in base], ["%.2f" % v for v in det]), flush=True)
        del step
        torch.cuda.empty_cache()
    if a.out and rows:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
