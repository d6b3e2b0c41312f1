#!/usr/bin/env python
"""The evaluation protocol on the MI355X (forge_amd/evaluation.py), timed:

  - predict_initial + evaluate_all for one scene (one encoder pass, the pose estimators on a batch of five clips, the five canonical choices
    scored as one batch of five scenes, one read-out) against the same work as five sequential passes through the same modules: per canonical
    choice one encoder pass, one pose-estimator pass and one evaluate with its own read-out - the only way without evaluation.py;
  - ops.pose_sync (forge_pose_sync) at N = 5 with all ten pairs, B = 1 and B = 64, eager launches.
Both versions are warmed up, then timed alternately; host clock around a device synchronise. Scene and model: the protocol goldens'
(tools/make_golden_eval_protocol.py), seeded weights.

    python tools/probe_eval_protocol.py [--reps 10]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from forge_amd import evaluation as ev, metrics as fm, ops, synthetic as syn  # noqa: E402
from forge_amd.model import FORGE  # noqa: E402
from make_golden_eval_protocol import eval_config, eval_dataset, eval_sample, problem  # noqa: E402


def sequential(model, lp, sample, ds, dev):
    clips, gt, extr = sample["images"][:, :5], sample["cam_poses_rel_cv2"][:, :5], sample["cam_extrinsics_cv2_canonicalized"]
    rows = []
    with torch.no_grad():
        for k in range(5):
            c, g, e = ev.permute_clips(clips, gt, extr, k)
            feats = model.encoder_3d.get_feat3D(c.reshape(5, *c.shape[2:]))
            feats = feats.reshape(1, 5, *feats.shape[1:])
            f = torch.cat([model.encoder_traj(feats, return_features=True), model.encoder_traj_2d(c, return_features=True)], dim=-1)
            p, _ = model.pose_head(f).split([model.encoder_traj.pose_dim, 1], dim=-1)
            p = torch.cat([F.normalize(p[:, :4]), p[:, 4:]], dim=1)
            rows.append(ev.evaluate(model, lp, sample, ds, p, feats, e, g, 0, k, dev))
    return rows


def batched(model, lp, sample, ds, dev):
    rd = ev.predict_initial(model, sample, dev)
    return ev.evaluate_all(model, lp, sample, ds, rd, 0, dev, None, return_table=True)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    ds = eval_dataset()
    sample = {k: v.to(dev) for k, v in eval_sample().items()}
    model = FORGE(eval_config(syn.kubric_config))
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    lp = fm.LPIPS(pretrained=False, seed=0).to(dev)
    for _ in range(2):
        seq = sequential(model, lp, sample, ds, dev)
        bat = batched(model, lp, sample, ds, dev)
    table = bat[-1].cpu()
    worst = max(abs(table[k, j].item() - seq[k][j]) / max(1.0, abs(seq[k][j])) for k in range(5) for j in range(6))
    print("one scene, five canonical choices: batched against sequential figures differ by at most %.2e (relative to max(1, |x|))" % worst)
    ts, tb = [], []
    for _ in range(args.reps):
        ts.append(clock(lambda: sequential(model, lp, sample, ds, dev))[0])
        tb.append(clock(lambda: batched(model, lp, sample, ds, dev))[0])
    med = lambda v: sorted(v)[len(v) // 2]
    print("five sequential passes (encoder, pose estimators, evaluate, read-out each): median %.2f ms (min %.2f, max %.2f) of %d"
          % (med(ts), min(ts), max(ts), len(ts)))
    print("predict_initial + evaluate_all:                                              median %.2f ms (min %.2f, max %.2f) of %d"
          % (med(tb), min(tb), max(tb), len(tb)))
    print("ratio of the medians: %.2f" % (med(ts) / med(tb)))
    pairs = [(i, j) for i in range(5) for j in range(i + 1, 5)]
    P3, c3 = problem(5, pairs, 0.02, 500)
    for B in (1, 64):
        P = P3.repeat((B + 2) // 3, 1, 1, 1)[:B].contiguous().to(dev)
        c = c3.repeat((B + 2) // 3, 1)[:B].contiguous().to(dev)
        for _ in range(20):
            ops.pose_sync(P, c, pairs, 5)
        n = 2000
        t, _ = clock(lambda: [ops.pose_sync(P, c, pairs, 5) for _ in range(n)][-1])
        print("ops.pose_sync N = 5, E = 10, squares = 10, B = %2d: %.1f us per call (%d eager calls back to back)" % (B, t / n * 1e3, n))


if __name__ == "__main__":
    main()
