#!/usr/bin/env python
"""Cost of the differentiable HIP attention (ops.attention_train = forge_attention_fwd_lse + forge_attention_bwd) against the path it replaces,
torch's autograd of matmul - softmax - matmul, alternating in one process:

    python tools/attention_bwd_probe.py [--repeats R] [--iters K] [--steps S] [--scenes 1,4] [--out profiles/attention_bwd_probe.txt]
    ATT_PROBE_ONLY=op python tools/attention_bwd_probe.py --repeats 1 --iters 3          # the operator alone (rocprofv3 --kernel-trace --stats pass)

  operator   forward + backward at (4, 4096, 4096), with the value table shared by the batch (the cross attention: no dv) and with a per-batch v
             (the self attention): median ms of R alternated windows of K iterations (HIP events around a window), the achieved fp32 MFMA rate of
             the HIP pair from the FLOPs it executes (forge_amd/flopmeter.py), and the peak allocated memory of one forward + backward above the
             level before the call.
  joint step BASELINE configs[4] (FORGE, predicted poses: forward + backward + clip + Adam) with ops.set_attention_training off and on,
             alternated, S steps a window after one warm-up step in each setting, device-synchronised host clock.
A machine without a GPU fails here: there is nothing to measure on it."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from forge_amd import ops  # noqa: E402
from deterministic_probe import joint  # noqa: E402  (tools/: the joint step as bench.py runs it)

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def stock(q, k, v):
    return torch.matmul(torch.matmul(q, k.transpose(1, 2)).softmax(dim=-1), v)


def operator(dev, shared, repeats, iters):
    B, N = 4, 4096
    g = torch.Generator(device=dev).manual_seed(1)
    q, k = (torch.randn(B, N, 64, device=dev, generator=g).mul_(0.5).requires_grad_(True) for _ in range(2))
    v = torch.randn(1 if shared else B, N, 64, device=dev, generator=g).requires_grad_(not shared)
    dout = torch.randn(B, N, 64, device=dev, generator=g)
    leaves = (q, k) if shared else (q, k, v)
    paths = {"torch": lambda: torch.autograd.grad(stock(q, k, v), leaves, dout), "hip": lambda: torch.autograd.grad(ops.attention_train(q, k, v), leaves, dout)}
    ms, peak = {n: [] for n in paths}, {}
    for name, fn in paths.items():
        fn()                                                             # warm-up: code objects, rocBLAS algorithm choice, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
    for _ in range(repeats):                                             # alternate: torch, hip, torch, ...
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / iters)
    mt, mh = statistics.median(ms["torch"]), statistics.median(ms["hip"])
    flop = (4.0 + (14.0 if shared else 16.0)) * B * N * N * 64           # what the two entry points execute
    say("operator (4, 4096, 4096) %-12s forward + backward: torch autograd %.3f ms, HIP %.3f ms (ratio %.2f; %.1f TF fp32 MFMA executed); peak memory above the "
        "inputs: torch %.0f MB, HIP %.0f MB   (medians of %d x %d; torch %s, HIP %s)"
        % ("shared v" if shared else "per-batch v", mt, mh, mh / mt, flop / mh / 1e9, peak["torch"], peak["hip"], repeats, iters,
           ["%.3f" % x for x in ms["torch"]], ["%.3f" % x for x in ms["hip"]]))


def joint_step(dev, scenes, repeats, steps):
    step = joint(scenes, dev)
    ms = {False: [], True: []}
    try:
        for _ in range(repeats):                                         # alternate: off, on, off, ...
            for on in (False, True):
                ops.set_attention_training(on)
                step()                                                   # warm-up in this setting
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                ms[on].append((time.perf_counter() - t0) / steps * 1e3)
    finally:
        ops.set_attention_training(False)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    say("joint step (configs[4]), %d scene%s: switch off %.2f ms, on %.2f ms (ratio %.3f)   (medians of %d x %d steps; off %s, on %s)"
        % (scenes, "" if scenes == 1 else "s", off, on, on / off, repeats, steps, ["%.2f" % x for x in ms[False]], ["%.2f" % x for x in ms[True]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--scenes", default="1,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attention_bwd_probe measures on the MI355X"
    dev = torch.device("cuda:0")
    only = os.environ.get("ATT_PROBE_ONLY")
    say("device: %s" % torch.cuda.get_device_name(0))
    if only in (None, "op"):
        for shared in (True, False):
            operator(dev, shared, a.repeats, a.iters)
    if only in (None, "joint"):
        for b in (int(x) for x in a.scenes.split(",") if x):
            joint_step(dev, b, max(3, a.repeats // 2), a.steps)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
