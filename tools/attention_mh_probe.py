#!/usr/bin/env python
"""Cost of the opt-in multi-head HIP attention of the 2-D pose estimator (ops.attention_mh / ops.attention_mh_train = forge_attention_mh_fwd /
forge_attention_mh_bwd, switch ops.set_multihead_attention) against the path it replaces - head-split copies, bmm, scale, softmax, bmm, head-merge
copy on torch's ops - alternating in one process:

    python tools/attention_mh_probe.py [--repeats R] [--iters K] [--steps S] [--scenes 1,4] [--out profiles/attention_mh_probe.txt]
    ATT_MH_PROBE_ONLY=op python tools/attention_mh_probe.py --repeats 1 --iters 3       # one part alone (rocprofv3 --kernel-trace --stats pass)
    ATT_MH_PROBE_ONLY=resources python tools/attention_mh_probe.py                      # needs hipcc, no GPU

  op         one block's attention at b scenes x 5 views (q [b,1024,256]; cross: k / v [b,256,256], self: [b,1024,1024]; 4 heads, scale 1/8):
             forward under no_grad and forward + backward, median ms of R alternated windows of K iterations (HIP events around a window) with
             the spread of the windows, and the peak allocated memory of one call above the level before it.
  estimator  PoseEstimator2D inference at [1,5,3,256,256] (eval, no_grad), eager and as a hipGraph replay, switch off and on, alternated.
  joint      BASELINE configs[4] (FORGE, predicted poses: forward + backward + clip + Adam) with the switch off and on, alternated, S steps a window
             after one warm-up step in each setting, device-synchronised host clock.
  resources  VGPR / AGPR / scratch / occupancy of every kernel in forge_amd/csrc/attention.hip, from the compiler's kernel-resource-usage remarks.
A machine without a GPU fails on the first three parts: there is nothing to measure on it."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from forge_amd import ops  # noqa: E402

LINES = []
H, SCALE = 4, 0.125


def say(line):
    print(line, flush=True)
    LINES.append(line)


def heads(x):
    b, n, c = x.shape
    return x.reshape(b, n, H, c // H).permute(0, 2, 1, 3).reshape(b * H, n, -1)


def stock(q, k, v):
    """MultiHeadAttention.forward between its projections, as the module spells it."""
    b = q.shape[0]
    attn = (torch.bmm(heads(q), heads(k).transpose(1, 2)) * SCALE).softmax(dim=-1)
    o = torch.bmm(attn, heads(v))
    return o.reshape(b, H, o.shape[1], -1).permute(0, 2, 1, 3).reshape(b, o.shape[1], -1)


def spread(xs):
    return "median %.4f, min %.4f, max %.4f" % (statistics.median(xs), min(xs), max(xs))


def alternate(paths, repeats, iters, dev):
    """{name: [ms per call of each window]} with the paths alternating window by window, and {name: MB} peak memory of one call."""
    ms, peak = {n: [] for n in paths}, {}
    for name, fn in paths.items():
        for _ in range(3):
            fn()                                                         # warm-up: code objects, rocBLAS algorithm choice, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
    for _ in range(repeats):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / iters)
    return ms, peak


def operator(dev, scenes, kind, repeats, iters):
    Nq, Nk = 1024, (256 if kind == "cross" else 1024)
    g = torch.Generator(device=dev).manual_seed(1)
    q, k, v = (torch.randn(scenes, n, H * 64, device=dev, generator=g).requires_grad_(True) for n in (Nq, Nk, Nk))
    dout = torch.randn(scenes, Nq, H * 64, device=dev, generator=g)

    def nograd(fn):
        def call():
            with torch.no_grad():
                return fn()
        return call

    for what, paths in (("forward", {"torch": nograd(lambda: stock(q, k, v)), "hip": nograd(lambda: ops.attention_mh(q, k, v, H, SCALE))}),
                        ("forward + backward", {"torch": lambda: torch.autograd.grad(stock(q, k, v), (q, k, v), dout),
                                                "hip": lambda: torch.autograd.grad(ops.attention_mh_train(q, k, v, H, SCALE), (q, k, v), dout)})):
        ms, peak = alternate(paths, repeats, iters, dev)
        mt, mh = statistics.median(ms["torch"]), statistics.median(ms["hip"])
        say("op %-5s %d scene%s (%d,%d,%d,%d) %-18s: torch %.4f ms, HIP %.4f ms (ratio %.2f); peak memory above the inputs: torch %.1f MB, HIP %.1f MB"
            "   (%d windows x %d; torch %s; HIP %s)" % (kind, scenes, " " if scenes == 1 else "s", scenes, H, Nq, Nk, what, mt, mh, mh / mt, peak["torch"],
                                                        peak["hip"], repeats, iters, spread(ms["torch"]), spread(ms["hip"])))


def estimator(dev, repeats, iters):
    from forge_amd import synthetic as syn
    from forge_amd.graph import GraphedCall
    from forge_amd.pose_estimator_2d import PoseEstimator2D
    torch.manual_seed(0)
    mod = PoseEstimator2D()
    sd = syn.seeded_state_dict({"m." + k: v for k, v in mod.state_dict().items()}, 13)
    mod.load_state_dict({k[2:]: v for k, v in sd.items()})
    mod = mod.to(dev).eval()
    x = torch.rand(1, 5, 3, 256, 256, device=dev)

    def run(on):
        def call():
            prev = ops.set_multihead_attention(on)
            try:
                with torch.no_grad():
                    return mod(x, return_features=True)
            finally:
                ops.set_multihead_attention(prev)
        return call

    ms, _ = alternate({"off": run(False), "on": run(True)}, repeats, iters, dev)
    say("estimator PoseEstimator2D [1,5,3,256,256] inference, eager       : switch off %.3f ms, on %.3f ms (ratio %.3f)   (%d windows x %d; off %s; on %s)"
        % (statistics.median(ms["off"]), statistics.median(ms["on"]), statistics.median(ms["on"]) / statistics.median(ms["off"]), repeats, iters,
           spread(ms["off"]), spread(ms["on"])))
    graphs = {name: GraphedCall(run(on), dev, warmup=2) for name, on in (("off", False), ("on", True))}     # the switch is read at capture
    ms, _ = alternate(graphs, repeats, iters, dev)
    d = (graphs["on"]() - graphs["off"]()).abs().max().item()
    say("estimator PoseEstimator2D [1,5,3,256,256] inference, hipGraph replay: switch off %.3f ms, on %.3f ms (ratio %.3f)   (%d windows x %d; off %s; on %s); "
        "features on vs off: max abs diff %.2e" % (statistics.median(ms["off"]), statistics.median(ms["on"]),
                                                   statistics.median(ms["on"]) / statistics.median(ms["off"]), repeats, iters, spread(ms["off"]),
                                                   spread(ms["on"]), d))


def joint_step(dev, scenes, repeats, steps):
    from deterministic_probe import joint                                # tools/: the joint step as bench.py runs it
    step = joint(scenes, dev)
    ms, peak = {False: [], True: []}, {False: [], True: []}
    prev = ops.multihead_attention()
    try:
        for _ in range(repeats):                                         # alternate: off, on, off, ...
            for on in (False, True):
                ops.set_multihead_attention(on)
                step()                                                   # warm-up in this setting
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                ms[on].append((time.perf_counter() - t0) / steps * 1e3)
                peak[on].append(torch.cuda.max_memory_allocated(dev) / 1e6)
    finally:
        ops.set_multihead_attention(prev)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    say("joint step (configs[4]), %d scene%s: switch off %.2f ms, on %.2f ms (ratio %.3f); peak allocated off %.0f MB, on %.0f MB   (%d windows x %d steps; "
        "off %s; on %s)" % (scenes, "" if scenes == 1 else "s", off, on, on / off, max(peak[False]), max(peak[True]), repeats, steps,
                            spread(ms[False]), spread(ms[True])))


def resources():
    """The compiler's own account of every kernel in attention.hip, with the library's flags."""
    from forge_amd import build as fb
    src = os.path.join(ROOT, "forge_amd", "csrc", "attention.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [fb.hipcc()] + fb.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "attention.o")]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    field = lambda blk, key: re.search(re.escape(key) + r"\s*([0-9]+)", blk).group(1)
    say("resources (%s): kernel, VGPRs, AGPRs, scratch bytes/lane, LDS bytes, waves/SIMD" % " ".join(fb.FLAGS))
    for blk in text.split("Function Name: ")[1:]:
        mangled = blk.split()[0]
        name = subprocess.run(["c++filt", mangled], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip() or mangled
        name = re.sub(r"^(void )?forge::|\(.*$", "", name)
        say("  %-42s VGPRs %3s  AGPRs %3s  scratch %s  LDS %5s  waves/SIMD %s" % (name, field(blk, "VGPRs:"), field(blk, "AGPRs:"), field(blk, "ScratchSize [bytes/lane]:"),
                                                                                 field(blk, "LDS Size [bytes/block]:"), field(blk, "Occupancy [waves/SIMD]:")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--scenes", default="1,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    only = os.environ.get("ATT_MH_PROBE_ONLY")
    scenes = [int(x) for x in a.scenes.split(",") if x]
    if only != "resources":
        assert torch.cuda.is_available(), "attention_mh_probe measures on the MI355X"
        dev = torch.device("cuda:0")
        say("device: %s" % torch.cuda.get_device_name(0))
    if only in (None, "op"):
        for b in scenes:
            for kind in ("cross", "self"):
                operator(dev, b, kind, a.repeats, a.iters)
    if only in (None, "estimator"):
        estimator(dev, a.repeats, max(5, a.iters // 10))
    if only in (None, "joint"):
        for b in scenes:
            joint_step(dev, b, max(3, a.repeats // 2), a.steps)
            torch.cuda.empty_cache()
    if only in (None, "resources"):
        resources()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
