#!/usr/bin/env python
"""Cost of the opt-in HIP token-row layers of both pose estimators (ops.token_linear / ops.layer_norm and their autograd forms =
forge_token_linear_fwd / _bwd, forge_layer_norm_fwd / _bwd, switch ops.set_token_layers) against the torch statements they replace - F.layer_norm,
F.linear, F.gelu, add - alternating in one process:

    python tools/token_layers_probe.py [--repeats R] [--iters K] [--steps S] [--scenes 1,4] [--out profiles/token_layers_probe.txt]
    TOKEN_PROBE_ONLY=op python tools/token_layers_probe.py --repeats 1 --iters 3        # one part alone
    TOKEN_PROBE_ONLY=resources python tools/token_layers_probe.py                       # needs hipcc, no GPU
    TOKEN_PROBE_ALL_SITES=1 ...                                                         # also the call sites ops.TOKEN_SITES_ON_TORCH leaves on torch

  op         every fused call site at b scenes' rows (2-D estimator: 1024 b x 256 channels; 3-D: 16384 b x 64): forward under no_grad and
             forward + backward, median ms of R alternated windows of K iterations (HIP events around a window) with the spread of the windows.
  estimator  PoseEstimator2D [1,5,3,256,256] and PoseEstimator3D [1,5,128,32,32,32] inference (eval, no_grad), eager and as a hipGraph replay,
             switch off and on, alternated; the multi-head attention switch is on in both arms.
  joint      BASELINE configs[4] (FORGE, predicted poses: forward + backward + clip + Adam) with the switch off and on, alternated, S steps a window
             after one warm-up step in each setting, device-synchronised host clock; the two attention switches on in both arms.
  resources  VGPR / AGPR / scratch / LDS / occupancy of every kernel in forge_amd/csrc/token.hip, from the compiler's kernel-resource-usage remarks.
  hashes     sha256 over the switch-OFF results this tree computes: the CASES of tests/test_gpu_attention_bwd.py and tests/test_gpu_attention_mh.py
             (outputs and gradients) and both estimators' training-mode features and parameter gradients. Run in the parent commit's tree and in this
             one on the same machine, the lines must agree. (Uses nothing the parent commit lacks.)
A machine without a GPU fails on every part but `resources`: there is nothing to measure on it."""
import argparse
import hashlib
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
import torch.nn.functional as F  # noqa: E402

from forge_amd import ops  # noqa: E402

LINES = []
EPS = 1e-5


def say(line):
    print(line, flush=True)
    LINES.append(line)


def spread(xs):
    return "median %.4f, min %.4f, max %.4f" % (statistics.median(xs), min(xs), max(xs))


def verdict(ms_torch, ms_hip):
    return "HIP wins every window" if max(ms_hip) <= min(ms_torch) else "torch wins every window" if max(ms_torch) <= min(ms_hip) else "windows overlap"


def alternate(paths, repeats, iters):
    """{name: [ms per call of each window]} with the paths alternating window by window."""
    ms = {n: [] for n in paths}
    for fn in paths.values():
        for _ in range(3):
            fn()                                                         # warm-up: code objects, rocBLAS algorithm choice, allocator
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / iters)
    return ms


#        site,      K,    N,    LayerNorm, GELU, residual
SITES_2D = [("2d.proj   LN + Linear", 256, 256, True, False, False), ("2d.o_proj Linear + residual", 256, 256, False, False, True),
            ("2d.fc1    LN + Linear + GELU", 256, 1024, True, True, False), ("2d.fc2    Linear", 1024, 256, False, False, False),
            ("2d.norm   LayerNorm alone", 256, 0, True, False, False)]
SITES_3D = [("3d.qk     LN + Linear", 64, 64, True, False, False), ("3d.v      Linear", 64, 64, False, False, False),
            ("3d.fc1    LN + Linear + GELU", 64, 128, True, True, False), ("3d.fc2    Linear + residual", 128, 64, False, False, True)]


def operator(dev, R, site, repeats, iters):
    name, K, N, ln, gelu, res = site
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    x = (3.0 + rnd(R, K)).requires_grad_(True)
    gamma, beta = (1.0 + 0.1 * rnd(K)).requires_grad_(True), (0.1 * rnd(K)).requires_grad_(True)
    if N == 0:                                                           # the stand-alone LayerNorm
        dy, wrt = rnd(R, K), (x, gamma, beta)
        stock = lambda: F.layer_norm(x, (K,), gamma, beta, EPS)
        hip, hip_train = (lambda: ops.layer_norm(x, gamma, beta, EPS)), (lambda: ops.layer_norm_train(x, gamma, beta, EPS))
    else:
        w, b = (rnd(N, K) / K ** 0.5).requires_grad_(True), (0.1 * rnd(N)).requires_grad_(True)
        r = rnd(R, N).requires_grad_(True) if res else None
        dy = rnd(R, N)
        wrt = (x, w, b) + ((gamma, beta) if ln else ()) + ((r,) if res else ())
        lnarg, act = ((gamma, beta, EPS) if ln else None), ("gelu" if gelu else None)

        def stock():
            y = F.linear(F.layer_norm(x, (K,), gamma, beta, EPS) if ln else x, w, b)
            y = F.gelu(y) if gelu else y
            return r + y if res else y
        hip = lambda: ops.token_linear(x, w, b, ln=lnarg, act=act, residual=r)
        hip_train = lambda: ops.token_linear_train(x, w, b, ln=lnarg, act=act, residual=r)

    def nograd(fn):
        def call():
            with torch.no_grad():
                return fn()
        return call

    for what, paths in (("forward", {"torch": nograd(stock), "hip": nograd(hip)}),
                        ("forward + backward", {"torch": lambda: torch.autograd.grad(stock(), wrt, dy), "hip": lambda: torch.autograd.grad(hip_train(), wrt, dy)})):
        ms = alternate(paths, repeats, iters)
        mt, mh = statistics.median(ms["torch"]), statistics.median(ms["hip"])
        say("op %-30s %6d x %4d -> %4d %-18s: torch %.4f ms, HIP %.4f ms (ratio %.2f; %s)   (%d windows x %d; torch %s; HIP %s)"
            % (name, R, K, N or K, what, mt, mh, mh / mt, verdict(ms["torch"], ms["hip"]), repeats, iters, spread(ms["torch"]), spread(ms["hip"])))


def seeded(mod, seed):
    from forge_amd import synthetic as syn
    sd = syn.seeded_state_dict({"m." + k: v for k, v in mod.state_dict().items()}, seed)
    mod.load_state_dict({k[2:]: v for k, v in sd.items()})
    return mod


def estimators(dev):
    from forge_amd import synthetic as syn
    from forge_amd.pose_estimator_2d import PoseEstimator2D
    from forge_amd.pose_estimator_3d import PoseEstimator3D
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(3)
    return (("PoseEstimator2D [1,5,3,256,256]", seeded(PoseEstimator2D(), 13).to(dev), torch.rand(1, 5, 3, 256, 256, generator=g).to(dev)),
            ("PoseEstimator3D [1,5,128,32,32,32]", seeded(PoseEstimator3D(syn.kubric_config()), 13).to(dev),
             (0.5 * torch.randn(1, 5, 128, 32, 32, 32, generator=g)).to(dev)))


def estimator(dev, repeats, iters):
    from forge_amd.graph import GraphedCall
    prev_mh = ops.set_multihead_attention(True)
    try:
        for name, mod, x in estimators(dev):
            mod.eval()

            def run(on):
                def call():
                    prev = ops.set_token_layers(on)
                    try:
                        with torch.no_grad():
                            return mod(x, return_features=True)
                    finally:
                        ops.set_token_layers(prev)
                return call

            ms = alternate({"off": run(False), "on": run(True)}, repeats, iters)
            say("estimator %s inference, eager          : switch off %.3f ms, on %.3f ms (ratio %.3f; %s)   (%d windows x %d; off %s; on %s)"
                % (name, statistics.median(ms["off"]), statistics.median(ms["on"]), statistics.median(ms["on"]) / statistics.median(ms["off"]),
                   verdict(ms["off"], ms["on"]), repeats, iters, spread(ms["off"]), spread(ms["on"])))
            graphs = {n: GraphedCall(run(on), dev, warmup=2) for n, on in (("off", False), ("on", True))}     # the switch is read at capture
            ms = alternate(graphs, repeats, iters)
            off, on = graphs["off"](), graphs["on"]()
            say("estimator %s inference, hipGraph replay: switch off %.3f ms, on %.3f ms (ratio %.3f; %s)   (%d windows x %d; off %s; on %s); "
                "features on vs off: max abs diff %.2e of max %.2e"
                % (name, statistics.median(ms["off"]), statistics.median(ms["on"]), statistics.median(ms["on"]) / statistics.median(ms["off"]),
                   verdict(ms["off"], ms["on"]), repeats, iters, spread(ms["off"]), spread(ms["on"]), (on - off).abs().max().item(), off.abs().max().item()))
            del graphs
    finally:
        ops.set_multihead_attention(prev_mh)


def joint_step(dev, scenes, repeats, steps):
    from deterministic_probe import joint                                # tools/: the joint step as bench.py runs it
    step = joint(scenes, dev)
    ms = {False: [], True: []}
    prev = ops.set_multihead_attention(True), ops.set_attention_training(True), ops.token_layers()
    try:
        for _ in range(repeats):                                         # alternate: off, on, off, ...
            for on in (False, True):
                ops.set_token_layers(on)
                step()                                                   # warm-up in this setting
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                ms[on].append((time.perf_counter() - t0) / steps * 1e3)
    finally:
        ops.set_multihead_attention(prev[0]), ops.set_attention_training(prev[1]), ops.set_token_layers(prev[2])
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    say("joint step (configs[4]), %d scene%s: switch off %.2f ms, on %.2f ms (ratio %.3f; %s)   (%d windows x %d steps; off %s; on %s)"
        % (scenes, "" if scenes == 1 else "s", off, on, on / off, verdict(ms[False], ms[True]), repeats, steps, spread(ms[False]), spread(ms[True])))


def resources():
    """The compiler's own account of every kernel in token.hip, with the library's flags."""
    from forge_amd import build as fb
    src = os.path.join(ROOT, "forge_amd", "csrc", "token.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [fb.hipcc()] + fb.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "token.o")]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    field = lambda blk, key: re.search(re.escape(key) + r"\s*([0-9]+)", blk).group(1)
    say("resources (%s): kernel, VGPRs, AGPRs, scratch bytes/lane, LDS bytes, waves/SIMD" % " ".join(fb.FLAGS))
    for blk in text.split("Function Name: ")[1:]:
        mangled = blk.split()[0]
        name = subprocess.run(["c++filt", mangled], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip() or mangled
        name = re.sub(r"^(void )?forge::|\(.*$", "", name)
        say("  %-42s VGPRs %3s  AGPRs %3s  scratch %s  LDS %5s  waves/SIMD %s" % (name, field(blk, "VGPRs:"), field(blk, "AGPRs:"), field(blk, "ScratchSize [bytes/lane]:"),
                                                                                 field(blk, "LDS Size [bytes/block]:"), field(blk, "Occupancy [waves/SIMD]:")))


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def hashes(dev):
    """Everything here runs with the switches off and uses only what the parent commit has as well."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_attention_bwd as tb
    import test_gpu_attention_mh as tm
    say("hashes (switch off): sha256 over outputs and gradients, this tree's Python and library")
    for case, cid in zip(tb.CASES, tb.IDS):
        ins = tb.inputs(dev, case)
        q, k, v, dout = ins[:4]
        with torch.no_grad():
            out = ops.attention(q, k, v)
        ls = [t.clone().requires_grad_(True) for t in (q, k)] + [v.clone().requires_grad_(v.shape[0] == q.shape[0])]
        o2 = ops.attention_train(*ls)
        grads = torch.autograd.grad(o2, [t for t in ls if t.requires_grad], dout)
        say("  attention     %-28s %s" % (cid, digest((out, o2) + tuple(grads))))
    for case, cid in zip(tm.CASES, tm.IDS):
        B, Hh, Nq, Nk, scale, sliced = case
        q, k, v, dout = tm.inputs(dev, case)
        ls = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = ops.attention_mh_train(*ls, Hh, scale)
        say("  attention_mh  %-28s %s" % (cid, digest((out,) + tuple(torch.autograd.grad(out, ls, dout)))))
    import forge_amd
    forge_amd.set_deterministic(True)                                    # the project's own weight gradients in their fixed-order form ...
    torch.use_deterministic_algorithms(True, warn_only=True)             # ... and torch's
    for name, mod, x in estimators(dev):
        mod.train()
        for m in mod.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
        feats = mod(x, return_features=True)
        w = torch.linspace(-1.0, 1.0, feats.numel(), device=dev).reshape(feats.shape)
        params = [p for p in mod.parameters() if p.requires_grad]
        grads = torch.autograd.grad((feats * w).sum(), params, allow_unused=True)
        torch.cuda.synchronize()
        again = mod(x, return_features=True)
        grads2 = torch.autograd.grad((again * w).sum(), params, allow_unused=True)
        stable = torch.equal(feats, again) and all(a is None or torch.equal(a, b) for a, b in zip(grads, grads2))
        say("  %-36s features %s" % (name, digest((feats,))))
        say("  %-36s gradients %s%s" % (name, digest([g for g in grads if g is not None]), "" if stable else "   (not bitwise stable run to run in this tree: torch's "
                                                                                                         "own atomics - compare the features)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--scenes", default="1,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    only = os.environ.get("TOKEN_PROBE_ONLY")
    if os.environ.get("TOKEN_PROBE_ALL_SITES") == "1":
        ops.TOKEN_SITES_ON_TORCH = frozenset()
        say("every call site on the kernels (TOKEN_PROBE_ALL_SITES=1: ops.TOKEN_SITES_ON_TORCH emptied)")
    elif hasattr(ops, "TOKEN_SITES_ON_TORCH"):
        say("call sites left on torch with the switch on: %s" % (", ".join(sorted(ops.TOKEN_SITES_ON_TORCH)) or "none"))
    scenes = [int(x) for x in a.scenes.split(",") if x]
    if only != "resources":
        assert torch.cuda.is_available(), "token_layers_probe measures on the MI355X"
        dev = torch.device("cuda:0")
        say("device: %s" % torch.cuda.get_device_name(0))
    if only in (None, "op"):
        for b in scenes:
            for site in SITES_2D:
                operator(dev, 1024 * b, site, a.repeats, a.iters)
            for site in SITES_3D:
                operator(dev, 16384 * b, site, a.repeats, a.iters)
    if only in (None, "estimator"):
        estimator(dev, a.repeats, max(5, a.iters // 10))
    if only in (None, "joint"):
        for b in scenes:
            joint_step(dev, b, max(3, a.repeats // 2), a.steps)
            torch.cuda.empty_cache()
    if only in (None, "resources"):
        resources()
    if only == "hashes":
        hashes(dev)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
