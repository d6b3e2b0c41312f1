#!/usr/bin/env python
"""Probe of the weight-gradient kernels of csrc/conv_wgrad.hip through the C entry points of the library of THIS checkout.

    python tools/wgrad_forms_probe.py hash     SHA-256 of forge_conv_wgrad_det (accumulate 0 over a NaN-filled dW, accumulate 1 onto the seeded
                                               prior) for every C-entry case of tests/conv_wgrad_cases.py, and of forge_wino_wgrad_det at the three
                                               Cin tile widths (32 / 64 / 128, and two inputs). The deterministic twins are bitwise reproducible, so
                                               two checkouts compute the same results exactly when every line is equal.
    python tools/wgrad_forms_probe.py time     one launch per kernel / twin pair, atomic and deterministic: microseconds per launch (device events,
                                               warmed up, best of 3 windows of 30 launches), one JSON line per launch.
The timed shapes are the 4-scene training step's (profiles/r05_train_step_by_shape_b4.txt): the Winograd weight gradient of the ConvGRU gates
(128-wide tile), conv1 (<64, 2>), the heads' up-convolution (<32, 4>), the heads' 32 -> 16 (16x16 line kernel, 8 waves), conv_rgb's stride-2 form
and its 16 -> 8 layer, the ResNet shapes of tools/wgrad_probe.py for the plain tiles; the small and the 32x32 line kernel, which the step does not
launch, run their shape of tests/test_gpu_deterministic.py with n raised until a launch takes 100 us."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import conv_wgrad_cases as wc  # noqa: E402
from forge_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")
P = _lib.ptr


def taps_array(taps):
    return (ctypes.c_int * (3 * len(taps)))(*[v for t in taps for v in t])


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def operand(x, ld, views):
    buf, start, bs = wc.poisoned(x, ld, views)
    return buf.to(dev)[start:], bs


def hash_mode():
    L = _lib.lib()
    for c in wc.CASES:
        if c.launcher:
            continue
        d = wc.make_data(c)
        dy, _ = operand(d["dy"].reshape(1, wc.M_of(c), c.Cout), c.ldy, None)
        x1, bs1 = operand(d["x1"].reshape(c.n, -1, c.C1), c.ld1, c.views1)
        x2, bs2 = operand(d["x2"].reshape(c.n, -1, c.C2), c.ld2, c.views2) if c.C2 else (None, 0)
        ta = taps_array(c.taps)
        nb = L.forge_conv_wgrad_det_ws_bytes(c.C1, c.C2, c.n, c.D, c.H, c.W, c.istride, *c.in_grid, c.Cout, ta, len(c.taps))
        ws = torch.full((nb // 4,), float("nan"), device=dev)
        for acc in (0, 1):
            out = d["prior"].to(dev).clone() if acc else torch.full((len(c.taps), c.Cout, c.C1 + c.C2), float("nan"), device=dev)
            _lib.check(L.forge_conv_wgrad_det(P(dy), c.ldy, P(x1), c.C1, c.ld1, bs1, P(x2), c.C2, c.ld2, bs2, P(out), c.n, c.D, c.H, c.W, c.istride,
                                              *c.in_grid, c.Cout, ta, len(c.taps), acc, P(ws), nb, _lib.current_stream()), "forge_conv_wgrad_det")
            print("HASH conv %-10s accumulate %d  %s nan=%d" % (c.name, acc, sha(out), int(torch.isnan(out).sum())), flush=True)
    n, D, Ht, Wt, Cout, kd = 2, 4, 8, 8, 64, 3
    R = n * D * Ht * Wt
    for C1, C2 in ((32, 0), (64, 0), (128, 0), (128, 128)):
        g = torch.Generator().manual_seed(C1 + C2)
        dM = torch.randn(16, R, Cout, generator=g).to(dev)
        V1 = torch.randn(16, R, C1, generator=g).to(dev)
        V2 = torch.randn(16, R, C2, generator=g).to(dev) if C2 else None
        prior = torch.randn(16, kd, Cout, C1 + C2, generator=g)
        nb = L.forge_wino_wgrad_det_ws_bytes(C1, C2, n, D, Ht, Wt, Cout, kd)
        ws = torch.full((nb // 4,), float("nan"), device=dev)
        for acc in (0, 1):
            out = prior.to(dev).clone() if acc else torch.full(prior.shape, float("nan"), device=dev)
            _lib.check(L.forge_wino_wgrad_det(P(dM), P(V1), C1, 0, 0, P(V2), C2, 0, 0, P(out), n, D, Ht, Wt, Cout, kd, acc, P(ws), nb,
                                              _lib.current_stream()), "forge_wino_wgrad_det")
            print("HASH wino C1 %d C2 %d accumulate %d  %s nan=%d" % (C1, C2, acc, sha(out), int(torch.isnan(out).sum())), flush=True)


T27, T9, T1 = wc.T27, wc.T9, wc.T1
# name: (n, D, H, W, Cout, C1, stride of the gathered operand, taps, expected plan (family, p1, p2, waves), raise n until 100 us)
TIMED = [
    ("conv1 <64,2>", (20, 32, 32, 32, 128, 64, 1, T27, (1, 64, 2, 4), False)),
    ("heads up-conv <32,4>", (4, 32, 32, 32, 128, 32, 2, wc.T64, (1, 32, 4, 4), False)),
    ("heads 32->16 lines16<32,1,4,8>", (4, 64, 64, 64, 16, 32, 1, T27, (4, 32, 1, 8), False)),
    ("conv_rgb s2 lines16<16,2,9,4>", (20, 1, 64, 64, 16, 16, 2, wc.T36, (4, 16, 2, 4), False)),
    ("conv_rgb 16->8 lines16<16,1,7,4>", (20, 1, 128, 128, 8, 16, 1, wc.T25, (4, 16, 1, 4), False)),
    ("resnet l3 3x3 256->256 <128,1>", (20, 1, 32, 32, 256, 256, 1, T9, (1, 128, 1, 4), False)),
    ("resnet l1 3x3 64->64 <64,1>", (20, 1, 64, 64, 64, 64, 1, T9, (1, 64, 1, 4), False)),
    ("resnet-like 3x3 32->64 <32,1>", (1, 1, 511, 256, 64, 32, 1, T9, (1, 32, 1, 4), False)),
    ("small", (2, 6, 10, 20, 8, 8, 1, wc.T5_FAR, (2, 32, 4, 4), True)),
    ("lines 32x32", (1, 8, 16, 40, 32, 32, 1, T27, (3, 32, 1, 4), True)),
]


def timed(f):
    for _ in range(5):
        f()
    best = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(30):
            f()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / 30
        best = us if best is None or us < best else best
    return best


def conv_launchers(n, D, H, W, Cout, C1, ist, taps, want):
    L = _lib.lib()
    grid = ((D * ist if D > 1 else 1), H * ist, W * ist)
    ta = taps_array(taps)
    plan = (ctypes.c_longlong * 8)()
    assert L.forge_conv_wgrad_plan(C1, 0, n, D, H, W, ist, *grid, Cout, ta, len(taps), 0, plan) == 0 and tuple(plan[:4]) == want, (tuple(plan), want)
    g = torch.Generator().manual_seed(n)
    dy = torch.randn(n * D * H * W, Cout, generator=g).to(dev)
    x = torch.randn(n * grid[0] * grid[1] * grid[2], C1, generator=g).to(dev)
    out = torch.zeros(len(taps), Cout, C1, device=dev)
    nb = L.forge_conv_wgrad_det_ws_bytes(C1, 0, n, D, H, W, ist, *grid, Cout, ta, len(taps))
    ws = torch.empty(nb // 4, device=dev)
    head = (P(dy), Cout, P(x), C1, C1, 0, None, 0, 0, 0, P(out), n, D, H, W, ist, *grid, Cout, ta, len(taps))
    st = _lib.current_stream()
    keep = (dy, x, out, ws, ta)
    return (lambda: L.forge_conv_wgrad(*head, st), lambda: L.forge_conv_wgrad_det(*head, 1, P(ws), nb, st), keep)


def time_mode():
    L = _lib.lib()
    rows = []
    # the Winograd weight gradient of the ConvGRU gates: 4 scenes, 32^3 voxels as 16 x 16 tiles per plane, 128 + 128 -> 256 channels
    n, D, Ht, Wt, Cout, C1, C2, kd = 4, 32, 16, 16, 256, 128, 128, 3
    R = n * D * Ht * Wt
    dM, V1, V2 = (torch.randn(16, R, c, device=dev) for c in (Cout, C1, C2))
    out = torch.zeros(16, kd, Cout, C1 + C2, device=dev)
    nb = L.forge_wino_wgrad_det_ws_bytes(C1, C2, n, D, Ht, Wt, Cout, kd)
    ws = torch.empty(nb // 4, device=dev)
    head = (P(dM), P(V1), C1, 0, 0, P(V2), C2, 0, 0, P(out), n, D, Ht, Wt, Cout, kd)
    st = _lib.current_stream()
    rows.append(("wino gates <128,1>", lambda: L.forge_wino_wgrad(*head, st), lambda: L.forge_wino_wgrad_det(*head, 1, P(ws), nb, st)))
    for name, fa, fd in rows:
        for what, f in (("atomic", fa), ("det", fd)):
            assert f() == 0
            print(json.dumps({"launch": name, "path": what, "us": round(timed(f), 2)}), flush=True)
    del dM, V1, V2, out, ws
    for name, (n, D, H, W, Cout, C1, ist, taps, want, grow) in TIMED:
        while True:
            fa, fd, keep = conv_launchers(n, D, H, W, Cout, C1, ist, taps, want)
            assert fa() == 0 and fd() == 0
            ua = timed(fa)
            if not grow or ua >= 100.0 or n >= 4096:
                break
            n *= 2
        print(json.dumps({"launch": name, "n": n, "path": "atomic", "us": round(ua, 2)}), flush=True)
        print(json.dumps({"launch": name, "n": n, "path": "det", "us": round(timed(fd), 2)}), flush=True)
        del fa, fd, keep


if __name__ == "__main__":
    {"hash": hash_mode, "time": time_mode}[sys.argv[1]]()
