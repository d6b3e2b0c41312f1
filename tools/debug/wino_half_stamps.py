"""Per-workgroup clock stamps of the four-point Winograd GEMM (forge_wino_gemm_half) on the ConvGRU gates and state launches of the one-scene step.

    FORGE_AMD_LIB=tools/debug/libforge_hip_timing.so python tools/debug/wino_half_stamps.py      (tools/debug/build_timing_lib.sh)

From the stamps entry / first barrier / loop end / exit (wall_clock64, 100 MHz) of every workgroup: how many are resident at once, the median
phases, and how tightly a round's workgroups start and end together. Without the stamp symbol in the library (a product build) it only runs
the launches (5 each) - the form a counter pass wants: rocprofv3 --pmc ... -- python tools/debug/wino_half_stamps.py."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from forge_amd import _lib, convops as co  # noqa: E402

dev = torch.device("cuda:0")
L = _lib.lib()
stamped = hasattr(L, "forge_debug_conv_stamps")
if stamped:
    L.forge_debug_conv_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
TICK = 0.01                                                      # us per wall_clock64 tick

for name, (n, D, Ht, Wt, C1, C2, Cout) in (("gates 16 x [8192 x 768] x [768 x 256]", (1, 32, 16, 16, 128, 128, 256)),
                                           ("state 16 x [8192 x 768] x [768 x 128]", (1, 32, 16, 16, 128, 128, 128))):
    g = torch.Generator(device=dev).manual_seed(1)
    R = n * D * Ht * Wt
    V1 = torch.randn(16, R, C1, device=dev, generator=g)
    V2 = torch.randn(16, R, C2, device=dev, generator=g)
    U = torch.randn(16, 3, Cout, C1 + C2, device=dev, generator=g) * 0.03
    Mm8 = torch.empty(8, R, Cout, device=dev)
    f = lambda: co.wino_gemm(V1, C1, V2, C2, U, Mm8, n, D, Ht, Wt, Cout, half=True)  # noqa: E731
    for _ in range(4):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record(); torch.cuda.synchronize()  # noqa: E702
    nwg = (R // 64) * (Cout // 128) * 4
    line = "%s: %d workgroups, event %.1f us" % (name, nwg, a.elapsed_time(b) * 1e3)
    if not stamped:
        print(line, flush=True)
        continue
    s = np.zeros((nwg, 4), dtype=np.int64)
    L.forge_debug_conv_stamps(s.ctypes.data_as(ctypes.c_void_p), nwg)
    s = (s - s[:, 0].min()) * TICK
    ev = sorted([(t, 1) for t in s[:, 0]] + [(t, -1) for t in s[:, 3]], key=lambda e: (e[0], e[1]))
    live = peak = 0
    for _, d in ev:
        live += d
        peak = max(peak, live)
    order = np.argsort(s[:, 0], kind="stable")
    med = [float(np.median(s[:, i + 1] - s[:, i])) for i in range(3)]
    q = lambda v, p: float(np.percentile(v, p))  # noqa: E731
    print(line + " | first entry .. last exit %.1f us, resident at once (peak) %d" % (s[:, 3].max(), peak))
    print("    per workgroup, median: entry -> first barrier %.2f, K loops %.1f, loop end -> exit %.2f us; whole workgroup p5 / p50 / p95 %.1f / %.1f / %.1f us"
          % (med[0], med[1], med[2], q(s[:, 3] - s[:, 0], 5), q(s[:, 3] - s[:, 0], 50), q(s[:, 3] - s[:, 0], 95)))
    for r in range((nwg + peak - 1) // max(peak, 1)):
        w = order[r * peak:(r + 1) * peak]
        print("    round %d (%d workgroups in entry order): entries p5 .. p95 %.1f .. %.1f us, loop ends %.1f .. %.1f, exits %.1f .. %.1f"
              % (r, len(w), q(s[w, 0], 5), q(s[w, 0], 95), q(s[w, 2], 5), q(s[w, 2], 95), q(s[w, 3], 5), q(s[w, 3], 95)), flush=True)
