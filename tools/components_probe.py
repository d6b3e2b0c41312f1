#!/usr/bin/env python
"""Probe of the connected-component stage (forge_amd.geometry.label_components / keep_components, csrc/components.hip) on the MI355X.

    python tools/components_probe.py [--reps 30] [--out profiles/rNN_components_probe.txt]

Volumes: one 64^3, one 128^3 and eight 128^3, two fields each:
    blob+dust   synthetic.blob_volumes densities with seeded dust: every voxel becomes 1.0 with probability 0.002 -
                the object as one component of 10^4 - 10^6 voxels plus thousands of floaters, the case the stage exists for
    random0.2   a seeded random mask at p = 0.2 given quantised values by tests/components_cases.from_mask (level 33/128), the construction of the
                test suite's random fields at the probe's sizes: a few giant components and tens of thousands of small ones, every wave sees
                many roots - the worst case for the union passes and for the per-wave aggregation
Timed, per volume set and field, medians (min, max) after warm-up, host clock around a device synchronise; the repetitions differ per quantity
and every line says them:
    keep_components                        --reps calls; label (5 launches) + select (2 launches), no read-back
    label_components                       --reps calls; with max_components (no synchronisation) and without (one read-back of the counts)
    extract_mesh / with components         max(5, reps / 3) calls; plain extract_mesh against extract_mesh(components="largest"): the difference
                                           is the price a user pays
    device-to-host copy                    max(5, reps / 3) calls
    copy + scipy                           5 calls, 3 at eight 128^3 volumes
Compared against:
    HBM floor        the bytes the launches move by design (csrc/components.hip's header: 32 bytes per voxel for keep_components, 44 for
                     label_components) at the 8 TB/s HBM3E peak - a lower bound for orientation, not a roofline the design claims to approach:
                     at these sizes the launches are latency-bound
    the other route  the device-to-host copy of the density tensor (pageable destination, as `.cpu()` makes it) plus scipy.ndimage.label with the
                     15-point structure on one host core, where scipy is installed; the copy alone is the floor of that route otherwise
The cleaned volume is also checked against scipy's labels where scipy is there: voxels that differ, 0 expected. The compiled kernels' resource
numbers are printed when hipcc is found (tests/resource_remarks.py).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import components_cases as cc  # noqa: E402

from forge_amd import synthetic as syn  # noqa: E402
from forge_amd.geometry import extract_mesh, keep_components, label_components  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, HBM3E peak of the MI355X
KEEP_BYTES, LABEL_BYTES = 32, 44
QUANT_LEVEL = 33.0 / 128.0


def clock(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def blob_dust(n, D, seed):
    dens = syn.blob_volumes(n, D, C=4, seed=1)[1].numpy().copy()
    dust = np.random.default_rng(seed).random(dens.shape) < 0.002
    dens[dust] = 1.0
    return np.ascontiguousarray(dens, np.float32), 0.5


def random02(n, D, seed):
    return cc.from_mask(cc.random_mask((n, 1, D, D, D), 0.2, seed), seed), QUANT_LEVEL


def scipy_structure():
    S = np.zeros((3, 3, 3), int)
    for code in range(1, 8):
        dx, dy, dz = code & 1, (code >> 1) & 1, code >> 2
        S[1 + dz, 1 + dy, 1 + dx] = S[1 - dz, 1 - dy, 1 - dx] = 1
    S[1, 1, 1] = 1
    return S


def resources():
    try:
        from resource_remarks import kernel_remarks
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            rem = kernel_remarks(os.path.join(ROOT, "forge_amd", "csrc", "components.hip"), tmp)
    except Exception as e:                                      # a probe: the timing stands without the remarks
        return ["kernel resources: not available (%s)" % (repr(e)[:120],)]
    if not rem:
        return ["kernel resources: hipcc not found"]
    return ["%-60s %3d VGPRs, occupancy %d, LDS %5d bytes, scratch %d" % (k, v["VGPRs"], v["Occupancy"], v["LDS Size"], v["ScratchSize"])
            for k, v in sorted(rem.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_probe: needs the MI355X (a timing taken elsewhere says nothing)")
    try:
        import scipy
        import scipy.ndimage as ndi
        sp = scipy.__version__
    except ImportError:
        ndi, sp = None, None
    few = max(5, args.reps // 3)
    lines = ["components probe: %s, torch %s, scipy %s; median (min, max) ms, host clock around a synchronise; repetitions: %d for keep_components "
             "and label_components, %d for extract_mesh and the device-to-host copy, 5 for copy + scipy (3 at eight 128^3 volumes)"
             % (torch.cuda.get_device_name(0), torch.__version__, sp, args.reps, few)]
    for n, D in ((1, 64), (1, 128), (8, 128)):
        for name, make in (("blob+dust", blob_dust), ("random0.2", random02)):
            host, level = make(n, D, 5 + D + n)
            dens = torch.from_numpy(host).cuda()
            comp = label_components(dens, level)
            K = comp.counts.cpu().tolist()
            kmax = max(K)
            largest = [int(s.max()) if s.numel() else 0 for s in comp.sizes]
            vox = n * D ** 3
            keep = clock(lambda: keep_components(dens, level), args.reps)
            plain = clock(lambda: extract_mesh(dens, level=level), few)
            cleaned = clock(lambda: extract_mesh(dens, level=level, components="largest"), few)
            capped = clock(lambda: label_components(dens, level, max_components=kmax), args.reps)
            exact = clock(lambda: label_components(dens, level), args.reps)
            d2h = clock(lambda: dens.cpu(), few)
            floor_keep, floor_label = vox * KEEP_BYTES / HBM_PEAK * 1e3, vox * LABEL_BYTES / HBM_PEAK * 1e3
            line = ("n = %d, D = %3d, %-9s: K = %s, largest = %s | keep_components [%d reps] %.3f (%.3f, %.3f) | extract_mesh [%d reps] %.3f (%.3f, %.3f), with "
                    "components=\"largest\" %.3f (%.3f, %.3f) | label_components [%d reps] capacity %.3f (%.3f, %.3f), with read-back %.3f (%.3f, %.3f) | "
                    "%.1f MB by design = %.4f ms at 8 TB/s (%.1f %% reached by keep_components; label: %.4f ms, %.1f %%) | device-to-host copy "
                    "of the density (%.1f MB) [%d reps] %.3f (%.3f, %.3f)"
                    % (n, D, name, K if n == 1 else "%d..%d" % (min(K), max(K)), largest if n == 1 else "%d..%d" % (min(largest), max(largest)),
                       args.reps, *keep, few, *plain, *cleaned, args.reps, *capped, *exact, vox * KEEP_BYTES / 1e6, floor_keep, 100 * floor_keep / keep[0], floor_label,
                       100 * floor_label / capped[0], vox * 4 / 1e6, few, *d2h))
            if ndi is not None:
                S = scipy_structure()

                def route():
                    h = dens.cpu().numpy()
                    return [ndi.label(h[v, 0] > np.float32(level), structure=S) for v in range(n)]
                reps = 3 if vox > 1 << 21 else 5
                sc = clock(route, reps, warm=1)
                got = keep_components(dens, level).cpu().numpy()
                differ = 0
                for v, (lab, k) in enumerate(route()):
                    sizes = np.bincount(lab.ravel())[1:]
                    want = host[v, 0].copy()
                    if k:
                        cand = np.flatnonzero(sizes == sizes.max()) + 1
                        flat = lab.ravel()
                        best = int(flat[np.argmax(np.isin(flat, cand))])             # of the largest, the one that comes first in linear order
                        want[(lab > 0) & (lab != best)] = 0.0
                    differ += int((want.view(np.int32) != got[v, 0].view(np.int32)).sum())
                line += " | copy + scipy.ndimage.label on one core [%d reps] %.3f (%.3f, %.3f), x %.0f keep_components | %d voxels differ" % (
                    reps, *sc, sc[0] / keep[0], differ)
            lines.append(line)
            print(line, flush=True)
    lines += ["", "kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):"] + resources()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
