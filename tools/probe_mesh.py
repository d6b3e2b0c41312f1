#!/usr/bin/env python
"""forge_amd.geometry.extract_mesh on the MI355X, timed, at the volumes the encoder produces: 64^3 and 128^3, n = 1 and 8, on
synthetic.blob_volumes densities (level 0.5).

Beside each time stands the time of the device-to-host copy of the SAME density tensor (pageable destination, as `.cpu()` makes it): without
extract_mesh the only route to geometry is to copy the volume to the host and run a CPU iso-surface library there, so that copy is the floor of the
other route before any of its work. Also printed: the bytes the five launches move by design (computed from shapes and the counts, below) and
the time those bytes take at the 8 TB/s HBM3E peak; the ratio says how far the extraction is from a bandwidth-bound run, and at these sizes the
volumes sit in the 256 MiB Infinity Cache and launch and read-back latencies dominate, so read it as an end-to-end figure, not a kernel's share.

Both modes are timed: the exact one (one read-back of the counts, exact allocation) and the capacity one (no synchronisation, padded tensors).
Everything is warmed up; host clock around a device synchronise; median of --reps calls.

    python tools/probe_mesh.py [--reps 50] [--out profiles/r18_mesh_probe.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from forge_amd import synthetic as syn  # noqa: E402
from forge_amd.geometry import extract_mesh  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, HBM3E peak of the MI355X


def clock(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def design_bytes(n, D, nv, nf):
    """Bytes the launches read and write by design: classify reads the density once and writes a 4-byte record per cell; apply reads the record;
    vertex emission reads record + offset (8 bytes), face emission the record (4); then the outputs (24 bytes per vertex, 12 per triangle).
    The neighbourhood reads of the active cells (a surface, O(D^2)) are left out."""
    cells = (D + 1) ** 3
    return n * (4 * D ** 3 + cells * (4 + 4 + 8 + 4)) + 24 * nv + 12 * nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = ["extract_mesh(level=0.5) on synthetic.blob_volumes densities; median (min, max) of %d calls, host clock around a synchronise" % args.reps]
    for D in (64, 128):
        for n in (1, 8):
            dens = syn.blob_volumes(n, D, C=4, seed=1)[1].cuda()
            meshes = extract_mesh(dens)
            nv, nf = sum(m.vertices.shape[0] for m in meshes), sum(m.faces.shape[0] for m in meshes)
            mv, mf = max(m.vertices.shape[0] for m in meshes), max(m.faces.shape[0] for m in meshes)
            for _ in range(5):
                extract_mesh(dens)
                extract_mesh(dens, max_vertices=mv, max_faces=mf)
                dens.cpu()
            exact = clock(lambda: extract_mesh(dens), args.reps)
            capped = clock(lambda: extract_mesh(dens, max_vertices=mv, max_faces=mf), args.reps)
            d2h = clock(lambda: dens.cpu(), args.reps)
            b = design_bytes(n, D, nv, nf)
            lines.append("D = %3d, n = %d: %8d vertices, %8d triangles | exact %.3f ms (%.3f, %.3f) | capacity mode %.3f ms (%.3f, %.3f) | "
                         "device-to-host copy of the density (%.1f MB) %.3f ms (%.3f, %.3f) | %.1f MB by design = %.4f ms at the 8 TB/s HBM peak, "
                         "%.1f %% of it reached (capacity mode)"
                         % (D, n, nv, nf, *exact, *capped, dens.numel() * 4 / 1e6, *d2h, b / 1e6, b / HBM_PEAK * 1e3, 100 * (b / HBM_PEAK * 1e3) / capped[0]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
