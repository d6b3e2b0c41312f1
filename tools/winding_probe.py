#!/usr/bin/env python
"""forge_amd.ops.winding_number and what stands on it (geometry.voxelize, geometry.volume_iou) on the MI355X, timed, beside the kernel's own VALU
floor and beside the same formula written in torch - the only other route to a winding number on the device.

  1. one call of winding_number: 1e5 queries (the unit cube) against one 64^3 and one 128^3 extraction (synthetic.blob_volumes densities, level
     0.5) and against 8 pairs of 64^3 extractions, beside the VALU floor: (query, face) pairs x VALU_PER_PAIR / 39.3e12 lane-instructions/s (the
     157.3 TF fp32 vector peak / 4, as tools/tridist_probe.py counts it). VALU_PER_PAIR = 465 / 8: the vector instructions of the compiled inner
     loop of winding_kernel (hipcc -O3 --offload-arch=gfx950, one group of 8 faces per iteration: 75 v_fmac, 70 v_pk_fma, 39 v_pk_add,
     30 v_pk_mul, 60 v_mul, 18 v_sub, 8 v_add, 9 v_fma, 24 v_sqrt, 8 v_rcp, 24 v_cmp, 24 v_cndmask, 8 v_max, 8 v_min, 8 v_bfi, 50 moves, and
     v_cvt_f64_f32 + v_add_f64 for the group). The 32 v_sqrt / v_rcp among them issue at half the rate of the others; the floor with them
     counted twice ((465 + 32) / 8) is printed beside it, and so is the plain count at the 32 lanes per clock a wave64 instruction issues at.
  2. voxelize at 64^3 and 128^3 (every lattice point against the extraction of that volume), and volume_iou at n = 1e5 for one and for 8 pairs.
  3. the torch composition: Van Oosterom and Strackee's formula with torch.atan2, queries in chunks of 2^22 / faces rows so that each temporary
     stays at 2^22 pairs. It is run on the first TORCH_QUERIES queries of each size (its time is proportional to the queries: every chunk does
     the same work) and compared as a RATE, pairs per second.

Everything is warmed up; host clock around a device synchronise; median (min, max) of --reps calls.

    python tools/winding_probe.py [--reps 5] [--out profiles/r31_winding_probe.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from forge_amd import ops, synthetic as syn  # noqa: E402
from forge_amd.geometry import _lattice, _surface_rows, extract_mesh, volume_iou, voxelize  # noqa: E402

VALU_PER_PAIR = 465.0 / 8.0
VALU_PER_PAIR_WEIGHTED = (465.0 + 32.0) / 8.0
FLOOR_RATE = 39.3e12        # lane-instructions / s: 157.3 TF / 4
ISSUE_RATE = 78.6e12        # lane-instructions / s: 1024 SIMDs x 32 lanes x 2.4 GHz
TORCH_QUERIES = 20_000
TORCH_PAIRS_PER_CHUNK = 1 << 22


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


def torch_winding(q, mesh):
    """w [Nq] of q [Nq,3] against one Mesh: the formula of section g3c composed of torch operators, chunked over the queries."""
    v, f = mesh.vertices, mesh.faces.long()
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    step = max(1, TORCH_PAIRS_PER_CHUNK // max(int(f.shape[0]), 1))
    out = []
    for i in range(0, q.shape[0], step):
        qc = q[i:i + step, None, :]
        A, B, C = a - qc, b - qc, c - qc
        la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
        num = (A * torch.linalg.cross(B, C)).sum(-1)
        den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
        out.append(torch.atan2(num, den).sum(dim=1) / (2.0 * math.pi))
    return torch.cat(out)


def kernel_line(what, pairs, t):
    floor = pairs * VALU_PER_PAIR / FLOOR_RATE * 1e3
    return ("%s: %.3f ms (%.3f, %.3f) = %.3f T pairs/s | VALU floor %.3f ms: %.0f %% of it reached (%.0f %% with v_sqrt / v_rcp counted twice; "
            "%.0f %% of the 32-lane issue rate)"
            % (what, *t, pairs / t[0] / 1e9, floor, 100.0 * floor / t[0], 100.0 * pairs * VALU_PER_PAIR_WEIGHTED / FLOOR_RATE * 1e3 / t[0],
               100.0 * pairs * VALU_PER_PAIR / ISSUE_RATE * 1e3 / t[0]))


def torch_line(what, q, meshes, kernel_rate, reps):
    """The torch composition on the first TORCH_QUERIES queries of every pair, as a rate, against the kernel's."""
    n = min(TORCH_QUERIES, int(q.shape[1]))
    run = lambda: [torch_winding(q[b, :n], m) for b, m in enumerate(meshes)]      # noqa: E731
    got = run()
    w = ops.winding_number(q[:, :n].contiguous(), *_rows(meshes))
    worst = max(float((g - w[b]).abs().max()) for b, g in enumerate(got))
    t = clock(run, reps)
    pairs = float(n) * sum(int(m.faces.shape[0]) for m in meshes)
    return ("%s, torch composition on the first %d queries: %.3f ms (%.3f, %.3f) = %.4f T pairs/s: the kernel is %.1f x that rate | largest "
            "|w_torch - w_kernel| there %.2e" % (what, n, *t, pairs / t[0] / 1e9, kernel_rate / (pairs / t[0] / 1e9), worst))


def _rows(meshes):
    vertices, faces, counts, offsets = _surface_rows(meshes, "winding_probe")
    return vertices, faces, counts, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda")
    Q, T = ops.nn_constants()[0], ops.nn_tile_faces()
    lines = ["winding_number / voxelize / volume_iou; median (min, max) of %d calls, host clock around a synchronise; %d queries per workgroup, tiles of "
             "%d faces, %.1f vector instructions per (query, face) pair (%.1f with v_sqrt / v_rcp counted twice)"
             % (args.reps, Q, T, VALU_PER_PAIR, VALU_PER_PAIR_WEIGHTED)]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    n = 100_000
    for B, D in ((1, 64), (1, 128), (8, 64)):
        meshes = extract_mesh(syn.blob_volumes(B, D, C=4, seed=1)[1].to(dev))
        gt = extract_mesh(syn.blob_volumes(B, D, C=4, seed=2)[1].to(dev))
        vertices, faces, counts, offsets = _rows(meshes)
        nfaces = "+".join(str(int(c)) for c in counts[:, 1].tolist())
        total = float(counts[:, 1].sum())
        q = (torch.rand(B, n, 3, device=dev, generator=torch.Generator(dev).manual_seed(3)) - 0.5).contiguous()
        run = lambda: ops.winding_number(q, vertices, faces, counts, offsets=offsets)      # noqa: E731
        for _ in range(2):
            run()
        t = clock(run, args.reps)
        what = "%d x %d queries against the %s faces of %d^3 extractions, winding_number" % (B, n, nfaces, D)
        emit(kernel_line(what, n * total, t))
        emit(torch_line(what, q, meshes, n * total / t[0] / 1e9, max(1, args.reps // 2)))
        run_i = lambda: volume_iou(meshes, gt, n=n)      # noqa: E731
        for _ in range(2):
            res = run_i()
        t_i = clock(run_i, args.reps)
        emit("%d pairs of %d^3 extractions, volume_iou at n = %d (two winding_number calls, the boxes, the counts): %.3f ms (%.3f, %.3f) | iou %s"
             % (B, D, n, *t_i, " ".join("%.4f" % x for x in res["iou"].tolist())))
        if B == 1:
            lat = _lattice((D, D, D), 1.0, dev)
            run_v = lambda: voxelize(meshes, (D, D, D))      # noqa: E731
            for _ in range(2):
                occ = run_v()
            t_v = clock(run_v, max(1, args.reps // 2))
            what = "voxelize at %d^3: %d lattice points against %s faces" % (D, lat.shape[0], nfaces)
            emit(kernel_line(what, lat.shape[0] * total, t_v) + " | %d voxels inside" % int(occ.sum()))
            emit(torch_line(what, lat[None], meshes, lat.shape[0] * total / t_v[0] / 1e9, max(1, args.reps // 2)))
        del meshes, gt, q
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
