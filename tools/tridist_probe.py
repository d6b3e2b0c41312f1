#!/usr/bin/env python
"""forge_amd.ops.nn_triangles and mesh_metrics(surface="triangles") on the MI355X, timed, at the sizes object-reconstruction benchmarks use, and
what the triangles buy: the same surfaces scored in both modes at two sample counts.

  1. one direction of nn_triangles: 1e5 queries (samples of one extraction) against the triangles of another, for one 64^3 and one 128^3
     extracted volume (synthetic.blob_volumes densities, level 0.5) and for 8 pairs of 64^3 volumes, beside the kernel's own VALU floor:
     (query, face) pairs x VALU_PER_PAIR / 39.3e12 lane-instructions/s (the 157.3 TF fp32 vector peak / 4, as tools/geometry_metrics_probe.py
     counts it). VALU_PER_PAIR = 668 / 8: the vector instructions of the compiled inner loop of nn_triangles_kernel (hipcc -O3
     --offload-arch=gfx950, one group of 8 faces per iteration: 114 v_cndmask, 120 v_cmp, 86 v_fmac, 49 v_pk_fma, 52 v_pk_add, 25 v_pk_mul,
     50 v_sub, 24 v_add, 46 v_mul, 8 v_rcp, 4 v_min3, 1 v_cmp for the group, 89 moves). The same count at the 32 lanes per clock a wave64
     instruction issues at is printed beside it.
  2. mesh_metrics(surface="triangles") beside mesh_metrics(surface="samples") (the code path as it was) on the same meshes at the same n.
  3. what the change buys: a Gaussian blob extracted at 64^3, against a second extraction of the same field moved by a known sub-voxel
     offset, scored under the transform that undoes the offset, in both modes at n = 1e4 and 1e5. What is left is the discretisation of the
     two extractions; in samples mode the sampling floor of about 0.5 sqrt(area / n) lies on top of it and moves with n.

Everything is warmed up; host clock around a device synchronise; median (min, max) of --reps calls.

    python tools/tridist_probe.py [--reps 10] [--out profiles/r29_tridist_probe.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from forge_amd import ops, synthetic as syn  # noqa: E402
from forge_amd.geometry import _surface_rows, extract_mesh, mesh_metrics, sample_surface  # noqa: E402

VALU_PER_PAIR = 668.0 / 8.0
FLOOR_RATE = 39.3e12        # lane-instructions / s: 157.3 TF / 4
ISSUE_RATE = 78.6e12        # lane-instructions / s: 1024 SIMDs x 32 lanes x 2.4 GHz


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


def shifted_blob(D, offset):
    """1.5 exp(-|x - c|^2 / 0.08) on the voxel-centre world grid of D^3 samples, c = offset (x, y, z) -> [1,1,D,D,D]."""
    lin = (torch.arange(D, dtype=torch.float64) - 0.5 * (D - 1)) / D
    Z, Y, X = torch.meshgrid(lin, lin, lin, indexing="ij")
    r2 = (X - offset[0]) ** 2 + (Y - offset[1]) ** 2 + (Z - offset[2]) ** 2
    return (1.5 * torch.exp(-r2 / 0.08)).to(torch.float32)[None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda")
    Q, T = ops.nn_constants()[0], ops.nn_tile_faces()
    lines = ["nn_triangles / mesh_metrics(surface='triangles'); median (min, max) of %d calls, host clock around a synchronise; %d queries per "
             "workgroup, tiles of %d faces, %.1f vector instructions per (query, face) pair" % (args.reps, Q, T, VALU_PER_PAIR)]
    n = 100_000
    for B, D in ((1, 64), (1, 128), (8, 64)):
        pred = extract_mesh(syn.blob_volumes(B, D, C=4, seed=1)[1].to(dev))
        gt = extract_mesh(syn.blob_volumes(B, D, C=4, seed=2)[1].to(dev))
        q = sample_surface(pred, n)[0]
        vertices, faces, counts, offsets = _surface_rows(gt, "tridist_probe")
        run_t = lambda: ops.nn_triangles(q, vertices, faces, counts, offsets=offsets, want_normal=True)      # noqa: E731
        run_p = lambda: ops.nn_points(q, sample_surface(gt, n)[0])                                           # noqa: E731
        for _ in range(2):
            run_t()
        t_t = clock(run_t, args.reps)
        pairs = float(n) * float(counts[:, 1].sum())
        floor = pairs * VALU_PER_PAIR / FLOOR_RATE * 1e3
        lines.append("%d x %d queries against the %s faces of %d^3 extractions: one direction of nn_triangles %.3f ms (%.3f, %.3f) = %.2f T pairs/s | "
                     "VALU floor %.3f ms: %.0f %% of it reached (%.0f %% of the 32-lane issue rate)"
                     % (B, n, "+".join(str(int(c)) for c in counts[:, 1].tolist()), D, *t_t, pairs / t_t[0] / 1e9, floor, 100.0 * floor / t_t[0],
                        100.0 * pairs * VALU_PER_PAIR / ISSUE_RATE * 1e3 / t_t[0]))
        print(lines[-1], flush=True)
        if B == 1:
            run_p()
            t_p = clock(run_p, args.reps)
            run_mt = lambda: mesh_metrics(pred, gt, n=n, surface="triangles")                                # noqa: E731
            run_ms = lambda: mesh_metrics(pred, gt, n=n)                                                     # noqa: E731
            for _ in range(2):
                run_mt()
                run_ms()
            t_mt, t_ms = clock(run_mt, args.reps), clock(run_ms, args.reps)
            rt, rs = run_mt(), run_ms()
            lines.append("D = %3d, n = %d: mesh_metrics triangles %.3f ms (%.3f, %.3f) | samples %.3f ms (%.3f, %.3f) | sampling gt + one direction of "
                         "nn_points %.3f ms (%.3f, %.3f) | chamfer_l1 %.5f / %.5f, fscore@0.01 %.4f / %.4f, normal_consistency %.4f / %.4f "
                         "(triangles / samples)"
                         % (D, n, *t_mt, *t_ms, *t_p, float(rt["chamfer_l1"][0]), float(rs["chamfer_l1"][0]), float(rt["fscore@0.01"][0]),
                            float(rs["fscore@0.01"][0]), float(rt["normal_consistency"][0]), float(rs["normal_consistency"][0])))
            print(lines[-1], flush=True)
        del pred, gt, q
    D = 64
    shift = (0.3 / D, -0.45 / D, 0.2 / D)                      # a known sub-voxel offset, in world units
    a = extract_mesh(shifted_blob(D, (0.0, 0.0, 0.0)).to(dev))
    b = extract_mesh(shifted_blob(D, shift).to(dev))
    back = torch.eye(4, device=dev)
    back[:3, 3] = -torch.tensor(shift, device=dev)
    area = float(a[0].area())
    for n in (10_000, 100_000):
        rt = mesh_metrics(b, a, n=n, surface="triangles", transform=back, thresholds=(0.01,))
        rs = mesh_metrics(b, a, n=n, surface="samples", transform=back, thresholds=(0.01,))
        st = mesh_metrics(a, a, n=n, surface="triangles", thresholds=(0.01,))
        lines.append("blob at 64^3 against itself moved by (%.5f, %.5f, %.5f) and moved back, n = %6d (0.5 sqrt(area / n) = %.5f): chamfer_l1 triangles "
                     "%.6f, samples %.6f | fscore@0.01 triangles %.4f, samples %.4f | the mesh against itself, triangles: chamfer_l1 %.2e"
                     % (*shift, n, 0.5 * (area / n) ** 0.5, float(rt["chamfer_l1"][0]), float(rs["chamfer_l1"][0]), float(rt["fscore@0.01"][0]),
                        float(rs["fscore@0.01"][0]), float(st["chamfer_l1"][0])))
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
