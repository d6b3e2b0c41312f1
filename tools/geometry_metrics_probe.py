#!/usr/bin/env python
"""forge_amd.geometry.point_metrics / mesh_metrics on the MI355X, timed, at the sizes object-reconstruction benchmarks use: point_metrics at
1 x 1e4 x 1e4, 1 x 1e5 x 1e5 and 8 x 1e5 x 1e5 points (two noisy samplings of one sphere: the near-identical regime the metric exists for), and
mesh_metrics on one 64^3 and one 128^3 extracted volume (synthetic.blob_volumes densities, level 0.5) at n = 1e5 samples per side.

Per point configuration: the whole call (both directions, the reduction, the allocation of its outputs), one direction of forge_nn_points alone,
and two yardsticks for that one direction:
  1. the only other route on the device: chunked torch.cdist(q, p).min(dim), chunks sized to a 1 GiB distance matrix, with the largest
     difference of its distances to the kernel's (cdist takes the expanded |q|^2 + |p|^2 - 2 q.p form at these sizes);
  2. the kernel's own VALU floor: pairs x VALU_PER_PAIR / 39.3e12 lane-instructions/s (the 157.3 TF fp32 vector peak / 4: single-width, mostly
     non-fma instructions). VALU_PER_PAIR = 113 / 16: the vector instructions of the compiled inner loop of nn_points_kernel (hipcc -O3
     --offload-arch=gfx950, two groups of 8 references per iteration: 48 v_sub, 16 v_mul, 32 v_fmac, 8 v_min3, 2 v_cmp, 4 v_cndmask, 3 v_mov).
     The floor's rate counts 16 lanes per SIMD and clock; the same count at the 32 lanes per clock a wave64 instruction issues at is printed beside it.

Everything is warmed up; host clock around a device synchronise; median (min, max) of --reps calls.

    python tools/geometry_metrics_probe.py [--reps 20] [--torch-reps 3] [--out profiles/r25_geometry_metrics_probe.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from forge_amd import ops, synthetic as syn  # noqa: E402
from forge_amd.geometry import extract_mesh, mesh_metrics, point_metrics, sample_surface  # noqa: E402

VALU_PER_PAIR = 113.0 / 16.0
FLOOR_RATE = 39.3e12        # lane-instructions / s: 157.3 TF / 4
ISSUE_RATE = 78.6e12        # lane-instructions / s: 1024 SIMDs x 32 lanes x 2.4 GHz
CDIST_BYTES = 1 << 30


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


def cdist_nn(q, p):
    """d [B,Nq] by torch.cdist(...).min(dim) in chunks of queries whose distance matrix is 1 GiB."""
    B, Nq, Np = q.shape[0], q.shape[1], p.shape[1]
    rows = max(1, CDIST_BYTES // (4 * Np * B))
    return torch.cat([torch.cdist(q[:, lo:lo + rows], p).min(dim=2)[0] for lo in range(0, Nq, rows)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    Q, T = ops.nn_constants()
    lines = ["point_metrics / mesh_metrics; median (min, max) of %d calls, host clock around a synchronise; %d queries per workgroup, tiles of %d "
             "references, %.4f vector instructions per pair" % (args.reps, Q, T, VALU_PER_PAIR)]
    for B, N in ((1, 10_000), (1, 100_000), (8, 100_000)):
        a = torch.nn.functional.normalize(torch.randn(B, N, 3, device=dev), dim=2) * 0.3
        b = (a + 0.001 * torch.randn_like(a))[:, torch.randperm(N, device=dev)].contiguous()
        na, nb = torch.nn.functional.normalize(a, dim=2), torch.nn.functional.normalize(b, dim=2)
        run_all = lambda: point_metrics(a, b, na, nb)                      # noqa: E731
        run_nn = lambda: ops.nn_points(a, b)                               # noqa: E731
        run_cd = lambda: cdist_nn(a, b)                                    # noqa: E731
        for _ in range(3):
            run_all()
            run_nn()
        run_cd()
        t_all, t_nn, t_cd = clock(run_all, args.reps), clock(run_nn, args.reps), clock(run_cd, args.torch_reps)
        d = ops.nn_points(a, b)[0].double().sqrt()
        diff = float((run_cd().double() - d).abs().max())
        pairs = float(B) * N * N
        floor = pairs * VALU_PER_PAIR / FLOOR_RATE * 1e3
        res = run_all()
        lines.append("%d x %d x %d: point_metrics %.3f ms (%.3f, %.3f) | one direction of nn_points %.3f ms (%.3f, %.3f) = %.2f T pairs/s | "
                     "VALU floor %.3f ms: %.0f %% of it reached (%.0f %% of the 32-lane issue rate) | chunked cdist + min %.2f ms (%.2f, %.2f) = %.1f x "
                     "the kernel; largest |d_cdist - d_kernel| %.2e at mean d %.2e | chamfer_l1 %.3e, fscore@0.01 %.4f"
                     % (B, N, N, *t_all, *t_nn, pairs / t_nn[0] / 1e9, floor, 100.0 * floor / t_nn[0],
                        100.0 * pairs * VALU_PER_PAIR / ISSUE_RATE * 1e3 / t_nn[0], *t_cd, t_cd[0] / t_nn[0], diff, float(d.mean()),
                        float(res["chamfer_l1"][0]), float(res["fscore@0.01"][0])))
        print(lines[-1], flush=True)
        del a, b, na, nb, d
    n = 100_000
    for D in (64, 128):
        pred = extract_mesh(syn.blob_volumes(1, D, C=4, seed=1)[1].to(dev))
        gt = extract_mesh(syn.blob_volumes(1, D, C=4, seed=2)[1].to(dev))
        run_s = lambda: sample_surface(pred, n)                            # noqa: E731
        run_m = lambda: mesh_metrics(pred, gt, n=n)                        # noqa: E731
        for _ in range(3):
            run_s()
            run_m()
        t_s, t_m = clock(run_s, args.reps), clock(run_m, args.reps)
        res = run_m()
        lines.append("D = %3d: %d / %d faces | sample_surface n = %d: %.3f ms (%.3f, %.3f) | mesh_metrics (two samplings, both directions, reduction) "
                     "%.3f ms (%.3f, %.3f) | chamfer_l1 %.4f, fscore@0.02 %.4f, normal_consistency %.4f"
                     % (D, pred[0].faces.shape[0], gt[0].faces.shape[0], n, *t_s, *t_m, float(res["chamfer_l1"][0]), float(res["fscore@0.02"][0]),
                        float(res["normal_consistency"][0])))
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
