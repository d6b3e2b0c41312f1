#!/usr/bin/env python
"""forge_amd.geometry.fit_similarity / align_points / mesh_metrics(align="icp") on the MI355X, timed (include/forge_hip.h section g5):
  1. fit_similarity (known correspondences) at 1 x 1e4, 1 x 2e4, 1 x 1e5 and 8 x 1e5 points;
  2. at the same sizes one forge_align_step alone - an UPDATING step (with scale and rejection: moments, SVD, the lot; the state is put back before
     every timed call, outside the clock) and a statistics-only one - beside the one forge_nn_points that feeds it, and the updating step's share
     of an iteration (step / (step + search));
  3. align_points at 32 iterations on 2e4 points against a RESAMPLED copy of the surface under a 25 degree motion, from the identity, and under a
     100 degree motion with the 24 cube starts; beside it the only other route on the device, a torch composition of the same loop (chunked
     torch.cdist(...).min, centred covariance, torch.linalg.svd), and - if scipy imports - a cKDTree ICP on one host core, copies included;
  4. mesh_metrics(align="icp") on one 64^3 and one 128^3 extraction (three Gaussian lumps of different sizes, level 0.5: no symmetry, so the
     rotation is observable) against a copy moved by 15 degrees whose faces are shuffled, so that the deterministic sampler draws other points
     of the same surface;
  5. how the recovered transform moves with the alignment's sample count n in {5e3, 1e4, 2e4, 5e4} on that pair.
The data of 2 and 3 is the asymmetric shape of tests/align_cases.py (an ellipsoid with a spherical bump), sampled with a seeded generator.

Everything is warmed up; host clock around a device synchronise; median (min, max) of --reps calls (--torch-reps for the torch composition; the
scipy route runs once).

    python tools/align_probe.py [--reps 10] [--torch-reps 3] [--out profiles/r28_align_probe.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from forge_amd import ops  # noqa: E402
from forge_amd.geometry import Mesh, align_meshes, align_points, extract_mesh, fit_similarity, mesh_metrics, rotation_starts  # noqa: E402

CDIST_BYTES = 1 << 30


def clock(fn, reps, setup=None):
    """median, min, max in ms of `reps` calls of fn; setup() runs before each, outside the clock."""
    ts = []
    for _ in range(reps):
        if setup is not None:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def shape(B, n, seed, dev):
    """[B,n,3] float32: the ellipsoid (0.40, 0.25, 0.15) whose first n // 3 points lie on a sphere of radius 0.10 about (0.30, 0.15, 0.05)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g, dtype=torch.float64), dim=2)
    pts = u * torch.tensor([0.40, 0.25, 0.15], dtype=torch.float64)
    k = n // 3
    pts[:, :k] = u[:, :k] * 0.10 + torch.tensor([0.30, 0.15, 0.05], dtype=torch.float64)
    return pts.to(dev)


def lumpy(D, dev):
    """[1,1,D,D,D] float32: 1.5 exp(-|x - c|^2 / w) summed over three lumps, on the voxel-centre world grid extract_mesh uses (volume_size 1)."""
    ax = (torch.arange(D, dtype=torch.float64) - 0.5 * (D - 1)) / D
    Z, Y, X = torch.meshgrid(ax, ax, ax, indexing="ij")
    d = torch.zeros_like(X)
    for (cx, cy, cz), w in (((-0.05, 0.0, 0.0), 0.06), ((0.22, 0.10, 0.02), 0.012), ((-0.08, 0.20, 0.15), 0.008)):
        d += 1.5 * torch.exp(-((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) / w)
    return d.float()[None, None].contiguous().to(dev)


def motion(angle_deg, axis, scale=1.0, shift=(0.0, 0.0, 0.0)):
    k = torch.tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    t = math.radians(angle_deg)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = scale * (torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K))
    M[:3, 3] = torch.tensor(shift, dtype=torch.float64)
    return M


def moved(x, M):
    M = M.to(x.device)
    return (x.double() @ M[:3, :3].T + M[:3, 3]).float().contiguous()


def miss(T, M):
    """(largest |T - M| over the entries, the angle between the two rotations in degrees)."""
    T, M = T.double().cpu(), M.double().cpu()
    Ra, Rb = T[:3, :3] / T[:3, :3].det().abs() ** (1 / 3), M[:3, :3] / M[:3, :3].det().abs() ** (1 / 3)
    c = ((Ra @ Rb.T).trace() - 1) / 2
    return float((T - M).abs().max()), math.degrees(math.acos(max(-1.0, min(1.0, float(c)))))


def cdist_nn(q, p):
    B, Nq, Np = q.shape[0], q.shape[1], p.shape[1]
    rows = max(1, CDIST_BYTES // (4 * Np * B))
    return torch.cat([torch.cdist(q[:, lo:lo + rows], p).min(dim=2)[1] for lo in range(0, Nq, rows)], dim=1)


def torch_icp(a, b, iterations):
    """The same loop from torch calls: chunked cdist + min, centred covariance, torch.linalg.svd with the determinant fix. [B,4,4] float64."""
    B = a.shape[0]
    a64, b64 = a.double(), b.double()
    R = torch.eye(3, dtype=torch.float64, device=a.device).expand(B, 3, 3)
    t = torch.zeros(B, 3, dtype=torch.float64, device=a.device)
    for _ in range(iterations):
        cur = (a64 @ R.transpose(1, 2) + t[:, None]).float()
        idx = cdist_nn(cur, b)
        p = torch.gather(b64, 1, idx[..., None].expand(-1, -1, 3))
        qm, pm = a64.mean(dim=1), p.mean(dim=1)
        H = (p - pm[:, None]).transpose(1, 2) @ (a64 - qm[:, None])
        U, _, Vt = torch.linalg.svd(H)
        d = torch.linalg.det(U @ Vt)
        D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=1))
        R = U @ D @ Vt
        t = pm - (R @ qm[..., None])[..., 0]
    T = torch.eye(4, dtype=torch.float64, device=a.device).repeat(B, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = R, t
    return T


def scipy_icp(a, b, iterations):
    """cKDTree ICP on one host core, the copies to and from the device included; None without scipy."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    import numpy as np
    A, Bp = a[0].double().cpu().numpy(), b[0].double().cpu().numpy()
    tree = cKDTree(Bp)
    R, t = np.eye(3), np.zeros(3)
    for _ in range(iterations):
        _, idx = tree.query(A @ R.T + t, workers=1)
        P = Bp[idx]
        qm, pm = A.mean(axis=0), P.mean(axis=0)
        U, _, Vt = np.linalg.svd((P - pm).T @ (A - qm))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        R = U @ D @ Vt
        t = pm - R @ qm
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return torch.from_numpy(T).to(a.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda")
    lines = ["fit_similarity / align_step / align_points / mesh_metrics(align='icp'); median (min, max) of %d calls (the torch composition: of %d; the "
             "scipy route: one run), host clock around a synchronise; %d workgroups per pair in the moments pass"
             % (args.reps, args.torch_reps, ops.align_blocks())]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    M25, M100 = motion(25, (3, -1, 2), 1.0, (0.02, 0.04, -0.05)), motion(100, (2, -1, 3), 1.0, (0.03, 0.02, -0.04))
    # 1, 2: the step and the search that feeds it
    for B, N in ((1, 10_000), (1, 20_000), (1, 100_000), (8, 100_000)):
        a = shape(B, N, 1, dev).float().contiguous()
        b = moved(shape(B, N, 2, dev), motion(5, (1, 2, 3), 1.0, (0.01, 0.0, -0.01)))
        state, xf, status = ops.align_state(None, B, dev)
        d2, idx = ops.nn_points(a, b, None, None, xf)
        run_nn = lambda: ops.nn_points(a, b, None, None, xf)                                        # noqa: E731
        state0, status0 = state.clone(), status.clone()

        def restore():                                 # every timed update starts from the same state: a second update on the same matches would
            state.copy_(state0)                        # find DELTA = 0, and a third would meet a frozen pair that does nothing
            status.copy_(status0)
        run_step = lambda: ops.align_step(a, b, state, xf, status, idx=idx, d2=d2, with_scale=True, reject=3.0)        # noqa: E731  (moments + the whole solve)
        run_stat = lambda: ops.align_step(a, b, state, xf, status, idx=idx, d2=d2, update=False)    # noqa: E731  (moments + statistics: no SVD)
        run_fit = lambda: fit_similarity(a, b)                                                      # noqa: E731
        for _ in range(3):
            restore()
            run_nn(), run_step(), run_fit()
        t_nn, t_step, t_fit = clock(run_nn, args.reps), clock(run_step, args.reps, restore), clock(run_fit, args.reps)
        restore()
        t_stat = clock(run_stat, args.reps)
        say("%d x %d points: align_step, an update (moments, SVD, scale, next threshold) %.3f ms (%.3f, %.3f), %.1f MB read = %.0f GB/s; statistics only "
            "(update=0) %.3f ms (%.3f, %.3f) | nn_points %.3f ms (%.3f, %.3f) | an updating step is %.1f %% of an iteration | fit_similarity (a step, "
            "residuals, a statistics step, select) %.3f ms (%.3f, %.3f)"
            % (B, N, *t_step, B * N * 32 / 1e6, B * N * 32 / t_step[0] / 1e6, *t_stat, *t_nn, 100 * t_step[0] / (t_step[0] + t_nn[0]), *t_fit))
        del a, b, d2, idx
    # 3: the loop
    N = 20_000
    a = shape(1, N, 1, dev).float().contiguous()
    for name, M, starts in (("25 degrees, from the identity", M25, None), ("100 degrees, 24 cube starts", M100, rotation_starts("cube").to(dev))):
        b = moved(shape(1, N, 2, dev), M)
        run = lambda: align_points(a, b, iterations=32, starts=starts)                              # noqa: E731
        for _ in range(2):
            run()
        t = clock(run, args.reps)
        res = run()
        e, ang = miss(res.transform[0], M)
        say("align_points 1 x %d, 32 iterations, %s: %.2f ms (%.2f, %.2f) | start %d, %d updates, rmse %.3e, |T - M| %.2e, %.4f degrees off"
            % (N, name, *t, int(res.start[0]), int(res.iterations[0]), float(res.rmse[0]), e, ang))
        if starts is None:
            run_t = lambda: torch_icp(a, b, 32)                                                     # noqa: E731
            run_t()
            tt = clock(run_t, args.torch_reps)
            e, ang = miss(run_t()[0], M)
            say("  torch composition (chunked cdist + min, centred covariance, torch.linalg.svd), 32 iterations, median (min, max) of %d calls: %.2f ms "
                "(%.2f, %.2f) = %.1f x | |T - M| %.2e, %.4f degrees off" % (args.torch_reps, *tt, tt[0] / t[0], e, ang))
            t0 = time.perf_counter()
            Ts = scipy_icp(a, b, 32)
            if Ts is None:
                say("  scipy does not import here: no cKDTree ICP on the host")
            else:
                ts = (time.perf_counter() - t0) * 1e3
                e, ang = miss(Ts, M)
                say("  scipy cKDTree ICP on one host core, copies included, 32 iterations, one run: %.1f ms = %.1f x | |T - M| %.2e, %.4f degrees off"
                    % (ts, ts / t[0], e, ang))
    # 4, 5: meshes
    M15 = motion(15, (1, 2, 3), 1.0, (0.05, -0.03, 0.02))
    for D in (64, 128):
        (pred,) = extract_mesh(lumpy(D, dev))
        perm = torch.randperm(pred.faces.shape[0], generator=torch.Generator().manual_seed(3)).to(dev)
        gt = Mesh(moved(pred.vertices, M15), (pred.normals.double() @ M15[:3, :3].T.to(dev)).float(), pred.faces[perm].contiguous())
        run = lambda: mesh_metrics(pred, gt, align="icp")                                           # noqa: E731
        plain = lambda: mesh_metrics(pred, gt)                                                      # noqa: E731
        for _ in range(2):
            run(), plain()
        t, tp = clock(run, args.reps), clock(plain, args.reps)
        res, raw = run(), plain()
        e, ang = miss(res["alignment"].transform[0], M15)
        say("D = %3d, %d faces: mesh_metrics(align='icp') %.2f ms (%.2f, %.2f), of which mesh_metrics itself %.2f ms (%.2f, %.2f) | chamfer_l1 %.5f "
            "unaligned, %.5f aligned, fscore@0.01 %.4f -> %.4f | %d updates, |T - M| %.2e, %.4f degrees off"
            % (D, pred.faces.shape[0], *t, *tp, float(raw["chamfer_l1"][0]), float(res["chamfer_l1"][0]), float(raw["fscore@0.01"][0]),
               float(res["fscore@0.01"][0]), int(res["alignment"].iterations[0]), e, ang))
        if D == 64:
            for n in (5_000, 10_000, 20_000, 50_000):
                run_n = lambda: align_meshes(pred, gt, n=n)                                         # noqa: E731
                run_n()
                tn = clock(run_n, args.reps)
                al = run_n()
                e, ang = miss(al.transform[0], M15)
                say("  align_meshes n = %5d (32 iterations): %.2f ms (%.2f, %.2f) | rmse %.3e, |T - M| %.2e, %.4f degrees off" % (n, *tn, float(al.rmse[0]), e, ang))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
