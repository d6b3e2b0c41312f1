#!/usr/bin/env python
"""forge_amd.geometry.bake_vertex_colors on the MI355X, timed, at the volumes the encoder produces: one 64^3 and one 128^3 volume and eight 128^3
volumes (synthetic.blob_volumes densities, level 0.5), each volume with 3 photographs + 28 rendered views at 256^2 (random pixels: the time does not
depend on them; cameras: three look-at cameras and the 28 of nvs.nvs_cameras, as geometry.colored_mesh passes them).

Per configuration: the bake's time in both row layouts (a list of Mesh: packed rows, one host-to-device copy of the counts; a MeshBatch: padded
rows, no host work), vertices per second and contract samples per second (vertices x views x S: what the contract sums over; most lie behind the
camera or outside the volume's support box and cost no gather), the samples that do gather (inside the support box, before the camera), and two
lower bounds on the launch's time from its bytes: the compulsory bytes (rows in and out, the density and the images once) at the 8 TB/s HBM peak, and
the gathered taps (8 x 4 B per gathering sample) at the 34.5 TB/s aggregate L2 rate. The larger bound over the measured time is the fraction reached:
an end-to-end figure of one call (launch latency included), not a kernel's share of peak.

Beside it the only other route on the device: the same weights and colours as a torch composition (F.grid_sample for the segments and for the image
taps, one view at a time), with its largest difference to the kernel. Last, the tolerances of tests/test_gpu_bake.py as measured here: per scene
4 x |float32 restatement - float64 restatement| and the kernel's own error against float64.

Everything is warmed up; host clock around a device synchronise; median (min, max) of --reps calls.

    python tools/bake_probe.py [--reps 30] [--torch-reps 2] [--out profiles/r19_bake_probe.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from forge_amd import nvs, synthetic as syn  # noqa: E402
from forge_amd.geometry import bake_vertex_colors, extract_mesh  # noqa: E402

HBM_PEAK = 8.0e12       # bytes / s, HBM3E peak of the MI355X
L2_RATE = 34.5e12       # bytes / s, the eight L2s together
IMG, PHOTOS, RENDERED, CAMERA_Z = 256, 3, 28, 1.5


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


def cameras(n, dev):
    """[n * 31, 16] packed cameras (scene-major: 3 photographs, then the 28 orbit views), view2vol, gains."""
    import bake_cases as bc
    K = syn.intrinsics(IMG)
    photo = torch.from_numpy(bc.pack(bc.orbit(PHOTOS, CAMERA_Z, elev_deg=15.0, phase_deg=200.0), IMG, IMG))
    R, T = nvs.nvs_cameras(CAMERA_Z, RENDERED)
    orbit = torch.cat([R.reshape(-1, 9), T, K[0, 0].expand(RENDERED, 1), K[1, 1].expand(RENDERED, 1), K[0, 2].expand(RENDERED, 1), K[1, 2].expand(RENDERED, 1)], dim=1)
    per = torch.cat([photo, orbit])
    V = per.shape[0]
    gain = torch.cat([torch.ones(PHOTOS), torch.full((RENDERED,), 0.05)])
    return per.repeat(n, 1).to(dev).contiguous(), torch.arange(n, dtype=torch.int32).repeat_interleave(V).to(dev), gain.repeat(n).to(dev)


def torch_bake(v, nh, dens, images, cam, gain, half, S, step, offset, cos_power=2, z_near=1e-3, w_min=1e-3, fill=0.5):
    """One volume's rows by stock torch ops, one view at a time. Returns (colors, weight, samples that gather)."""
    rows, (Hi, Wi) = v.shape[0], images.shape[-2:]
    dev = v.device
    hv = torch.tensor(half, device=dev)
    p0 = v + offset * nh
    t = (torch.arange(S, device=dev, dtype=torch.float32) + 0.5) * step
    box = hv * (1.0 + 2.0 / (torch.tensor(dens.shape[:1:-1], device=dev, dtype=torch.float32) - 1.0))          # support: one voxel beyond the border samples
    wsum, acc, gathers = torch.zeros(rows, device=dev), torch.zeros(rows, images.shape[1], device=dev), 0
    for k in range(cam.shape[0]):
        R, T, (fx, fy, cx, cy) = cam[k, :9].reshape(3, 3), cam[k, 9:12], cam[k, 12:]
        q = v @ R.T + T
        x, y = fx * q[:, 0] / q[:, 2] + cx - 0.5, fy * q[:, 1] / q[:, 2] + cy - 0.5
        seen = (q[:, 2] >= z_near) & (x >= 0) & (x <= Wi - 1) & (y >= 0) & (y <= Hi - 1)
        g2 = torch.stack([2 * x / (Wi - 1) - 1, 2 * y / (Hi - 1) - 1], dim=1).reshape(1, rows, 1, 2)
        c = F.grid_sample(images[k][None], g2, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0].T
        d = -(R.T @ T) - v
        dist = d.norm(dim=1)
        u = d / dist[:, None]
        facing = (nh * u).sum(dim=1).clamp(min=0) ** cos_power
        pos = p0[:, None, :] + t[None, :, None] * u[:, None, :]
        live = t[None, :] < dist[:, None]
        gathers += int(((pos.abs() < box).all(dim=2) & live & (seen & (facing > 0))[:, None]).sum())
        a = F.grid_sample(dens, (pos / hv).reshape(1, rows, S, 1, 3), mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, :, :, 0]
        w = gain[k] * (1.0 - torch.where(live, a.clamp(0, 1), torch.zeros_like(a))).prod(dim=1) * facing * seen
        wsum += w
        acc += w[:, None] * c
    colors = torch.where((wsum >= w_min)[:, None], acc / wsum[:, None], torch.full_like(acc, fill))
    return colors, wsum, gathers


def tolerances(lines):
    """The scenes of tests/test_gpu_bake.py: allowed = 4 x |fp32 restatement - float64 restatement|, beside the kernel's error against float64."""
    import bake_cases as bc
    import test_gpu_bake as tg
    lines.append("tolerances of tests/test_gpu_bake.py (w_min = %g): allowed = 4 x max |float32 restatement - float64 restatement| per scene" % tg.W_MIN)
    for name in bc.SCENES:
        meshes, extras = tg.bake(name)
        r64, r32 = tg.references(name, 0)
        for k, (m, (w, _)) in enumerate(zip(meshes, extras)):
            sure = r64[k].weight >= 2 * tg.W_MIN
            lines.append("  %-26s volume %d, %4d rows: colour %.3g allowed, %.3g measured | weight %.3g allowed, %.3g measured"
                         % (name, k, len(sure), 4 * np.abs(r32[k].colors - r64[k].colors)[sure].max(),
                            np.abs(m.colors.cpu().numpy() - r64[k].colors)[sure].max(), 4 * np.abs(r32[k].weight - r64[k].weight).max(),
                            np.abs(w.cpu().numpy() - r64[k].weight).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda")
    lines = ["bake_vertex_colors on synthetic.blob_volumes densities, %d photographs + %d rendered views at %d^2 per volume; median (min, max) of %d calls, "
             "host clock around a synchronise" % (PHOTOS, RENDERED, IMG, args.reps)]
    for D, n in ((64, 1), (128, 1), (128, 8)):
        dens = syn.blob_volumes(n, D, C=4, seed=1)[1].to(dev)
        meshes = extract_mesh(dens)
        mv, mf = max(m.vertices.shape[0] for m in meshes), max(m.faces.shape[0] for m in meshes)
        batch = extract_mesh(dens, max_vertices=mv, max_faces=mf)
        cam, v2v, gain = cameras(n, dev)
        V = cam.shape[0]
        images = torch.rand(V, 3, IMG, IMG, device=dev)
        step = 1.0 / D
        S = int(math.ceil(1.8 / step))
        half = tuple(0.5 * (D - 1) / D for _ in range(3))
        run_list = lambda: bake_vertex_colors(meshes, dens, images, cam, v2v, view_gain=gain)
        run_batch = lambda: bake_vertex_colors(batch, dens, images, cam, v2v, view_gain=gain)
        for _ in range(3):
            run_list()
            run_batch()
        t_list, t_batch = clock(run_list, args.reps), clock(run_batch, args.reps)
        out, extras = run_list()
        rows = sum(m.vertices.shape[0] for m in meshes)
        per = V // n
        # the torch composition, volume by volume
        def run_torch():
            res = []
            for k, m in enumerate(meshes):
                sl = slice(k * per, (k + 1) * per)
                res.append(torch_bake(m.vertices, m.normals, dens[k:k + 1], images[sl], cam[sl], gain[sl], half, S, step, step))
            return res
        res = run_torch()
        t_torch = clock(run_torch, args.torch_reps)
        gathers = sum(r[2] for r in res)
        dc = max(float((r[0] - o.colors).abs().max()) for r, o in zip(res, out))
        dw = max(float((r[1] - e[0]).abs().max()) for r, e in zip(res, extras))
        compulsory = rows * (24 + 12 + 8) + dens.numel() * 4 + images.numel() * 4 + V * 72
        bound_hbm, bound_l2 = compulsory / HBM_PEAK * 1e3, gathers * 32 / L2_RATE * 1e3
        bound = max(bound_hbm, bound_l2)
        lines.append("D = %3d, n = %d: %7d vertices, %3d views, S = %d | list of Mesh %.3f ms (%.3f, %.3f) | MeshBatch %.3f ms (%.3f, %.3f) | "
                     "%.1f M vertices/s, %.2f G contract samples/s, %.2f G gathering samples (%.1f %% of the contract's) = %.2f G/s | "
                     "bounds: %.1f MB compulsory = %.4f ms at the 8 TB/s HBM peak, %.1f MB of taps = %.4f ms at 34.5 TB/s of L2: %.1f %% of the %s bound reached | "
                     "torch composition %.1f ms (%.1f, %.1f) = %.0f x; largest difference to it: colour %.2g, weight %.2g"
                     % (D, n, rows, V, S, *t_list, *t_batch, rows / t_batch[0] / 1e3, rows * per * S / t_batch[0] / 1e6, gathers / 1e9,
                        100.0 * gathers / (rows * per * S), gathers / t_batch[0] / 1e6, compulsory / 1e6, bound_hbm, gathers * 32 / 1e6, bound_l2,
                        100.0 * bound / t_batch[0], "L2" if bound_l2 > bound_hbm else "HBM", *t_torch, t_torch[0] / t_batch[0], dc, dw))
        print(lines[-1], flush=True)
    tolerances(lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
