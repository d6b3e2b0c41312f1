#!/usr/bin/env python
"""One SHA-256 per output tensor of the geometry stack and the image metrics, over fixed inputs: the listing two builds must share bit for bit.

    python tools/geometry_digest.py [--json FILE]

Only ops-level calls are used (ops.mesh_count / mesh_emit, mesh_bake, surface_sample, nn_points, geom_metrics, components_label / stats /
select, metrics.psnr / ssim / LPIPS), so the same file runs from a checkout of any commit that has them. Inputs come from the case modules of
tests/: volumes from 1x1x1 and 7x8x9 up to 24^3 and one batch of three, every mesh call padded and packed, with and without features, a bake
over 3 views, point sets of 257 x 300 points (two query blocks, a ragged last LDS tile). Every output is written into zeroed tensors or is fully
defined, so no digest depends on what an allocation held. "image/lpips" runs the whole seeded LPIPS module, so it also pins the convolution trunk
and torch's seeded CPU generator: a deliberate change of either regenerates that one entry. tests/golden/geometry_digests.json is this listing;
tests/test_gpu_geometry_digests.py asserts that the tree still reproduces it."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PATHS = [os.path.join(ROOT, "tests"), ROOT]
sys.path[:0] = _PATHS                              # for the imports below only: an importer's sys.path is left as it was
try:
    import bake_cases as bc
    import geom_cases as gc
    import mesh_cases as mc
    from forge_amd import metrics as fm
    from forge_amd import ops
finally:
    del sys.path[:len(_PATHS)]


def volumes():
    """(name, density [n,D,H,W] float32 numpy, level)"""
    return [("1x1x1", mc.ones(1)[None], 0.5),
            ("7x8x9", mc.quantised((7, 8, 9), 3)[None], mc.QUANT_LEVEL),
            ("blob12", mc.blob(12)[None], 0.5),
            ("ellipsoid16", mc.ellipsoid(16)[None], 0.5),
            ("torus24", mc.torus(24)[None], 0.5),
            ("batch3_blob8", np.stack([mc.blob(8, c) for c in ((0.06, -0.04, 0.02), (-0.05, 0.03, -0.07), (0.0, 0.0, 0.0))]), 0.5)]


def _exclusive(counts):
    return (torch.cumsum(counts, dim=0, dtype=torch.int32) - counts).contiguous()


def digests(dev="cuda"):
    out = {}

    def put(name, t):
        assert name not in out, name
        a = t.detach().cpu().contiguous().numpy()
        out[name] = hashlib.sha256(("%s%s" % (a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()

    def zeros(*shape, dtype=torch.float32, fill=0):
        return torch.full(shape, fill, dtype=dtype, device=dev)

    for name, dens_np, level in volumes():
        n, D, H, W = dens_np.shape
        dens = torch.from_numpy(dens_np).to(dev).reshape(n, 1, D, H, W).contiguous()
        feat = ops.to_channels_last_3d(torch.from_numpy(np.stack([mc.random_features(8, (D, H, W), 11 + k) for k in range(n)])).to(dev))
        counts, ws = ops.mesh_count(dens, level)
        put(name + "/mesh/counts", counts)
        host = counts.cpu()
        cap_v, cap_f = (max(int(x), 1) for x in host.max(dim=0).values)
        tot_v, tot_f = (max(int(x), 1) for x in host.sum(dim=0))
        offsets = _exclusive(counts)
        images = torch.from_numpy(bc.random_images(3, 3, 16, 16, 5)).to(dev)
        cam = torch.from_numpy(np.ascontiguousarray(bc.pack(bc.orbit(3, phase_deg=15.0, elev_deg=(0.0, 20.0, -20.0)), 16, 16), dtype=np.float32)).to(dev)
        v2v = torch.arange(3, dtype=torch.int32, device=dev) % n
        step, S, offset = bc.defaults((D, H, W))
        half = tuple(float(h) for h in bc.half_extents((D, H, W)))
        layouts = [("padded", None, (n,), cap_v, cap_f), ("packed", offsets, (), tot_v, tot_f), ("padded_half", None, (n,), max(cap_v // 2, 1), max(cap_f // 2, 1))]
        for lay, offs, lead, mv, mf in layouts:
            for fname, f in (("nofeat", None), ("feat", feat)):
                bufs = (zeros(*lead, mv, 3), zeros(*lead, mv, 3), zeros(*lead, mf, 3, dtype=torch.int32), None if f is None else zeros(*lead, mv, 8))
                v, nr, fa, vf, status = ops.mesh_emit(dens, ws, counts, mv, mf, level, 1.0, f, offsets=offs, out=bufs)
                tag = "%s/mesh/%s/%s/" % (name, lay, fname)
                for k, t in (("vertices", v), ("normals", nr), ("faces", fa), ("features", vf), ("status", status)):
                    if t is not None:
                        put(tag + k, t)
            bake_out = (zeros(*lead, mv, 3), zeros(*lead, mv), zeros(*lead, mv, dtype=torch.int32, fill=-1))
            for mode in ("blend", "best") if min(D, H, W) > 1 else ():       # a one-voxel axis has half extent 0: forge_mesh_bake refuses it
                cwb = ops.mesh_bake(v, nr, counts, dens, images, cam, v2v, offsets=offs, half=half, S=S, step=step, offset=offset, mode=mode, out=bake_out)
                for k, t in zip(("colors", "weight", "best"), cwb):
                    put("%s/bake/%s/%s/%s" % (name, lay, mode, k), t)
            smp = ops.surface_sample(v, fa, counts, 300, offsets=offs)
            for k, t in zip(("points", "normals", "face", "bary", "status"), smp):
                put("%s/sample/%s/%s" % (name, lay, k), t)
            if lay == "packed":
                pts, pn = smp[0], smp[1]
        # the samples of this volume set against a shifted copy of themselves
        d2_ab, idx_ab = ops.nn_points(pts, (pts.flip(1) + 0.01).contiguous())
        d2_ba, idx_ba = ops.nn_points((pts.flip(1) + 0.01).contiguous(), pts)
        for k, t in (("d2_ab", d2_ab), ("idx_ab", idx_ab), ("d2_ba", d2_ba), ("idx_ba", idx_ba)):
            put("%s/nn_samples/%s" % (name, k), t)
        m, st = ops.geom_metrics(d2_ab, idx_ab, d2_ba, idx_ba, pn, pn.flip(1).contiguous(), thresholds=(0.01, 0.02, 0.05))
        put(name + "/geom_metrics/out", m)
        put(name + "/geom_metrics/status", st)
        labels, kcounts, cws = ops.components_label(dens, level)
        put(name + "/components/labels", labels)
        put(name + "/components/counts", kcounts)
        for k, t in zip(("sizes", "bbox", "coord_sum", "status"), ops.components_stats(dens, cws, 8)):
            put(name + "/components/stats/" + k, t)
        for keep in (True, False):
            put("%s/components/select/largest=%d" % (name, keep), ops.components_select(dens, cws, keep_largest=keep, min_voxels=2, min_fraction=0.25))

    # point sets: 257 queries (two blocks of 256), 300 references (a ragged second tile), 3 pairs
    q = torch.from_numpy(gc.uniform_points((3, 257, 3), 1)).to(dev)
    p = torch.from_numpy(gc.uniform_points((3, 300, 3), 2)).to(dev)
    nq = torch.from_numpy(gc.sphere_points(3 * 257, seed=3)[1].reshape(3, 257, 3)).to(dev)
    npn = torch.from_numpy(gc.sphere_points(3 * 300, seed=4)[1].reshape(3, 300, 3)).to(dev)
    qc = torch.tensor([257, 256, 1], dtype=torch.int32, device=dev)
    pc = torch.tensor([300, 257, 255], dtype=torch.int32, device=dev)
    xf = torch.tensor([[1, 0, 0, 0.01, 0, 1, 0, -0.02, 0, 0, 1, 0.03], [0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0], [0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0.5, 0.1]],
                      dtype=torch.float32, device=dev)
    for tag, kw in (("plain", {}), ("counts_xf", dict(q_count=qc, p_count=pc, xf=xf))):
        d2_ab, idx_ab, qx = ops.nn_points(q, p, return_transformed=True, **kw)
        d2_ba, idx_ba = ops.nn_points(p, qx, kw.get("p_count"), kw.get("q_count"))
        for k, t in (("d2_ab", d2_ab), ("idx_ab", idx_ab), ("q_xf", qx), ("d2_ba", d2_ba), ("idx_ba", idx_ba)):
            put("points/%s/%s" % (tag, k), t)
        for ntag, na, nb in (("normals", nq, npn), ("nonormals", None, None)):
            m, st = ops.geom_metrics(d2_ab, idx_ab, d2_ba, idx_ba, na, nb, kw.get("q_count"), kw.get("p_count"), thresholds=(0.05, 0.1, 0.2, 0.4))
            put("points/%s/metrics/%s/out" % (tag, ntag), m)
            put("points/%s/metrics/%s/status" % (tag, ntag), st)

    # image metrics
    rng = np.random.default_rng(21)
    a = torch.from_numpy(rng.random((2, 3, 40, 52), dtype=np.float32)).to(dev)
    b = (a + torch.from_numpy(0.1 * rng.standard_normal((2, 3, 40, 52)).astype(np.float32)).to(dev)).clamp(0, 1)
    put("image/psnr", fm.psnr(a, b))
    put("image/ssim", fm.ssim(a, b))
    put("image/ssim_strided", fm.ssim(a[..., ::2], b[..., ::2]))
    a64 = torch.from_numpy(rng.random((2, 3, 64, 64), dtype=np.float32)).to(dev)
    b64 = torch.from_numpy(rng.random((2, 3, 64, 64), dtype=np.float32)).to(dev)
    with torch.no_grad():
        put("image/lpips", fm.LPIPS(pretrained=False).to(dev)(a64, b64, normalize=True))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="also write the listing to this file")
    args = ap.parse_args()
    d = digests()
    for k in sorted(d):
        print(d[k], k)
    print("%d tensors, digest of the listing %s" % (len(d), hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(d, fh, indent=0, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
