"""Probe of the photograph ingest (forge_amd/ingest.py, csrc/ingest.hip) on the MI355X, beside the only other route: Pillow on one host core.

    python tools/ingest_probe.py [--reps 20] [--out profiles/rNN_ingest_probe.txt]

One scene's frames at three source sizes, RGBA, resized to 256 x 256 on a black background:
    kubric    10 frames of 256 x 256    (both passes are copies: nothing to resample)
    omni      10 frames of 800 x 800    (OmniObject3D)
    phone      3 frames of 4032 x 3024  (12 MP photographs, demo.py's three frames)
Per size, medians over --reps timed repetitions after warm-up:
    ingest + upload   host clock around: uint8 frames (pageable numpy) -> device -> both kernels -> torch.cuda.synchronize()
    device only       HIP events around the two kernels, frames already on the device
    Pillow + upload   host clock around the loaders' steps per frame (Image.fromarray, resize LANCZOS, mask resize NEAREST, / 255, times mask),
                      np.stack, float32, .cuda(), synchronize - where Pillow imports; the reference's route
    roofline          bytes the design moves (source once, the 4-byte-per-pixel intermediate written and read once, the float outputs) over the
                      device-only time, as a fraction of 6.29 TB/s, the rate a float4 copy kernel reaches on this chip (8 TB/s on the data sheet)
The results are also checked: the device bytes against Pillow's, 0 differing, at every size.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
SIZES = (("kubric", 10, 256, 256), ("omni", 10, 800, 800), ("phone", 3, 4032, 3024))
S = 256


def frames_of(n, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for v in range(n):
        smooth = (128 + 100 * np.sin(xx / (9.0 + v)) * np.cos(yy / (7.0 + v)))[..., None]
        img = np.clip(smooth + rng.integers(-40, 41, size=(H, W, 3)), 0, 255).astype(np.uint8)
        alpha = (((xx - W / 2) / (0.4 * W)) ** 2 + ((yy - H / 2) / (0.35 * H)) ** 2 < 1.0).astype(np.uint8) * 255
        out.append(np.ascontiguousarray(np.dstack([img, alpha])))
    return np.stack(out)


def pillow_route(frames):
    from PIL import Image
    rgbs, masks = [], []
    for f in frames:
        mask = Image.fromarray((f[:, :, 3] > 0).astype(float)).resize((S, S), Image.NEAREST)
        rgb = Image.fromarray(f[:, :, :3]).resize((S, S), Image.LANCZOS)
        mask = np.asarray(mask)[None]
        rgbs.append(np.asarray(rgb).transpose(2, 0, 1) / 255.0 * mask)
        masks.append(mask)
    return torch.from_numpy(np.stack(rgbs).astype(np.float32)).cuda(), torch.from_numpy(np.stack(masks).astype(np.float32)).cuda()


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def device_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_probe: needs the MI355X (a timing taken elsewhere says nothing)")
    from forge_amd import ingest as ig
    try:
        import PIL
        pil = PIL.__version__
    except ImportError:
        pil = None
    lines = ["ingest probe: %s, torch %s, Pillow %s, %d repetitions, medians (min)" % (torch.cuda.get_device_name(0), torch.__version__, pil, args.reps)]
    for name, n, H, W in SIZES:
        frames = frames_of(n, H, W, seed=H + n)
        dev = torch.from_numpy(frames).cuda()
        ig.ingest(dev, S)                                       # builds the coefficient tables (host) and their device copies, once per size pair
        up = median_ms(lambda: ig.ingest(frames, S), args.reps)
        on = device_ms(lambda: ig.ingest(dev, S), args.reps)
        moved = n * (H * W * 4 + 2 * H * S * 4 + S * S * 16)
        frac = moved / (on[0] * 1e-3) / HBM_BYTES_PER_S
        line = "%-7s %2d x %4d x %4d RGBA -> %d^2 | ingest + upload %8.3f ms (%.3f) | device only %7.3f ms (%.3f) | %6.1f MB moved, %4.1f %% of the HBM copy rate" % (
            name, n, H, W, S, up[0], up[1], on[0], on[1], moved / 1e6, 100 * frac)
        if pil:
            reps = max(3, args.reps // 4) if H * W > 1 << 20 else args.reps
            pl = median_ms(lambda: pillow_route(frames), reps, warm=1)
            from PIL import Image
            want = np.stack([np.asarray(Image.fromarray(f[:, :, :3]).resize((S, S), Image.LANCZOS)) for f in frames])
            got = ig.ingest(dev, S, return_bytes=True)[2].cpu().numpy()
            line += " | Pillow + upload %9.3f ms (%.3f), x %.1f | %d bytes differ" % (pl[0], pl[1], pl[0] / up[0], int((got != want).sum()))
        lines.append(line)
        print(line, flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(lines[0])


if __name__ == "__main__":
    main()
