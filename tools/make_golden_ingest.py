"""Writes tests/golden/ingest_pillow.npz: Pillow's own output (Image.LANCZOS on the RGB image, Image.NEAREST on the mask, paste over white) for the
cases of tests/ingest_cases.py, with 3 and 4 channels and the three backgrounds, as the reference's loaders call it (dataset/kubric.py:410-445,
dataset/omniobject3d.py:221-258, demo.py:236-256). The sources come from the seeded generator of tests/ingest_cases.py and are not stored.

    python tools/make_golden_ingest.py

Pillow does not export its coefficient tables. The three stored tables are the restatement's, and this script refuses to write them unless
(a) the restatement reproduces every Pillow byte of every case and (b) each row agrees with Pillow's float resampler on unit impulses (mode "F",
float64 coefficients, float32 result) to within half a fixed-point step plus the float32 rounding.
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ingest_cases as ic  # noqa: E402


def pillow_ingest(img, Ho, Wo, background):
    """The loaders' steps on one uint8 [H, W, C] frame -> (bytes [Ho, Wo, 3], images float32 [3, Ho, Wo], mask float32 [1, Ho, Wo])."""
    if img.shape[-1] == 4:
        src_mask = img[:, :, 3] > 0
    else:
        src_mask = np.logical_or(img[:, :, 0] > 0, img[:, :, 1] > 0)
    mask = Image.fromarray(src_mask.astype(float))
    if img.shape[-1] == 4 and background == "white":
        pil = Image.fromarray(img, "RGBA")
        canvas = Image.new("RGBA", pil.size, "WHITE")
        canvas.paste(pil, (0, 0), pil)
        rgb = canvas.convert("RGB")
    elif img.shape[-1] == 4 and background == "premasked":
        rgb = Image.fromarray(img[:, :, :3] * np.uint8(img[:, :, 3:] > 0))
    else:
        rgb = Image.fromarray(np.ascontiguousarray(img[:, :, :3]))
    rgb = np.asarray(rgb.resize((Wo, Ho), Image.LANCZOS))
    mask = np.asarray(mask.resize((Wo, Ho), Image.NEAREST))[None]
    f = rgb.transpose(2, 0, 1) / 255.0
    if background == "black":
        f = f * mask
    return rgb, f.astype(np.float32), mask.astype(np.float32)


def check_table_against_pillow(n_in, n_out):
    first, count, k = ic.coeffs(n_in, n_out)
    worst = 0.0
    for j in range(n_in):
        imp = np.zeros((1, n_in), np.float32)
        imp[0, j] = 1.0
        w = np.asarray(Image.fromarray(imp, "F").resize((n_out, 1), Image.LANCZOS))[0].astype(np.float64)
        mine = np.zeros(n_out)
        for i in range(n_out):
            if first[i] <= j < first[i] + count[i]:
                mine[i] = k[i, j - first[i]] / float(1 << ic.PRECISION_BITS)
        worst = max(worst, np.abs(mine - w).max())
    assert worst <= 0.5 / (1 << ic.PRECISION_BITS) + 2.0 ** -24, (n_in, n_out, worst)
    return first, count, k


def main():
    out = {}
    for name, H, W, Ho, Wo in ic.CASES:
        rgba = ic.source(name, H, W)
        for ch in (3, 4):
            img = np.ascontiguousarray(rgba[:, :, :ch])
            for bg in ic.BACKGROUNDS:
                b, f, m = pillow_ingest(img, Ho, Wo, bg)
                clips = [0, 0]
                rb, rf, rm = ic.ingest(img, Ho, Wo, bg, clips)
                assert name not in ic.NOISE_CASES or min(clips) > 0, (name, ch, bg, clips)       # the clip fires at both ends
                assert np.array_equal(b, rb) and np.array_equal(f.view(np.int32), rf.view(np.int32)) and np.array_equal(m, rm), (name, ch, bg)
                out[ic.key(name, ch, bg) + "/bytes"] = b
                out[ic.key(name, ch, bg) + "/mask"] = m[0].astype(np.uint8)
        print("%-14s clipped at 0: %d, at 255: %d (4 channels, premasked), mask mean %.2f" % (name, clips[0], clips[1], float(m.mean())))
    for n_in, n_out in ic.TABLES:
        if n_in <= 512:
            first, count, k = check_table_against_pillow(n_in, n_out)
        else:
            first, count, k = ic.coeffs(n_in, n_out)              # 4100 impulses through Pillow's byte path instead: the h3w4100_4x8 case above
        out["table/%d_%d/first" % (n_in, n_out)], out["table/%d_%d/count" % (n_in, n_out)], out["table/%d_%d/k" % (n_in, n_out)] = first, count, k
    photos = []
    for img in ic.photo_frames():                                # what demo.py:236-256 makes of them; the clips of the reconstruct_photos test
        b, _, _ = pillow_ingest(img, ic.PHOTO_SIZE, ic.PHOTO_SIZE, "premasked")
        assert np.array_equal(b, ic.ingest(img, ic.PHOTO_SIZE, ic.PHOTO_SIZE, "premasked")[0])
        photos.append(b)
    out["photos/premasked/bytes"] = np.stack(photos)
    path = os.path.join(ROOT, "tests", "golden", "ingest_pillow.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes (Pillow %s)" % (os.path.relpath(path, ROOT), len(out), os.path.getsize(path), Image.__version__))


if __name__ == "__main__":
    main()
