"""The photograph-ingest contract (include/forge_hip.h section h) restated in numpy, and the cases the ingest tests run on.

The contract is Pillow's 8-bit resampler (Image.resize with Image.LANCZOS on an RGB image, Image.NEAREST on the mask) as the reference's loaders use
it (dataset/kubric.py:410-445, dataset/gso.py:257-290, dataset/omniobject3d.py:221-258, demo.py:236-256). Everything after the coefficient table is
integer arithmetic, so the restatement, the library and Pillow agree byte for byte: tests/golden/ingest_pillow.npz (tools/make_golden_ingest.py)
holds Pillow's own output for every case below.

Nothing here imports the library or Pillow. math.sin, not numpy.sin: the table must come from the C library's sin, as Pillow's and the library's do.
"""
import math

import numpy as np

PRECISION_BITS = 22
BACKGROUNDS = ("black", "white", "premasked")

# (name, H, W, Ho, Wo). `noise` cases carry cells of pure 0 / 255 noise (the clip fires at both ends), `alpha` holds every alpha in {0, 1, 128, 255}.
CASES = (
    ("h7w5_4", 7, 5, 4, 4),
    ("h13w29_8", 13, 29, 8, 8),
    ("h8w8_8", 8, 8, 8, 8),                 # both passes are copies
    ("h5w9_16", 5, 9, 16, 16),              # up-scaling
    ("h301w257_32", 301, 257, 32, 32),      # noise
    ("h64w100_32", 64, 100, 32, 32),        # noise, alpha
    ("h1w3_4", 1, 3, 4, 4),
    ("h33w32_32", 33, 32, 32, 32),          # the horizontal pass is a copy
    ("h3w4100_4x8", 3, 4100, 4, 8),         # 3075 taps per output: more than one staged chunk of a row
    ("h6w10_9", 6, 10, 9, 9),               # nearest-mask taps that land on exact integers (6 / 9 (y + 0.5))
)
NOISE_CASES = ("h301w257_32", "h64w100_32")
ALPHA_CASE = "h64w100_32"
TABLES = ((301, 32), (5, 16), (4100, 8))


def source(name, H, W):
    """The RGBA source of a case, uint8 [H, W, 4], from a generator seeded by the case's name."""
    rng = np.random.default_rng([ord(c) for c in name])
    img = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = ((yy * 7 + xx * 3) % 256).astype(np.uint8)
    img[..., 1] = (img[..., 1] // 4 + ramp // 2).astype(np.uint8)                      # a smooth component: not every output sits at mid-grey
    alpha = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    alpha[rng.random((H, W)) < 0.3] = 0                                                # holes: the mask has both values
    alpha[rng.random((H, W)) < 0.3] = 255
    if name == ALPHA_CASE:
        alpha = np.array([0, 1, 128, 255], np.uint8)[rng.integers(0, 4, size=(H, W))]
    img[..., 3] = alpha
    if name in NOISE_CASES:
        # cells of pure 0 / 255, a few output pixels wide: Lanczos over- and undershoots at their edges, so the clip fires at both ends
        cell = 12 if H > 256 else 5
        h2 = H // 2
        cells = 255 * rng.integers(0, 2, size=(-(-h2 // cell), -(-W // cell), 3), dtype=np.uint8)
        img[:h2, :, :3] = np.repeat(np.repeat(cells, cell, axis=0), cell, axis=1)[:h2, :W]
    if name == "h7w5_4":
        img[0, 0, :2] = 0                                                              # a 3-channel mask needs a pixel with R = G = 0 ...
        img[0, 1, :3] = (0, 0, 200)                                                    # ... and one where only blue is set (it plays no part)
    return img


PHOTO_SHAPES = ((300, 280), (256, 256), (333, 410))       # three frames of one object, differing sizes; the second needs no resampling
PHOTO_SIZE = 256


def photo_frames():
    """Three RGBA 'photographs' of a shaded blob on a transparent background (uint8 [H, W, 4] each): smooth inside, so their resized bytes compress
    well in the golden file, with the object's edge cutting through alpha."""
    frames = []
    for v, (H, W) in enumerate(PHOTO_SHAPES):
        yy, xx = np.mgrid[0:H, 0:W]
        u, w = (xx + 0.5) / W - 0.5, (yy + 0.5) / H - 0.5
        a = 0.6 * v
        r2 = ((u * math.cos(a) + w * math.sin(a)) / 0.34) ** 2 + ((w * math.cos(a) - u * math.sin(a)) / 0.22) ** 2
        shade = np.clip(1.0 - 0.7 * r2, 0.0, 1.0)
        rgb = np.stack([40 + 200 * shade * (0.6 + 0.4 * np.cos(6 * u + v)), 30 + 180 * shade * (0.5 + 0.5 * np.sin(5 * w - v)), 60 + 150 * shade], axis=-1)
        img = np.concatenate([rgb, np.where(r2 < 1.0, 255.0, 0.0)[..., None]], axis=-1)
        frames.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return frames


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def coeffs(n_in, n_out):
    """(first [n_out], count [n_out], k [n_out, K]) int32, rows zero-padded to K = the largest count. All float64 until the last step."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    inv = 1.0 / fs                                           # the argument is multiplied by 1 / fs, not divided by fs
    rows, first, count = [], [], []
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - lo
        w = [_lanczos((j + lo - c + 0.5) * inv) for j in range(n)]
        s = 0.0
        for v in w:
            s += v
        if s != 0.0:
            w = [v / s for v in w]
        rows.append([int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in w])
        first.append(lo)
        count.append(n)
    K = max(count)
    k = np.zeros((n_out, K), np.int32)
    for i, r in enumerate(rows):
        k[i, :len(r)] = r
    return np.array(first, np.int32), np.array(count, np.int32), k


def nearest(n_in, n_out):
    """Source index of every output sample of a nearest-neighbour resize: int(p_i), p_0 = 0.5 s, p_{i+1} = p_i + s, s = n_in / n_out - the running
    float64 sum, not (i + 0.5) s: the two differ where a tap lands on an integer."""
    s = n_in / n_out
    p = s * 0.5
    out = []
    for _ in range(n_out):
        out.append(min(int(p), n_in - 1))
        p += s
    return np.array(out, np.int32)


def resample_axis(img, n_out, axis, clips=None):
    """One pass over uint8 [H, W, ch] along `axis` (0 or 1); a pass whose sizes agree is a copy. clips: a two-element list that takes the number
    of results clipped at 0 and at 255."""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img.copy()
    first, count, k = coeffs(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for i in range(n_out):
        acc = np.tensordot(k[i, :count[i]].astype(np.int64), src[first[i]:first[i] + count[i]], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                                             # the contract's accumulator is int32
        if clips is not None:
            clips[0] += int(((acc >> PRECISION_BITS) < 0).sum())
            clips[1] += int(((acc >> PRECISION_BITS) > 255).sum())
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def source_mask(img):
    """alpha > 0 with 4 channels; (R > 0) | (G > 0) with 3: blue plays no part (the third operand of np.logical_or at omniobject3d.py:228-230 is `out=`)."""
    return img[..., 3] > 0 if img.shape[-1] == 4 else (img[..., 0] > 0) | (img[..., 1] > 0)


def composite_white(img):
    c, a = img[..., :3].astype(np.int32), img[..., 3:].astype(np.int32)
    t = c * a + 255 * (255 - a) + 128
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def ingest(img, Ho, Wo, background, clips=None):
    """uint8 [H, W, 3 or 4] -> (bytes uint8 [Ho, Wo, 3], images float32 [3, Ho, Wo], mask float32 [1, Ho, Wo])."""
    rgb = img[..., :3]
    if img.shape[-1] == 4 and background == "white":
        rgb = composite_white(img)
    elif img.shape[-1] == 4 and background == "premasked":
        rgb = rgb * (img[..., 3:] > 0)
    out = resample_axis(resample_axis(np.ascontiguousarray(rgb), Wo, 1, clips), Ho, 0, clips)       # horizontal first: the 8-bit intermediate is H x Wo
    m = source_mask(img)[nearest(img.shape[0], Ho)][:, nearest(img.shape[1], Wo)]
    f = (out.astype(np.float64) / 255.0).transpose(2, 0, 1)
    if background == "black":
        f = f * m[None]
    return out, f.astype(np.float32), m[None].astype(np.float32)


def key(name, channels, background):
    return "%s/c%d/%s" % (name, channels, background)
