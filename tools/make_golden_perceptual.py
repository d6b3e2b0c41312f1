"""Golden of the VGG-16 perceptual loss from the reference's OWN class (models/perceptual_loss.py:7), CPU only, float64.

Puts the reference and oracle/shims on sys.path through oracle/ref_import.py (unchanged) and replaces, at runtime, the shim's
`torchvision.models.vgg16` by a constructor of VGG-16 configuration D whose features carry forge_amd.perceptual's seeded initialisation
(there is no network for the ImageNet checkpoint). Writes tests/golden/perceptual_vgg.npz:
  keys / shapes               the reference's state_dict() key list and shapes
  seed, wsum / wsq            per convolution (features[:23]) float64 sum and sum of squares of the seeded weights (RNG drift check)
  <case>_codesum              int64 sums of the 8-bit codes of input and target: the images themselves are not stored but made by
                              images() below from an integer hash (exact, independent of any RNG version); the tests import it
  <case>_loss                 the float64 loss
  <case>_grad, _gscale        d loss / d input as float16 of grad / gscale (gscale = max |grad|, float64), rows 0, s, 2s, ... of the image
  <case>_rowstep              s: 1, or 4 for case b (its full gradient alone would be 0.8 MB)
Cases: a (resize, 3 channels, 2 non-square upsampled pairs), b (3x256x256: the 256 -> 224 downsample), c (1 channel: the repeat path),
d (only_deepest), e (resize=False at 64x64).

    python tools/make_golden_perceptual.py      (needs the reference tree; seconds on a CPU)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SEED = 0
ROWSTEP = {"b": 4}
CASES = {            # name: (pairs, C, H, W, resize, only_deepest)
    "a": (2, 3, 48, 72, True, False),
    "b": (1, 3, 256, 256, True, False),
    "c": (1, 1, 64, 64, True, False),
    "d": (1, 3, 80, 64, True, True),
    "e": (1, 3, 64, 64, False, False),
}


def _codes(n, salt):
    """n 8-bit codes from an integer hash of (index, salt): uint64 arithmetic masked to 32 bits, identical on every platform and numpy."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(0x9E3779B9)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x45D9F3B)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x45D9F3B)) & m
    h ^= h >> np.uint64(16)
    return (h & np.uint64(255)).astype(np.uint8)


def images(case, pairs, C, H, W):
    """(input, target) of a golden case as 8-bit codes [pairs][C][H][W]; the loss sees code / 255 in float32."""
    n = pairs * C * H * W
    return _codes(n, 2 * ord(case)).reshape(pairs, C, H, W), _codes(n, 2 * ord(case) + 1).reshape(pairs, C, H, W)


def to_float(codes):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(255.0))


def main():
    import ref_import
    from forge_amd import perceptual as fp
    ref_import.import_reference()
    import torchvision

    sd = fp.seeded_vgg16_state_dict(SEED)

    class _VGG(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.features = fp.vgg16_features()
            self.features.load_state_dict({k[len("features."):]: v for k, v in sd.items()})

    torchvision.models.vgg16 = lambda pretrained=False, **kw: _VGG()
    import importlib
    pl = importlib.import_module("models.perceptual_loss")
    pl.torchvision.models.vgg16 = torchvision.models.vgg16
    torch.set_num_threads(max(1, os.cpu_count() or 1))

    out = {}
    ref = pl.VGGPerceptualLoss(resize=True)
    keys = list(ref.state_dict().keys())
    out["keys"] = np.array(keys)
    out["shapes"] = np.array([str(tuple(v.shape)) for v in ref.state_dict().values()])
    out["seed"] = np.array(SEED)
    conv_keys = [k for k in sd if int(k.split(".")[1]) < 23 and k.endswith("weight")]
    out["wkeys"] = np.array(conv_keys)
    out["wsum"] = np.array([sd[k].double().sum().item() for k in conv_keys])
    out["wsq"] = np.array([sd[k].double().square().sum().item() for k in conv_keys])
    for name, (pairs, C, H, W, resize, deepest) in CASES.items():
        m = pl.VGGPerceptualLoss(resize=resize).double()
        m.mean.requires_grad_(False)       # d loss / d input does not depend on them; skips the target-branch backward
        m.std.requires_grad_(False)
        for p in m.blocks.parameters():
            p.requires_grad_(False)
        inp, tgt = images(name, pairs, C, H, W)
        x, y = to_float(inp), to_float(tgt)
        x = x.double().requires_grad_(True)
        loss = m(x, y.double(), only_deepest=deepest)
        (grad,) = torch.autograd.grad(loss, x)
        step = ROWSTEP.get(name, 1)
        gs = grad[:, :, ::step].numpy()
        scale = float(np.abs(gs).max())
        out[name + "_codesum"] = np.array([int(inp.astype(np.int64).sum()), int(tgt.astype(np.int64).sum())])
        out[name + "_loss"] = np.array(loss.item())
        out[name + "_grad"] = (gs / scale).astype(np.float16)
        out[name + "_gscale"] = np.array(scale)
        out[name + "_rowstep"] = np.array(step)
        out[name + "_meta"] = np.array([pairs, C, H, W, int(resize), int(deepest)])
        print("case %s: %s loss %.10g |grad| %.4g" % (name, (pairs, C, H, W, resize, deepest), loss.item(), grad.norm().item()), flush=True)
    path = os.path.join(ROOT, "tests", "golden", "perceptual_vgg.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
