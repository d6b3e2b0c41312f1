"""Image metrics of the evaluation protocol (kubric_eval.py:297-311, scripts/kubric_validation.py) on the MI355X HIP kernels:

    psnr(pred, gt)             skimage.metrics.peak_signal_noise_ratio(gt, pred, data_range=1), per image        forge_psnr
    ssim(pred, gt)             skimage.metrics.structural_similarity(gt, pred, multichannel=True, data_range=1)   forge_ssim
    LPIPS(net="vgg")(in0, in1) lpips.LPIPS(net="vgg") (lpips 0.1): VGG-16 features[:30] on forge_amd/perceptual.py's trunk, then
                               forge_lpips_tap per tap and forge_lpips_finalize
    image_metrics(pred, gt, lpips)   all three for a batch of pairs, on the current stream, with no host synchronisation (graph-capturable)
    compute_img_metric(rgb, gt)      utils/eval_utils.py:compute_img_metric: numpy HWC in, Python floats (psnr, ssim) out

Images are float32 [N, C, H, W] on the device (any strides); image n of `pred` is scored against image n of `gt`. PSNR and SSIM are computed in
float64 (PSNR's squared differences, SSIM's window moments) and returned as float64 [N]. SSIM is the mean over all valid 7x7 windows: skimage
crops its map by 3 pixels on every side, so its boundary mode never reaches the result. Every reduction is a per-workgroup slab summed in a fixed
order: two calls give bitwise-identical results.

`from forge_amd import metrics as lpips; lpips.LPIPS(net="vgg")` replaces `import lpips; lpips.LPIPS(net="vgg")` (kubric_eval.py:16, 623).
Deliberate deviations from the lpips package (also in INTEGRATION.md):
  - metric only: the result never requires grad, even when the inputs do (no LPIPS gradient);
  - only net="vgg", version="0.1", lpips=True, spatial=False; anything else raises ValueError;
  - H and W must be multiples of 16 (four 2x2 pools); otherwise ValueError. VGG runs at the input size, as in lpips;
  - host tensors raise RuntimeError, as everywhere in the package.
Weights are never downloaded. The lin weights come from `model_path=`, else $FORGE_LPIPS_WEIGHTS, else an installed lpips package's
weights/v0.1/vgg.pth (found with importlib.util.find_spec, not imported); the VGG-16 weights from `vgg_weights=`, else perceptual.py's lookup
($FORGE_VGG16_WEIGHTS, the torch hub cache). pretrained=False: seeded CPU initialisations (seeded_vgg16_state_dict, seeded_lin_state_dict).
"""
import importlib.util
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import convops as co
from . import perceptual as fp

SSIM_WIN = 7
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
LIN_CHANNELS = (64, 128, 256, 512, 512)                       # channels of relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
LIN_FILE = os.path.join("weights", "v0.1", "vgg.pth")


def _check_pair(pred, gt, what):
    for t in (pred, gt):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("forge_amd ops need tensors on the MI355X (cuda/HIP device); got a %s. There is no CPU fallback."
                               % (t.device if torch.is_tensor(t) else type(t).__name__))
    if pred.dim() != 4 or pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError("%s: images must be [N, C, H, W] of the same shape on one device, got %s on %s and %s on %s"
                         % (what, tuple(pred.shape), pred.device, tuple(gt.shape), gt.device))
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise TypeError("%s: float32 images (got %s, %s)" % (what, pred.dtype, gt.dtype))
    if pred.shape[0] == 0 or pred.numel() == 0:
        raise ValueError("%s: empty batch %s" % (what, tuple(pred.shape)))


def _strides(t):
    return [int(s) for s in t.stride()]


@_lib.on_tensor_device
def _image_stat(entry, pred, gt, data_range, n_partial):
    lib, st = _lib.lib(), _lib.current_stream()
    N, C, H, W = pred.shape
    partial = torch.empty(n_partial, dtype=torch.float64, device=pred.device)
    out = torch.empty(N, dtype=torch.float64, device=pred.device)
    _lib.check(getattr(lib, entry)(_lib.ptr(pred), *_strides(pred), _lib.ptr(gt), *_strides(gt), N, C, H, W, float(data_range), _lib.ptr(partial),
                                   _lib.ptr(out), st), entry)
    return out


def psnr(pred, gt, data_range=1.0):
    """Per-image PSNR [N] (float64, on the device): 10 log10(data_range^2 / mse), mse over C H W in float64; +inf for identical images."""
    _check_pair(pred, gt, "psnr")
    return _image_stat("forge_psnr", pred.detach(), gt.detach(), data_range, pred.shape[0] * _lib.lib().forge_metric_blocks())


def ssim(pred, gt, data_range=1.0):
    """Per-image SSIM [N] (float64, on the device) with skimage's defaults as the reference calls them: 7x7 uniform window, sample covariance
    (49/48), K1 = 0.01, K2 = 0.03, the map averaged over all valid windows and over channels. H or W below 7 raises ValueError."""
    _check_pair(pred, gt, "ssim")
    N, C, H, W = pred.shape
    if H < SSIM_WIN or W < SSIM_WIN:
        raise ValueError("ssim: %dx%d images are smaller than the 7x7 window (skimage raises too)" % (H, W))
    return _image_stat("forge_ssim", pred.detach(), gt.detach(), data_range, N * C * _lib.lib().forge_ssim_tiles(H, W))


# ------------------------------------------------------------------------------------------------------------------------------------ LPIPS
def seeded_lin_state_dict(seed=0):
    """The documented seeded lin weights (pretrained=False): `lin{k}.model.1.weight` [1, C_k, 1, 1] = 0.1 * rand from a torch.Generator seeded
    with `seed`, float32: non-negative, as trained LPIPS weights are."""
    g = torch.Generator().manual_seed(int(seed))
    return {"lin%d.model.1.weight" % k: torch.rand(1, c, 1, 1, generator=g, dtype=torch.float32) * 0.1 for k, c in enumerate(LIN_CHANNELS)}


def default_lin_path():
    """$FORGE_LPIPS_WEIGHTS, else an installed lpips package's weights/v0.1/vgg.pth (located, not imported); FileNotFoundError naming all
    three sources otherwise."""
    env = os.environ.get("FORGE_LPIPS_WEIGHTS")
    if env and os.path.isfile(env):
        return env
    spec = importlib.util.find_spec("lpips")
    for d in (spec.submodule_search_locations or []) if spec is not None else []:
        p = os.path.join(d, LIN_FILE)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError("LPIPS(pretrained=True): no lin weights found. Looked for model_path= (not given), $FORGE_LPIPS_WEIGHTS (%s) and an "
                            "installed lpips package's %s (%s). Nothing is downloaded; pass model_path=, set $FORGE_LPIPS_WEIGHTS, or use "
                            "pretrained=False for the seeded initialisation." % (env or "unset", LIN_FILE, "package not found" if spec is None
                                                                                  else "not in the package"))


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1))


class _VGG16Slices(nn.Module):
    """lpips.pretrained_networks.vgg16's layout: slice{1..5} holding torchvision's features[:30] under their own indices."""

    def __init__(self):
        super().__init__()
        feats = fp.vgg16_features()
        for k, (lo, hi) in enumerate(fp.TRUNK_SLICES):
            s = nn.Sequential()
            for i in range(lo, hi):
                s.add_module(str(i), feats[i])
            setattr(self, "slice%d" % (k + 1), s)


class _NetLinLayer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(c, 1, 1, stride=1, padding=0, bias=False))


class LPIPS(co.PackedModule):
    """lpips.LPIPS(net="vgg") (version 0.1) with the lpips package's state_dict layout (`scaling_layer.shift/scale`, `net.slice{1..5}.N.*`,
    `lin{0..4}.model.1.weight`; `lins.{k}.model.1.weight` is accepted on load). forward(in0, in1, normalize=False) -> [N, 1, 1, 1] float32.
    Metric only: the result never requires grad. See the module docstring for the weight sources and the deviations."""

    def __init__(self, pretrained=True, net="vgg", version="0.1", lpips=True, spatial=False, model_path=None, vgg_weights=None, seed=0):
        super().__init__()
        if net != "vgg" or version != "0.1" or not lpips or spatial:
            raise ValueError("LPIPS: only net='vgg', version='0.1', lpips=True, spatial=False are implemented (got net=%r, version=%r, lpips=%r, "
                             "spatial=%r)" % (net, version, lpips, spatial))
        self.scaling_layer = _ScalingLayer()
        self.net = _VGG16Slices()
        for k, c in enumerate(LIN_CHANNELS):
            setattr(self, "lin%d" % k, _NetLinLayer(c))
        for p in self.parameters():
            p.requires_grad_(False)
        self._register_load_state_dict_pre_hook(_lins_alias)
        self.plan = {n: (fp.LAYER_PLAN[n][0], None) for n in fp.LAYER_NAMES[1:]}
        self._packed = co.PackCache()
        if vgg_weights is None:
            vgg_weights = fp.default_weights_path() if pretrained else fp.seeded_vgg16_state_dict(seed)
        self.load_vgg_weights(vgg_weights)
        if model_path is None:
            model_path = default_lin_path() if pretrained else seeded_lin_state_dict(seed)
        self.load_lin_weights(model_path)
        self.eval()

    def convs(self):
        """The thirteen nn.Conv2d of features[:30] in order (conv1_1 .. conv5_3)."""
        return [m for k in range(5) for m in getattr(self.net, "slice%d" % (k + 1)) if isinstance(m, nn.Conv2d)]

    def lins(self):
        return [getattr(self, "lin%d" % k).model[1] for k in range(5)]

    def load_vgg_weights(self, weights):
        """VGG-16 weights from a path or a dict in torchvision's layout (features.N.*, N < 30; the rest ignored) or in this class's (net.*)."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        own = {k: v for k, v in self.state_dict().items() if k.startswith("net.")}
        sd = {}
        for k, v in weights.items():
            if k.startswith("features."):
                _, n, leaf = k.split(".")
                for s, (lo, hi) in enumerate(fp.TRUNK_SLICES):
                    if lo <= int(n) < hi:
                        sd["net.slice%d.%s.%s" % (s + 1, n, leaf)] = v
            elif k in own:
                sd[k] = v
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError("VGG-16 weights lack %s" % ", ".join(missing))
        self.load_state_dict(sd, strict=False)

    def load_lin_weights(self, weights):
        """The five lin weights from a path or a dict (lpips's weights/v0.1/vgg.pth layout `lin{k}.model.1.weight`, or `lins.{k}.model.1.weight`;
        other keys ignored)."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        sd = {}
        for k in range(5):
            for key in ("lin%d.model.1.weight" % k, "lins.%d.model.1.weight" % k):
                if key in weights:
                    sd["lin%d.model.1.weight" % k] = weights[key]
                    break
            else:
                raise KeyError("LPIPS lin weights lack lin%d.model.1.weight" % k)
        self.load_state_dict(sd, strict=False)

    def _pack(self, device):
        convs, lins = self.convs(), self.lins()
        plan = tuple(self.plan[n] for n in fp.LAYER_NAMES[1:])
        if plan != self._plan_key:
            self._packed.clear()
            self._plan_key = plan
        shift, scale = self.scaling_layer.shift, self.scaling_layer.scale

        def build():
            sh = shift.detach().to(device=device, dtype=torch.float32).reshape(3).contiguous()
            sc = scale.detach().to(device=device, dtype=torch.float32).reshape(3).contiguous()
            return {"layers": fp.pack_layers(convs, plan, device),
                    "lins": [w.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous() for w in (m.weight for m in lins)],
                    # prep constants: (x - shift) / scale, and with normalize=True ((2x - 1) - shift) / scale = (x - (shift + 1) / 2) / (scale / 2)
                    "prep": {False: (sh, sc), True: (((sh + 1) / 2).contiguous(), (sc / 2).contiguous())}}
        return self._packed.get([p for m in convs for p in (m.weight, m.bias)] + [m.weight for m in lins] + [shift, scale], build)

    _plan_key = None

    def forward(self, in0, in1, normalize=False):
        _check_pair(in0, in1, "LPIPS")
        if self.scaling_layer.shift.device != in0.device:
            raise RuntimeError("LPIPS: move the module to the input's device (.to(%s)); there is no CPU fallback" % in0.device)
        N, C, H, W = in0.shape
        if C != 3:
            raise ValueError("LPIPS: 3-channel images, got C=%d" % C)
        if H % 16 or W % 16:
            raise ValueError("LPIPS: H and W must be multiples of 16, got %dx%d" % (H, W))
        with torch.no_grad(), torch.cuda.device(in0.device):
            return _lpips(in0.detach(), in1.detach(), self._pack(in0.device), bool(normalize)).view(N, 1, 1, 1)


def _lins_alias(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    """load_state_dict pre-hook: `lins.{k}.*` (the lpips package's ModuleList view of the same layers) loads as `lin{k}.*`."""
    for k in [k for k in state_dict if k.startswith(prefix + "lins.")]:
        rest = k[len(prefix) + len("lins."):]
        i, leaf = rest.split(".", 1)
        v = state_dict.pop(k)
        state_dict.setdefault("%slin%s.%s" % (prefix, i, leaf), v)


@_lib.on_tensor_device
def _lpips(in0, in1, P, normalize):
    lib, st = _lib.lib(), _lib.current_stream()
    N, _, H, W = in0.shape
    partial = torch.empty(5, N, lib.forge_metric_blocks(), dtype=torch.float64, device=in0.device)
    hw = []

    def tap(k, x):
        _, h, w, c = x.shape
        hw.append(h * w)
        _lib.check(lib.forge_lpips_tap(_lib.ptr(x), N, h * w, c, _lib.ptr(P["lins"][k]), _lib.ptr(partial[k]), st), "forge_lpips_tap")
    mean, std = P["prep"][normalize]
    fp.trunk(in0, in1, P["layers"], mean, std, False, H, W, tap)
    out = torch.empty(N, dtype=torch.float32, device=in0.device)
    _lib.check(lib.forge_lpips_finalize(_lib.ptr(partial), N, *hw, _lib.ptr(out), st), "forge_lpips_finalize")
    return out


# ------------------------------------------------------------------------------------------------------------------------------------ protocol
def image_metrics(pred, gt, lpips=None):
    """{"psnr": [N] float64, "ssim": [N] float64, "lpips": [N] float32} of the pairs (pred[n], gt[n]) on the device, as the reference's evaluation
    scores a scene's novel views; "lpips" only when an LPIPS module is given (called as the reference does: lpips(pred, gt), normalize=False).
    No host synchronisation; everything runs on the current stream, so the call can be captured into a hipGraph."""
    out = {"psnr": psnr(pred, gt), "ssim": ssim(pred, gt)}
    if lpips is not None:
        out["lpips"] = lpips(pred, gt).view(-1)
    return out


def compute_img_metric(rgb, gt):
    """utils/eval_utils.py:compute_img_metric: (psnr, ssim) as Python floats of two HWC numpy images in [0, 1] (data_range 1), computed on the
    current device. The one place in the package that accepts host arrays."""
    a, b = np.asarray(rgb), np.asarray(gt)
    if a.ndim != 3 or a.shape != b.shape:
        raise ValueError("compute_img_metric: two HWC images of the same shape, got %s and %s" % (a.shape, b.shape))
    dev = torch.device("cuda", torch.cuda.current_device())
    x, y = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).permute(2, 0, 1)[None].to(dev) for v in (a, b))
    return float(psnr(x, y)[0]), float(ssim(x, y)[0])
