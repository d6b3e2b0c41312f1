"""VGG-16 perceptual loss of the training objective (models/perceptual_loss.py:7, `loss.perceptual_img` of every config/kubric/*.yaml) on the
MI355X HIP kernels.

    loss = sum over relu1_2, relu2_2, relu3_3, relu4_3 of F.l1_loss(vgg(prep(input)), vgg(prep(target)))     (only_deepest: relu4_3 alone)
    prep = repeat to 3 channels, (x - mean) / std, bilinear resize to 224^2 (align_corners = False)

The whole loss is ONE autograd node (_VGGLossFn). Forward runs input and target as one batch of 2N images:
  prep + conv1_1 patch rows   forge_vgg_prep_fwd (one launch), conv1_1 as a one-tap GEMM (forge_conv_igemm, ReLU epilogue)
  conv1_2 .. conv4_3          forge_wino_* with one depth tap (F(2x2, 3x3)) or forge_conv_igemm with 9 taps, per LAYER_PLAN; ReLU in the epilogue
  max-pool 2x2                forge_maxpool2d_nhwc
  L1 per tap                  forge_l1_partial: fixed-tree per-workgroup partial sums of |x - y|, added on the device in a fixed order
Backward (input branch only; the weights are frozen, so only data gradients):
  tap boundary                forge_vgg_tap_bwd: (maxpool2x2_bwd(g_next) + coef sign(x - y)) * (x > 0) in one pass
  ReLU inside a block         forge_affine_act_bwd (slope 0)
  data gradients              transposed Winograd weights (forge_wino_weights(transpose=1)) or negated taps on forge_conv_igemm; conv1_1 as a
                              Cout = 4 (3 padded) launch on the narrow kernel
  prep adjoint                forge_vgg_prep_bwd: deterministic gather per source pixel, / std, summed over the repeated channels
The forward walk (prep, conv1_1, the blocks with their pools) is `trunk`, shared with LPIPS (forge_amd/metrics.py), which runs it through block 5.
No atomics anywhere: two calls give bitwise-identical loss and gradient. Everything runs on the caller's current stream (a captured training
step stays a linear graph).

Deliberate deviations from the reference class (also in INTEGRATION.md):
  - `mean` / `std` stay Parameters with requires_grad=True (the reference's DDP wrap with find_unused_parameters=True keeps working) but are not
    inputs of the graph: they get no gradient. The reference computes one (through a second VGG backward over the targets) no optimiser uses.
  - the VGG weights have requires_grad=False. (The reference's `for p in bl: p.requires_grad = False` sets an attribute on the layer modules, so
    its weights do receive gradients - that no optimiser uses either.)
  - a `target` that requires grad raises ValueError instead of silently getting no gradient.
  - resize=False needs H and W to be multiples of 16 (three 2x2 pools and even extents for the Winograd tiles); otherwise ValueError.
  - host tensors raise RuntimeError, as everywhere in the package; C must be 1 or 3.

Weights are never downloaded: `weights=` (a path or a state dict in torchvision's `vgg16` layout `features.N.*`, or in this class's layout
`blocks.B.N.*`), else $FORGE_VGG16_WEIGHTS, else $TORCH_HOME/hub/checkpoints/vgg16-397923af.pth (the file torchvision's
`vgg16(pretrained=True)` caches). pretrained=False: seeded_vgg16_state_dict(seed), a CPU-only initialisation for tests and probes.
"""
import collections
import ctypes
import os

import torch
import torch.nn as nn

from . import _lib
from . import convops as co

# VGG-16 configuration D (Simonyan & Zisserman): features[:23] is what the loss uses (four blocks up to relu4_3), features[:30] what LPIPS uses
# (five blocks up to relu5_3, forge_amd/metrics.py)
VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
BLOCK_SLICES = ((0, 4), (4, 9), (9, 16), (16, 23))
TRUNK_SLICES = BLOCK_SLICES + ((23, 30),)
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # features index of each convolution inside features[:30]
BLOCK_CONVS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))  # CONV_IDX positions per block; the last one of each block is a tap
LAYER_NAMES = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2",
               "conv5_3")
WEIGHTS_FILE = "vgg16-397923af.pth"

# (forward, data gradient) of conv1_2 .. conv5_3: "wino" = F(2x2, 3x3) with one depth tap (forge_wino_input / _gemm / _output), "direct" =
# forge_conv_igemm with 9 taps. Chosen per layer from the A/B of tools/perceptual_probe.py at 10 and 40 pairs (DESIGN.md "VGG-16 perceptual loss",
# profiles/perceptual_probe.txt): the 64-channel layers at 224^2 / 112^2 are faster direct (K = 64 per Winograd point does not amortise the
# transforms), every layer from conv2_2 on is faster on Winograd. conv5_x (LPIPS only: forward only, at H/16) from the A/B of
# tools/metrics_probe.py (DESIGN.md "Evaluation metrics"). A layer whose extent is odd takes the 9-tap GEMM whatever its plan (convops.wino_fits).
LAYER_PLAN = {name: (("direct", "direct") if name in ("conv1_2", "conv2_1") else ("wino", "wino")) for name in LAYER_NAMES[1:]}


def vgg16_features():
    """nn.Sequential of VGG-16 configuration D's `features` (plain Conv2d / ReLU / MaxPool2d, torchvision's indices)."""
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


def seeded_vgg16_state_dict(seed=0):
    """The documented seeded initialisation (pretrained=False; tests, probes, tools/make_golden_perceptual.py): a pure CPU function of `seed`.
    torchvision layout `features.N.{weight,bias}` for all 13 convolutions of configuration D, in features order, from one torch.Generator:
    weight = randn * sqrt(2 / (9 Cin)) (He), bias = 0.05 randn, float32."""
    g = torch.Generator().manual_seed(int(seed))
    out, cin, i = collections.OrderedDict(), 3, 0
    for v in VGG16_CFG:
        if v == "M":
            i += 1
            continue
        out["features.%d.weight" % i] = torch.randn(v, cin, 3, 3, generator=g, dtype=torch.float32) * (2.0 / (9 * cin)) ** 0.5
        out["features.%d.bias" % i] = torch.randn(v, generator=g, dtype=torch.float32) * 0.05
        cin, i = v, i + 2
    return out


def default_weights_path():
    """$FORGE_VGG16_WEIGHTS, else $TORCH_HOME/hub/checkpoints/vgg16-397923af.pth if that file exists; FileNotFoundError naming both otherwise."""
    env = os.environ.get("FORGE_VGG16_WEIGHTS")
    if env and os.path.isfile(env):
        return env
    torch_home = os.environ.get("TORCH_HOME") or os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.expanduser("~/.cache"), "torch")
    cached = os.path.join(torch_home, "hub", "checkpoints", WEIGHTS_FILE)
    if os.path.isfile(cached):
        return cached
    raise FileNotFoundError("VGGPerceptualLoss(pretrained=True): no VGG-16 weights found. Looked for $FORGE_VGG16_WEIGHTS (%s) and %s. Copy "
                            "torchvision's %s there (nothing is downloaded), pass weights=, or use pretrained=False for the seeded "
                            "initialisation." % (env or "unset", cached, WEIGHTS_FILE))


def _ref_key(features_key):
    """'features.N.weight' -> 'blocks.B.N.weight' (N < 23), or None for layers the loss does not use."""
    _, n, leaf = features_key.split(".")
    n = int(n)
    for b, (lo, hi) in enumerate(BLOCK_SLICES):
        if lo <= n < hi:
            return "blocks.%d.%d.%s" % (b, n, leaf)
    return None


def pack_layers(convs, plan, device):
    """Launch arguments of the VGG convolutions `convs` (conv1_1 first): conv1_1's patch-row weight and its transposed Cout = 4 form, the 9-tap
    forms of the others (direct forward / data gradient) and their Winograd transforms where plan[i - 1] = (forward, data gradient) takes
    Winograd (a data gradient of None: forward only)."""
    layers = []
    for i, m in enumerate(convs):
        w = m.weight.detach().to(device=device, dtype=torch.float32)
        cout, cin = w.shape[:2]
        L = {"cin": cin, "cout": cout, "bias": m.bias.detach().to(device=device, dtype=torch.float32).contiguous(),
             "one": torch.ones(cout, device=device), "zero": torch.zeros(cout, device=device)}
        wp, _ = co.pack_conv2d_weight(w)                                          # [9][Cout][Cin], tap (ky, kx)
        if i == 0:
            L["w0"] = co.pad_cin(w.permute(0, 2, 3, 1).reshape(1, cout, 27).contiguous(), 32)      # patch-row order (ky, kx, c)
            L["wT"] = torch.nn.functional.pad(wp.transpose(1, 2), (0, 0, 0, 1)).contiguous()        # [9][4][64]: Cin 3 -> 4
        else:
            L["plan"] = plan[i - 1]
            L["wp"], L["wT"] = wp, wp.transpose(1, 2).contiguous()
            L["U"] = co.wino_pack_packed(wp) if plan[i - 1][0] == "wino" else None
            L["UT"] = co.wino_pack_packed(wp, transpose=True) if plan[i - 1][1] == "wino" else None
        layers.append(L)
    return layers


class VGGPerceptualLoss(co.PackedModule):
    """models/perceptual_loss.py:7 with the reference's state_dict layout (`blocks.{0..3}.N.{weight,bias}`, `mean`, `std`). See the module
    docstring for the kernels, the weight sources and the deliberate deviations."""

    def __init__(self, resize=True, pretrained=True, weights=None, seed=0):
        super().__init__()
        feats = vgg16_features()
        self.blocks = nn.ModuleList([feats[lo:hi].eval() for lo, hi in BLOCK_SLICES])
        for p in self.blocks.parameters():
            p.requires_grad_(False)
        self.mean = nn.Parameter(torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.std = nn.Parameter(torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self.resize = bool(resize)
        self.plan = dict(LAYER_PLAN)
        self._packed = co.PackCache()
        if weights is None:
            weights = default_weights_path() if pretrained else seeded_vgg16_state_dict(seed)
        self.load_vgg_weights(weights)

    def convs(self):
        """The ten nn.Conv2d of features[:23] in order (conv1_1 .. conv4_3)."""
        return [m for blk in self.blocks for m in blk if isinstance(m, nn.Conv2d)]

    def load_vgg_weights(self, weights):
        """Load VGG-16 weights from a path or a dict, in torchvision's layout (features.N.*; classifier.* and features beyond relu4_3 ignored)
        or in this class's (blocks.B.N.*, optionally with mean / std). Raises KeyError when a convolution is missing."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        sd = {}
        for k, v in weights.items():
            if k.startswith("features."):
                rk = _ref_key(k)
                if rk is not None:
                    sd[rk] = v
            elif k.startswith("blocks.") or k in ("mean", "std"):
                sd[k] = v
        own = self.state_dict()
        missing = [k for k in own if k not in sd and k not in ("mean", "std")]
        if missing:
            raise KeyError("VGG-16 weights lack %s" % ", ".join(missing))
        for k in ("mean", "std"):
            sd.setdefault(k, own[k])
        self.load_state_dict(sd, strict=True)

    # ---------------------------------------------------------------------------------------------------------------- packed weights
    def _pack(self, device):
        """Launch arguments of the ten convolutions (cached; rebuilt when a weight changed, on load_state_dict / .to() / train(), or when
        self.plan changed): conv1_1's patch-row weight and its transposed Cout = 4 form, the 9-tap forms of the others (direct forward / data
        gradient) and their Winograd transforms where the plan takes Winograd."""
        convs = self.convs()
        plan = tuple(self.plan[n] for n in LAYER_NAMES[1:len(convs)])
        if plan != self._plan_key:
            self._packed.clear()
            self._plan_key = plan
        return self._packed.get([p for m in convs for p in (m.weight, m.bias)], lambda: pack_layers(convs, plan, device))

    _plan_key = None

    # ---------------------------------------------------------------------------------------------------------------- forward
    def forward(self, input, target, only_deepest=False):
        for t in (input, target):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError("forge_amd ops need tensors on the MI355X (cuda/HIP device); got a %s. There is no CPU fallback."
                                   % (t.device if torch.is_tensor(t) else type(t).__name__))
        if not self.mean.is_cuda or self.mean.device != input.device:
            raise RuntimeError("VGGPerceptualLoss: move the module to the input's device (.to(%s)); there is no CPU fallback" % input.device)
        if input.dim() != 4 or input.shape != target.shape or input.shape[1] not in (1, 3):
            raise ValueError("VGGPerceptualLoss: input and target must be [N, 1 | 3, H, W] of the same shape, got %s and %s"
                             % (tuple(input.shape), tuple(target.shape)))
        if input.dtype != torch.float32 or target.dtype != torch.float32:
            raise TypeError("VGGPerceptualLoss: float32 images (got %s, %s)" % (input.dtype, target.dtype))
        if torch.is_grad_enabled() and target.requires_grad:
            raise ValueError("VGGPerceptualLoss: `target` requires grad; this implementation differentiates w.r.t. `input` only")
        H, W = input.shape[-2:]
        if not self.resize and (H % 16 or W % 16):
            raise ValueError("VGGPerceptualLoss(resize=False): H and W must be multiples of 16, got %dx%d" % (H, W))
        with torch.cuda.device(input.device):
            layers = self._pack(input.device)
            args = (layers, self.mean.detach(), self.std.detach(), self.resize, bool(only_deepest))
            if torch.is_grad_enabled() and input.requires_grad:
                return _VGGLossFn.apply(input, target, args)
            return _forward(input, target, *args, save=False)[0]


# -------------------------------------------------------------------------------------------------------------------- launches
def _conv(L, x, nb, H, W, out):
    """out [nb,H,W,Cout] = ReLU(conv3x3(x) + bias) on NHWC rows, per the layer's plan (the 9-tap GEMM when the Winograd operands would exceed
    the kernels' 32-bit buffer offsets)."""
    cin, cout = L["cin"], L["cout"]
    if L["U"] is not None and co.wino_fits(nb, 1, H, W, max(cin, cout)):
        V = co.wino_input(x, cin, cin, nb, 1, H, W)
        Mm = co.wino_gemm(V, cin, None, 0, L["U"], None, nb, 1, H // 2, W // 2, cout)
        return co.wino_output(Mm, L["bias"], L["one"], L["zero"], 0.0, None, None, None, out, None, None, nb, 1, H, W, cout, cout, co.EPI_AFFINE_ACT)
    return co.conv_igemm(x, cin, cin, None, 0, 0, L["wp"], L["bias"], L["one"], L["zero"], 0.0, None, None, None, out, None, (nb, 1, H, W), (1, H, W),
                         cout, cout, co.TAPS_3x3, epilogue=co.EPI_AFFINE_ACT)


_NEG_TAPS_3x3 = [(-a, -b, -c) for a, b, c in co.TAPS_3x3]


def _dgrad(L, d, nb, H, W):
    """dx [nb,H,W,Cin] = data gradient of the layer's convolution for the pre-activation gradient d [nb,H,W,Cout]."""
    cin, cout = L["cin"], L["cout"]
    dx = torch.empty(nb, H, W, cin, dtype=torch.float32, device=d.device)
    if L["UT"] is not None and co.wino_fits(nb, 1, H, W, max(cin, cout)):
        V = co.wino_input(d, cout, cout, nb, 1, H, W)
        Mm = co.wino_gemm(V, cout, None, 0, L["UT"], None, nb, 1, H // 2, W // 2, cin)
        return co.wino_output(Mm, None, None, None, 1.0, None, None, None, dx, None, None, nb, 1, H, W, cin, cin, co.EPI_BIAS)
    return co.conv_igemm(d, cout, cout, None, 0, 0, L["wT"], None, None, None, 1.0, None, None, None, dx, None, (nb, 1, H, W), (1, H, W), cin, cin,
                         _NEG_TAPS_3x3, epilogue=co.EPI_BIAS)
    return co.conv_igemm(d, cout, cout, None, 0, 0, wT, None, None, None, 1.0, None, None, None, dx, None, (nb, 1, H, W), (1, H, W), cin, cin,
                         _NEG_TAPS_3x3, epilogue=co.EPI_BIAS)


def _strides(t):
    return [int(s) for s in t.stride()]


def trunk(a, b, layers, mean, std, resize, Ho, Wo, tap):
    """The VGG-16 features of the batch [a; b] (2N images, [N, C, Hi, Wi] each): prep (forge_vgg_prep_fwd with the DEVICE scalars mean / std,
    resized to Ho x Wo when `resize`), conv1_1, then the blocks of BLOCK_CONVS whose convolutions `layers` holds (four for the loss's ten,
    five for LPIPS's thirteen), each after the first starting with the 2x2 max-pool. tap(block, x) is called on each block's last post-ReLU output [2N, H, W, C] as soon as it is written. Returns the
    post-ReLU output of every convolution. The caller makes the operands' device current."""
    lib, st = _lib.lib(), _lib.current_stream()
    N, C, Hi, Wi = a.shape
    dev = a.device
    nb = 2 * N
    rows = torch.empty(nb * Ho * Wo, 32, dtype=torch.float32, device=dev)
    _lib.check(lib.forge_vgg_prep_fwd(_lib.ptr(a), *_strides(a), _lib.ptr(b), *_strides(b), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(rows),
                                      N, C, Hi, Wi, Ho, Wo, int(resize), st), "forge_vgg_prep_fwd")
    L0 = layers[0]
    x = torch.empty(nb, Ho, Wo, 64, dtype=torch.float32, device=dev)
    co.conv_igemm(rows, 32, 32, None, 0, 0, L0["w0"], L0["bias"], L0["one"], L0["zero"], 0.0, None, None, None, x, None, (nb, 1, Ho, Wo), (1, Ho, Wo),
                  64, 64, [(0, 0, 0)], epilogue=co.EPI_AFFINE_ACT)
    acts = [x]
    H, W = Ho, Wo
    for blk, convs in enumerate(BLOCK_CONVS):
        if convs[-1] >= len(layers):
            break
        for j in convs:
            if j == 0:
                continue
            if j == convs[0]:                                       # a block after the first starts with the 2x2 max-pool
                Hp, Wp = H // 2, W // 2
                p = torch.empty(nb, Hp, Wp, x.shape[-1], dtype=torch.float32, device=dev)
                _lib.check(lib.forge_maxpool2d_nhwc(_lib.ptr(x), _lib.ptr(p), nb, H, W, x.shape[-1], 2, 2, 0, st), "forge_maxpool2d_nhwc")
                x, H, W = p, Hp, Wp
            out = torch.empty(nb, H, W, layers[j]["cout"], dtype=torch.float32, device=dev)
            x = _conv(layers[j], x, nb, H, W, out)
            acts.append(x)
        tap(blk, x)
    return acts


@_lib.on_tensor_device
def _forward(input, target, layers, mean, std, resize, only_deepest, save):
    """(loss, saved) for the batch [input; target]. saved (save=True): the input half of every convolution's post-ReLU output and the target half
    of every tap, as views of the 2N-image activations."""
    lib, st = _lib.lib(), _lib.current_stream()
    N, C, Hi, Wi = input.shape
    Ho, Wo = (224, 224) if resize else (Hi, Wi)
    nblk = lib.forge_l1_partial_blocks()
    partial = torch.empty(4, nblk, dtype=torch.float32, device=input.device)
    numel, taps = [], []

    def l1(b, x):
        half = x.numel() // 2
        numel.append(half)
        taps.append(x)
        if not only_deepest or b == 3:
            flat = x.reshape(-1)
            _lib.check(lib.forge_l1_partial(_lib.ptr(flat), ctypes.c_void_p(flat.data_ptr() + 4 * half), half, _lib.ptr(partial[b]), st), "forge_l1_partial")
    acts = trunk(input, target, layers, mean, std, resize, Ho, Wo, l1)
    if only_deepest:
        loss = partial[3].sum() / numel[3]
    else:
        loss = partial[0].sum() / numel[0]
        for b in range(1, 4):
            loss = loss + partial[b].sum() / numel[b]
    saved = None
    if save:
        saved = {"acts": [a[:N] for a in acts], "ytaps": [t[N:] for t in taps], "numel": numel, "shape": (N, C, Hi, Wi, Ho, Wo)}
    return loss, saved


@_lib.on_tensor_device
def _backward(gout, saved, layers, std, resize, only_deepest, din):
    lib, st = _lib.lib(), _lib.current_stream()
    N, C, Hi, Wi, Ho, Wo = saved["shape"]
    acts, ytaps, numel = saved["acts"], saved["ytaps"], saved["numel"]
    dev = gout.device
    g = None
    for b in (3, 2, 1, 0):
        convs = BLOCK_CONVS[b]
        x = acts[convs[-1]]
        _, H, W, Ct = x.shape
        coef = (gout / numel[b]).reshape(1) if (not only_deepest or b == 3) else None
        d = torch.empty_like(x)
        _lib.check(lib.forge_vgg_tap_bwd(_lib.ptr(x), _lib.ptr(ytaps[b]), _lib.ptr(g), _lib.ptr(coef), _lib.ptr(d), N, H, W, Ct, st), "forge_vgg_tap_bwd")
        for j in reversed(convs):
            if j == 0:
                L0 = layers[0]
                dimg = torch.empty(N, Ho, Wo, 4, dtype=torch.float32, device=dev)
                co.conv_igemm(d, 64, 64, None, 0, 0, L0["wT"], None, None, None, 1.0, None, None, None, dimg, None, (N, 1, Ho, Wo), (1, Ho, Wo), 4, 4,
                              _NEG_TAPS_3x3, epilogue=co.EPI_BIAS)
                _lib.check(lib.forge_vgg_prep_bwd(_lib.ptr(dimg), 4, _lib.ptr(std), _lib.ptr(din), *_strides(din), N, C, Hi, Wi, Ho, Wo, int(resize), st),
                           "forge_vgg_prep_bwd")
                break
            dx = _dgrad(layers[j], d, N, H, W)
            if j == convs[0]:
                g = dx
            else:
                d = torch.empty_like(dx)
                prev = acts[j - 1]
                C_ = dx.shape[-1]
                _lib.check(lib.forge_affine_act_bwd(_lib.ptr(dx), C_, _lib.ptr(prev), C_, None, 0.0, _lib.ptr(d), C_, dx.numel() // C_, C_, st),
                           "forge_affine_act_bwd")
    return din


class _VGGLossFn(torch.autograd.Function):
    """The whole perceptual loss as one node: d loss / d input only (see the module docstring)."""

    @staticmethod
    def forward(ctx, input, target, args):
        layers, mean, std, resize, only_deepest = args
        loss, saved = _forward(input, target, layers, mean, std, resize, only_deepest, save=True)
        ctx.saved = saved
        ctx.args = (layers, std, resize, only_deepest)
        # the input gradient is written with the input's own strides (a channels-last NCHW view stays channels-last); non-dense views get a dense one
        dense = input.is_contiguous() or input.is_contiguous(memory_format=torch.channels_last)
        ctx.din_spec = (tuple(input.shape), tuple(input.stride()) if dense else None, input.device)
        return loss

    @staticmethod
    def backward(ctx, gout):
        layers, std, resize, only_deepest = ctx.args
        shape, stride, dev = ctx.din_spec
        din = (torch.empty_strided(shape, stride, dtype=torch.float32, device=dev) if stride is not None
               else torch.empty(shape, dtype=torch.float32, device=dev))
        _backward(gout.detach().reshape(()).contiguous(), ctx.saved, layers, std, resize, only_deepest, din)
        ctx.saved = None
        return din, None, None
