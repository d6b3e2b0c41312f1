"""The shape cases of the ConvGRU fusion parity matrix and the float64 reference it is measured against.

tests/test_gpu_convgru_matrix.py runs every fusion schedule of ConvGRU_3D over CASES; tests/test_convgru_paths_cpu.py checks, through the host
predicates of convops alone, that each case reaches the launch path and point-product form it is meant to (Case.expect). Both import this
module, so the table cannot drift between them.

A case's expectation (paths()):
  chunks      scene counts of the Winograd inference passes (fuse_hip / fuse_groups_hip, _eval_chunks); () = the direct kernel
  gates8      the gate point GEMMs (Cout = 2C) of a training step take the 8-plane form (wino_half_applies(R, 2C, C))
  state8      the state point GEMMs (Cout = C) take the 8-plane form (wino_half_applies(R, C, C))
  fc_wino     fusion_conv of the autograd path runs on the Winograd launches (wino_applies)
  wgrad_wino  (gate, state) weight gradients of the autograd cell on the Winograd wgrad (wino_wgrad_applies), else the direct kernel
  frozen_wino the frozen-weight forward (_FuseFrozen) on the Winograd launches
  node        fuse_groups_autograd_hip takes the hand-scheduled _FuseGroupsTrain node (else the per-step _GRUCellPreRows fallback)
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import forge_oracle as fo

T = 5                                                      # views per scene
PRODUCT_GROUPS = ((0, 1, 2), (3, 4), (0, 1, 2, 3, 4))      # model_single_pose_estimator.py: the three fusions of the pose3d step
EXTRA_GROUPS = ((2,), (4, 0, 2))                           # a single view; an out-of-order group (torch view mean, no nsum in wino_input)
ALL_GROUPS = PRODUCT_GROUPS + EXTRA_GROUPS

Case = namedtuple("Case", "name C b D H W groups small_limit expect")


def _exp(chunks, gates8, state8, fc_wino, wgrad_wino, frozen_wino, node):
    return dict(chunks=tuple(chunks), gates8=gates8, state8=state8, fc_wino=fc_wino, wgrad_wino=tuple(wgrad_wino), frozen_wino=frozen_wino, node=node)


# R = b D (H/2) (W/2) tile rows per point GEMM; the 8-plane form needs R >= 2048 and Cout > 64 (forge_wino_gemm_tile 'B')
CASES = [
    Case("a", 32, 2, 4, 16, 16, ALL_GROUPS, False, _exp([2], False, False, False, (False, False), True, False)),       # R 512: 16-plane, direct fc / wgrad
    Case("b", 64, 1, 8, 32, 32, ALL_GROUPS, False, _exp([1], True, False, True, (False, False), True, False)),          # R 2048: gates 8, state 16 (55b773a)
    Case("c", 96, 1, 6, 38, 38, ALL_GROUPS, False, _exp([1], True, True, True, (False, False), True, False)),           # R 2166: 8-plane, ragged rows / columns
    Case("d", 128, 1, 4, 16, 16, ALL_GROUPS, False, _exp([1], False, False, True, (True, True), True, True)),           # R 256: 16-plane at C 128
    Case("e", 128, 1, 8, 32, 32, ALL_GROUPS, False, _exp([1], True, True, True, (True, True), True, True)),         # R 2048: the product form
    Case("f", 160, 1, 8, 32, 32, ALL_GROUPS, False, _exp([1], True, True, True, (False, False), True, True)),       # node on 320 / 160 columns
    Case("g", 128, 1, 4, 16, 15, ALL_GROUPS, False, _exp([], False, False, False, (False, False), False, False)),      # odd W: direct everywhere
    Case("h", 128, 3, 4, 8, 8, ALL_GROUPS, True, _exp([2, 1], False, False, True, (True, True), False, False)),        # operand limit: chunks 2 + 1
]
CASE = {c.name: c for c in CASES}


def operand_limit(case):
    """MAX_OPERAND_BYTES of case h: two scenes' worth of the transformed views per Winograd point, so 3 scenes run as chunks of 2 and 1."""
    return 2 * T * case.D * (case.H // 2) * (case.W // 2) * case.C * 4


def paths(co, case):
    """What the host predicates of convops (co) choose for the case, in the vocabulary of Case.expect. The caller applies operand_limit()."""
    C, b, D, H, W = case.C, case.b, case.D, case.H, case.W
    R = b * D * (H // 2) * (W // 2)
    nb = co.wino_scene_chunk(b, D, H, W, C, views=T) if co.wino_enabled() else 0
    chunks = [min(nb, b - i) for i in range(0, b, nb)] if nb else []
    wino = co.wino_applies(co.TAPS_3x3x3, 1, b, D, H, W, C, C, C)
    return _exp(chunks, wino and co.wino_half_applies(R, 2 * C, C), wino and co.wino_half_applies(R, C, C),
                co.wino_applies(co.TAPS_3x3x3, 1, b, D, H, W, C, 0, C),
                (co.wino_wgrad_applies(b, D, H, W, C, C, 2 * C), co.wino_wgrad_applies(b, D, H, W, C, C, C)),
                co.wino_enabled() and co.wino_fits(b, D, H, W, C, views=T),
                co.wino_enabled() and co.wino_fits(b, D, H, W, 2 * C, views=T) and co.wino_wgrad_applies(b, D, H, W, C, 0, C))


# ------------------------------------------------------------------------------------------------------------ float64 reference
MOMENTUM = 0.1


def _bn(v, w, k, training, log):
    """nn.BatchNorm3d k of w on v; train mode logs (k, batch mean, unbiased batch variance) for the running statistics."""
    if training and log is not None:
        log.setdefault("stats", []).append((k, v.mean(dim=(0, 2, 3, 4)).detach(), v.var(dim=(0, 2, 3, 4), unbiased=True).detach()))
    return fo._bn(v, w, k, training)


def _cell_swapped(x, h, w, prefix):
    """fo.conv_gru_cell with the update and reset gates swapped (a deliberately wrong reference)."""
    hid = h.shape[1]
    g = F.conv3d(torch.cat([x, h], dim=1), w[prefix + ".conv_gate.weight"], w[prefix + ".conv_gate.bias"], padding=1)
    reset, update = torch.sigmoid(g[:, :hid]), torch.sigmoid(g[:, hid:])
    cand = torch.tanh(F.conv3d(torch.cat([x, h * reset], dim=1), w[prefix + ".out_gate.weight"], w[prefix + ".out_gate.bias"], padding=1))
    return h * (1 - update) + cand * update


def ref_fuse(x, w, training, h0=None, log=None, swap=False, slope=fo.LRELU, mean_div=None):
    """ConvGRU_3D fusion in the dtype of x (models/encoder.py:59-63, models/fusion.py:71-95; the same ops as forge_oracle.fuse):
    h0 = fusion_conv(mean_t x) unless given, one conv_gru_cell per view, fusion_norm. log (a dict) receives the LeakyReLU pre-activations of
    fusion_conv ("pre"), the view mean ("m", retaining its gradient when x requires one) and the train-mode batch statistics ("stats").
    swap / slope / mean_div: the deliberately wrong references (gates swapped, another LeakyReLU slope, the view sum divided by mean_div)."""
    log = {} if log is None else log
    if h0 is None:
        m = x.mean(dim=1) if mean_div is None else x.sum(dim=1) / mean_div
        if m.requires_grad:
            m.retain_grad()
        log["m"] = m
        h = m
        for i in (0, 3):
            h = _bn(F.conv3d(h, w["fusion_conv.%d.weight" % i], w["fusion_conv.%d.bias" % i], padding=1), w, "fusion_conv.%d" % (i + 1), training, log)
            log.setdefault("pre", []).append(h.detach())
            h = F.leaky_relu(h, slope)
        log["h0"] = h
    else:
        h = h0
    for t in range(x.shape[1]):
        h = _cell_swapped(x[:, t], h, w, "cells.0") if swap else fo.conv_gru_cell(x[:, t], h, w, "cells.0")
    return _bn(h, w, "fusion_norm", training, log)


def running_after(w, stats_seq):
    """{BN name: (running_mean, running_var)} after one momentum update per (name, mean, unbiased var) of stats_seq, in order."""
    out = {}
    for k, mean, var in stats_seq:
        rm, rv = out.get(k, (w[k + ".running_mean"].double(), w[k + ".running_var"].double()))
        out[k] = ((1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * var)
    return out


@torch.no_grad()
def pin_lrelu_signs(x, w, groups, window=1e-3):
    """Moves each channel's BatchNorm shift of fusion_conv.1 / .4 (float32 w, in place) by about `window` of the pre-activation scale at most,
    to the middle of the widest gap between the channel's pre-activation values (over every group, eval and train mode) near the seeded
    shift. A pre-activation within rounding distance of zero could take the other LeakyReLU slope in fp32 and move the gradients of its
    5^3 neighbourhood far beyond fp32 noise; after this no value lies near zero, and the references check that they have a margin
    (lrelu_margin). Returns the largest shift relative to the scale."""
    worst = 0.0
    x = x.double()
    wd = {k: v.double() for k, v in w.items()}
    for layer in (1, 4):
        us = []
        for g in groups:
            m = x[:, list(g)].mean(dim=1)
            for training in (False, True):
                h = m
                for i in (0, 3):
                    a = F.conv3d(h, wd["fusion_conv.%d.weight" % i], wd["fusion_conv.%d.bias" % i], padding=1)
                    u = fo._bn(a, dict(wd, **{"fusion_conv.%d.bias" % (i + 1): torch.zeros_like(wd["fusion_conv.%d.bias" % (i + 1)])}),
                               "fusion_conv.%d" % (i + 1), training)              # the normalised, scaled value before the shift
                    if i + 1 == layer:
                        us.append(u.transpose(0, 1).reshape(u.shape[1], -1))
                        break
                    h = F.leaky_relu(u + wd["fusion_conv.%d.bias" % (i + 1)].view(1, -1, 1, 1, 1), fo.LRELU)
        U = torch.cat(us, dim=1)
        scale = U.abs().max().item()
        key = "fusion_conv.%d.bias" % layer
        beta = wd[key].clone()
        for c in range(U.shape[0]):
            s = torch.sort(-U[c]).values                                  # v = u + beta is zero at beta = -u
            lo, hi = torch.searchsorted(s, beta[c] - window * scale).item(), torch.searchsorted(s, beta[c] + window * scale).item()
            lo, hi = max(lo - 1, 0), min(hi + 1, s.numel())
            seg = s[lo:hi]
            if seg.numel() < 2:
                continue
            j = torch.argmax(seg[1:] - seg[:-1]).item()
            beta[c] = 0.5 * (seg[j] + seg[j + 1])
        worst = max(worst, (beta - wd[key]).abs().max().item() / scale)
        w[key] = beta.float()
        wd[key] = w[key].double()
    return worst


def lrelu_margin(log):
    """min |v| / max |v| over the fusion_conv LeakyReLU pre-activations a reference logged."""
    return min(p.abs().min().item() / p.abs().max().item() for p in log["pre"])
