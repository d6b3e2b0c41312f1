"""torch.autograd bindings of the HIP kernels in libforge_hip.so.

Host-side plumbing only: layout checks, output allocation, stream hand-off, autograd wiring.
All arithmetic of the hot path happens in forge_amd/csrc/*.hip. There is no CPU implementation
here: calling these ops with CPU tensors (or without the built library) raises.
"""
import math
import os

import torch

from . import _lib, determinism


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("forge_amd ops need tensors on the MI355X (cuda/HIP device); got a %s tensor. "
                               "There is no CPU fallback." % t.device)


def to_channels_last_3d(x):
    """[N,C,D,H,W] float32 -> same logical tensor whose memory is [N,D,H,W,C] (no copy if it already is)."""
    if x.dtype != torch.float32:
        raise TypeError("forge_amd ops are fp32 (got %s)" % x.dtype)
    if x.permute(0, 2, 3, 4, 1).is_contiguous():
        return x
    return x.contiguous(memory_format=torch.channels_last_3d)


def _empty_like_cl(x_cl):
    n, c, d, h, w = x_cl.shape
    return torch.empty((n, d, h, w, c), dtype=x_cl.dtype, device=x_cl.device).permute(0, 4, 1, 2, 3)


def _zeros_like_cl(x_cl):
    n, c, d, h, w = x_cl.shape
    return torch.zeros((n, d, h, w, c), dtype=x_cl.dtype, device=x_cl.device).permute(0, 4, 1, 2, 3)


class _RotateWarp(torch.autograd.Function):
    """forge_rotate_fwd / forge_rotate_bwd (models/rotate.py:127-141). slot (optional, int32 [n]): the warp stores view i at volume slot[i]
    (the view order of models/model.py:127-128 fused into the store, forge_rotate_fwd_slots) and the backward reads its gradient there."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, vox, xf, mode, slot=None):
        _require_cuda(vox, xf, mode)
        vox_cl = to_channels_last_3d(vox)
        n, C, D, H, W = vox_cl.shape
        xf_c = xf.detach().to(torch.float32).contiguous()
        out = _empty_like_cl(vox_cl)
        if slot is None:
            _lib.check(_lib.lib().forge_rotate_fwd(_lib.ptr(vox_cl), _lib.ptr(xf_c), _lib.ptr(mode), _lib.ptr(out),
                                                   n, C, D, H, W, _lib.current_stream()), "forge_rotate_fwd")
        else:
            _lib.check(_lib.lib().forge_rotate_fwd_slots(_lib.ptr(vox_cl), _lib.ptr(xf_c), _lib.ptr(mode), _lib.ptr(slot), _lib.ptr(out),
                                                         n, C, D, H, W, _lib.current_stream()), "forge_rotate_fwd_slots")
        ctx.save_for_backward(vox_cl, xf_c, mode, slot)
        return out

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, g):
        vox_cl, xf_c, mode, slot = ctx.saved_tensors
        n, C, D, H, W = vox_cl.shape
        dvox = _empty_like_cl(vox_cl) if ctx.needs_input_grad[0] else None     # written by the gather kernel; frozen volumes (refinement): skipped
        dxf = torch.zeros_like(xf_c) if ctx.needs_input_grad[1] else None
        if dvox is None and dxf is None:
            return None, None, None, None
        g_cl = to_channels_last_3d(g)
        # deterministic mode (forge_amd/determinism.py): the _det entries sum the pose gradient's per-workgroup partials in a fixed order
        if slot is None:
            determinism.launch("forge_rotate_bwd", (_lib.ptr(g_cl), _lib.ptr(vox_cl), _lib.ptr(xf_c), _lib.ptr(mode), _lib.ptr(dvox), _lib.ptr(dxf),
                                                    n, C, D, H, W), (n, C, D, H, W), g_cl.device)
        else:
            determinism.launch("forge_rotate_bwd_slots", (_lib.ptr(g_cl), _lib.ptr(vox_cl), _lib.ptr(xf_c), _lib.ptr(mode), _lib.ptr(slot),
                                                          _lib.ptr(dvox), _lib.ptr(dxf), n, C, D, H, W), (n, C, D, H, W), g_cl.device)
        return dvox, dxf, None, None


class _PoseChain(torch.autograd.Function):
    """forge_pose_chain_fwd / _bwd: the refinement loop's pose algebra (normalise, quaternion -> matrix, canonical @ rel, inverse, P_0 @ inverse,
    camera packing) as one launch forward (values + Jacobian by forward-mode differentiation) and one launch backward."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, rot, trans, can_p, can_e, K, half_extent, b, t):
        _require_cuda(rot, trans, can_p, can_e, K)
        dev = rot.device
        f32 = lambda x: x.detach().to(torch.float32).contiguous()
        rot_c, trans_c, Kc = f32(rot), f32(trans), f32(K).reshape(b * t, 9)
        if rot_c.shape != (b * (t - 1), 4) or trans_c.shape != (b * (t - 1), 3):
            raise ValueError("pose_chain: rot %s / trans %s do not match b=%d, t=%d" % (tuple(rot.shape), tuple(trans.shape), b, t))
        new = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        xf, cam, poses, origin, jac = new(b * t, 12), new(b * t, 16), new(b, t, 4, 4), new(b * t, 2), new(b * (t - 1), 24, 7)
        mode, slot = torch.empty(b * t, dtype=torch.int32, device=dev), torch.empty(b * t, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().forge_pose_chain_fwd(_lib.ptr(rot_c), _lib.ptr(trans_c), _lib.ptr(f32(can_p)), _lib.ptr(f32(can_e)), _lib.ptr(Kc), float(half_extent),
                                                   b, t, _lib.ptr(xf), _lib.ptr(mode), _lib.ptr(slot), _lib.ptr(cam), _lib.ptr(poses), _lib.ptr(origin),
                                                   _lib.ptr(jac), _lib.current_stream()), "forge_pose_chain_fwd")
        ctx.save_for_backward(jac)
        ctx.bt = (b, t)
        ctx.mark_non_differentiable(mode, slot, poses, origin)
        return xf, cam, mode, slot, poses, origin

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, dxf, dcam, _dmode, _dslot, _dposes, _dorigin):
        (jac,) = ctx.saved_tensors
        b, t = ctx.bt
        if dxf is None and dcam is None:
            return (None,) * 8
        c = lambda g: None if g is None else g.to(torch.float32).contiguous()
        dxf, dcam = c(dxf), c(dcam)
        drot = torch.empty(b * (t - 1), 4, dtype=torch.float32, device=jac.device)
        dtrans = torch.empty(b * (t - 1), 3, dtype=torch.float32, device=jac.device)
        _lib.check(_lib.lib().forge_pose_chain_bwd(_lib.ptr(jac), _lib.ptr(dxf), _lib.ptr(dcam), _lib.ptr(drot), _lib.ptr(dtrans), b, t, _lib.current_stream()),
                   "forge_pose_chain_bwd")
        return drot, dtrans, None, None, None, None, None, None


def pose_chain(rot, trans, can_p, can_e, K, half_extent, b, t):
    """rot [b(t-1),4] raw quaternions, trans [b(t-1),3], can_p / can_e [4,4], K [b,t,3,3] -> (xf [b t,12], cam [b t,16], mode [b t] int32,
    slot [b t] int32 (view i goes to volume slot[i]: the order of models/model.py:152-158), poses [b,t,4,4], origin [b t,2]); gradients reach
    rot / trans through xf (the warp) and cam (the ray-marcher)."""
    return _PoseChain.apply(rot, trans, can_p, can_e, K, half_extent, b, t)


def rotate_warp(vox, xf, mode, slot=None):
    """vox [n,C,D,H,W]; xf [n,12] 3x4 affine in normalised grid coords; mode [n] int32 (0 copy, 1 warp); slot [n] int32 (optional): view i is
    stored at volume slot[i]."""
    return _RotateWarp.apply(vox, xf, mode, slot)


class _RenderRays(torch.autograd.Function):
    """forge_render_fwd / forge_render_bwd (models/volume_render.py:53-63)."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, feat, dens, cam, view2vol, Hr, Wr, S, zmin, zmax, half, want_depth):
        _require_cuda(feat, dens, cam, view2vol)
        feat_cl = to_channels_last_3d(feat)
        nvol, C, D, H, W = feat_cl.shape
        if dens.shape != (nvol, 1, D, H, W):
            raise ValueError("density volume must be [%d,1,%d,%d,%d], got %s" % (nvol, D, H, W, tuple(dens.shape)))
        dens_c = dens.to(torch.float32).contiguous()
        cam_c = cam.detach().to(torch.float32).contiguous()
        V = cam_c.shape[0]
        out_feat = torch.empty((V, Hr, Wr, C), dtype=torch.float32, device=feat.device).permute(0, 3, 1, 2)   # NCHW view of NHWC memory
        out_opac = torch.empty((V, 1, Hr, Wr), dtype=torch.float32, device=feat.device)
        out_depth = torch.empty((V, 1, Hr, Wr), dtype=torch.float32, device=feat.device) if want_depth else None
        _lib.check(_lib.lib().forge_render_fwd(
            _lib.ptr(feat_cl), _lib.ptr(dens_c), _lib.ptr(cam_c), _lib.ptr(view2vol),
            _lib.ptr(out_feat), _lib.ptr(out_opac), _lib.ptr(out_depth),
            V, nvol, C, D, H, W, Hr, Wr, S, zmin, zmax, half[0], half[1], half[2], _lib.current_stream()),
            "forge_render_fwd")
        ctx.save_for_backward(feat_cl, dens_c, cam_c, view2vol)
        ctx.cfg = (Hr, Wr, S, zmin, zmax, half, want_depth)
        if want_depth:
            return out_feat, out_opac, out_depth
        return out_feat, out_opac

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, g_feat, g_opac, g_depth=None):
        feat_cl, dens_c, cam_c, view2vol = ctx.saved_tensors
        Hr, Wr, S, zmin, zmax, half, want_depth = ctx.cfg
        nvol, C, D, H, W = feat_cl.shape
        V = cam_c.shape[0]
        g_feat = g_feat.contiguous(memory_format=torch.channels_last)      # [V,Hr,Wr,C] in memory
        g_opac = g_opac.contiguous()
        g_depth = g_depth.contiguous() if (want_depth and g_depth is not None) else None
        # every element of dfeat / ddens / dcam is WRITTEN by the voxel-parallel gather (deterministic, no atomics): no zero-fills
        dfeat = _empty_like_cl(feat_cl)
        ddens = torch.empty_like(dens_c)
        dcam = torch.empty_like(cam_c) if ctx.needs_input_grad[2] else None        # pose refinement / joint training
        L = _lib.lib()
        ws_bytes = L.forge_render_bwd_ws_bytes(V, C, Hr, Wr, S, 0 if dcam is None else 1)
        if ws_bytes < 0:
            raise RuntimeError("forge_amd: forge_render_bwd_ws_bytes rejected V=%d C=%d Hr=%d Wr=%d S=%d" % (V, C, Hr, Wr, S))
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=feat_cl.device)   # per-sample (dL/dd_s, T_s d_s) of every ray: 8 V Hr Wr S bytes
        _lib.check(L.forge_render_bwd(
            _lib.ptr(feat_cl), _lib.ptr(dens_c), _lib.ptr(cam_c), _lib.ptr(view2vol),
            _lib.ptr(g_feat), _lib.ptr(g_opac), _lib.ptr(g_depth), _lib.ptr(dfeat), _lib.ptr(ddens), _lib.ptr(dcam),
            V, nvol, C, D, H, W, Hr, Wr, S, zmin, zmax, half[0], half[1], half[2], _lib.ptr(ws), ws_bytes, _lib.current_stream()),
            "forge_render_bwd")
        return (dfeat, ddens, dcam) + (None,) * 8


def render_rays(feat, dens, cam, view2vol, Hr, Wr, S, zmin, zmax, half, want_depth=False):
    """feat [nvol,C,D,H,W], dens [nvol,1,D,H,W], cam [V,16] (R9,T3,fx,fy,cx,cy at half res),
    view2vol [V] int32 -> (feat [V,C,Hr,Wr], opacity [V,1,Hr,Wr][, depth [V,1,Hr,Wr]])."""
    return _RenderRays.apply(feat, dens, cam, view2vol, int(Hr), int(Wr), int(S), float(zmin), float(zmax),
                             tuple(float(h) for h in half), bool(want_depth))


class _ResizeBilinear(torch.autograd.Function):
    """forge_resize_bilinear_fwd / _bwd: planes [..., Hi, Wi] -> [..., Ho, Wo], bilinear, align_corners=False (models/volume_render.py:69,74)."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, x, Ho, Wo):
        _require_cuda(x)
        if x.dtype != torch.float32:
            raise TypeError("forge_amd ops are fp32 (got %s)" % x.dtype)
        xc = x.contiguous()
        Hi, Wi = xc.shape[-2:]
        P = xc.numel() // (Hi * Wi)
        out = torch.empty(xc.shape[:-2] + (Ho, Wo), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().forge_resize_bilinear_fwd(_lib.ptr(xc), _lib.ptr(out), P, Hi, Wi, Ho, Wo, _lib.current_stream()), "forge_resize_bilinear_fwd")
        ctx.dims = (P, Hi, Wi, Ho, Wo, tuple(x.shape))
        return out

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, g):
        P, Hi, Wi, Ho, Wo, shape = ctx.dims
        gc = g.contiguous()
        din = torch.empty(shape, dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().forge_resize_bilinear_bwd(_lib.ptr(gc), _lib.ptr(din), P, Hi, Wi, Ho, Wo, _lib.current_stream()), "forge_resize_bilinear_bwd")
        return din, None, None


def resize_bilinear(x, Ho, Wo):
    """F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=False) on the HIP kernels (forward and adjoint)."""
    return _ResizeBilinear.apply(x, int(Ho), int(Wo))


def attention_applies(q, k, v):
    """forge_attention_fwd's domain: fp32 on the MI355X, no autograd graph wanted, one head of 64 channels, token counts multiples of 64,
    q / k [B,N,64] and v [B,Nk,64] or [1,Nk,64] (shared)."""
    return (q.is_cuda and k.device == q.device and v.device == q.device                 # raw pointers go to the kernel: all three on q's HIP device
            and q.dtype == torch.float32 and k.dtype == torch.float32 and v.dtype == torch.float32 and not torch.is_grad_enabled()
            and q.dim() == 3 and k.dim() == 3 and v.dim() == 3 and q.shape[-1] == 64 and k.shape[-1] == 64 and v.shape[-1] == 64
            and q.shape[0] == k.shape[0] and v.shape[0] in (1, q.shape[0]) and v.shape[1] == k.shape[1]
            and q.shape[1] % 64 == 0 and k.shape[1] % 64 == 0 and q.shape[1] > 0 and k.shape[1] > 0)


@_lib.on_tensor_device
def attention(q, k, v):
    """softmax(q k^T) v for one head (models/model_utils.py:207-229, unscaled) without materialising the [B,Nq,Nk] matrix: forge_attention_fwd.
    q [B,Nq,64], k [B,Nk,64], v [B,Nk,64] or [1,Nk,64] (one value table for every batch element) -> [B,Nq,64]. Inference only (no autograd node)."""
    if not attention_applies(q, k, v):
        raise RuntimeError("forge_amd: ops.attention needs fp32 [B,N,64] tensors on the MI355X with token counts that are multiples of 64, outside autograd "
                           "(got q %s, k %s, v %s, grad mode %s)" % (tuple(q.shape), tuple(k.shape), tuple(v.shape), torch.is_grad_enabled()))
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    B, Nq, d = q.shape
    Nk = k.shape[1]
    out = torch.empty(B, Nq, d, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().forge_attention_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 0 if v.shape[0] == 1 and B > 1 else Nk, _lib.ptr(out), B, Nq, Nk, d,
                                              _lib.current_stream()), "forge_attention_fwd")
    return out


# ---- differentiable attention (training), opt-in: forge_attention_fwd_lse / forge_attention_bwd. Off by default - with the switch off nothing
# in the package calls the two entry points and every training attention stays on torch's differentiable ops, bit for bit as before.
_attention_training = os.environ.get("FORGE_ATTENTION_TRAIN", "0") == "1"          # read once, at import


def set_attention_training(flag):
    """True: attentions inside an autograd graph run ops.attention_train (where attention_train_applies holds); False (the default, or
    FORGE_ATTENTION_TRAIN unset at import): they keep torch's matmul - softmax - matmul. Returns the previous setting."""
    global _attention_training
    if not isinstance(flag, bool):
        raise TypeError("set_attention_training takes True or False (got %r)" % (flag,))
    prev, _attention_training = _attention_training, flag
    return prev


def attention_training():
    """The current setting of set_attention_training()."""
    return _attention_training


def _attention_train_domain(q, k, v):
    """attention_applies' shape / dtype / device rules without its grad-mode clause, plus: a value table shared by the batch (v [1,Nk,64], B > 1)
    is a constant - forge_attention_bwd does not sum a gradient over the batch for it."""
    return (q.is_cuda and k.device == q.device and v.device == q.device
            and q.dtype == torch.float32 and k.dtype == torch.float32 and v.dtype == torch.float32
            and q.dim() == 3 and k.dim() == 3 and v.dim() == 3 and q.shape[-1] == 64 and k.shape[-1] == 64 and v.shape[-1] == 64
            and q.shape[0] == k.shape[0] and v.shape[0] in (1, q.shape[0]) and v.shape[1] == k.shape[1]
            and q.shape[1] % 64 == 0 and k.shape[1] % 64 == 0 and q.shape[1] > 0 and k.shape[1] > 0
            and not (v.shape[0] == 1 and q.shape[0] > 1 and v.requires_grad))


def attention_train_applies(q, k, v):
    """ops.attention_train's domain, and the switch (set_attention_training / FORGE_ATTENTION_TRAIN=1) is on."""
    return _attention_training and _attention_train_domain(q, k, v)


class _AttentionTrain(torch.autograd.Function):
    """forge_attention_fwd_lse / forge_attention_bwd: saved for backward are q, k, v, out and lse [B,Nq] - never a [B,Nq,Nk] matrix."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, q, k, v):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Nq, d = q.shape
        Nk = k.shape[1]
        out = torch.empty(B, Nq, d, dtype=torch.float32, device=q.device)
        lse = torch.empty(B, Nq, dtype=torch.float32, device=q.device)
        ctx.v_rows = 0 if v.shape[0] == 1 and B > 1 else Nk
        _lib.check(_lib.lib().forge_attention_fwd_lse(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ctx.v_rows, _lib.ptr(out), _lib.ptr(lse), B, Nq, Nk, d,
                                                      _lib.current_stream()), "forge_attention_fwd_lse")
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        B, Nq, d = q.shape
        Nk = k.shape[1]
        dout = dout.contiguous()
        dq, dk = torch.empty_like(q), torch.empty_like(k)                       # written in full by the kernels: no zero-fills
        dv = torch.empty_like(v) if ctx.needs_input_grad[2] and ctx.v_rows else None
        delta = torch.empty(B, Nq, dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().forge_attention_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ctx.v_rows, _lib.ptr(out), _lib.ptr(lse), _lib.ptr(dout),
                                                  _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(delta), B, Nq, Nk, d, _lib.current_stream()),
                   "forge_attention_bwd")
        return dq, dk, dv


def attention_train(q, k, v):
    """ops.attention inside an autograd graph: softmax(q k^T) v (same kernel, same bits) with a HIP backward that recomputes the softmax from the
    saved log-sum-exp - no [B,Nq,Nk] matrix forward or backward, no atomics (bitwise reproducible). q [B,Nq,64], k [B,Nk,64], v [B,Nk,64] or a
    constant [1,Nk,64] shared by the batch. Independent of the switch (that gates attention_train_applies, the models' dispatch); outside the
    domain it raises."""
    if not _attention_train_domain(q, k, v):
        raise RuntimeError("forge_amd: ops.attention_train needs fp32 [B,N,64] tensors on the MI355X with token counts that are multiples of 64, and a "
                           "value table shared by the batch must not require grad (got q %s, k %s, v %s%s)"
                           % (tuple(q.shape), tuple(k.shape), tuple(v.shape), ", v.requires_grad" if v.requires_grad else ""))
    return _AttentionTrain.apply(q, k, v)


# ---- multi-head attention (the 2-D pose estimator's six blocks), opt-in: forge_attention_mh_fwd / forge_attention_mh_bwd. Off by default - with
# the switch off nothing in the package calls the two entry points and MultiHeadAttention runs torch's bmm - softmax - bmm, bit for bit as before.
# Independent of set_attention_training (which keeps its meaning: the single-head attentions of the 3-D estimator inside an autograd graph).
_multihead_attention = os.environ.get("FORGE_ATTENTION_MH", "0") == "1"            # read once, at import


def set_multihead_attention(flag):
    """True: MultiHeadAttention (forge_amd/pose_estimator_2d.py) runs ops.attention_mh / ops.attention_mh_train where attention_mh_applies holds;
    False (the default, or FORGE_ATTENTION_MH unset at import): it keeps torch's head split - bmm - softmax - bmm - head merge. Returns the
    previous setting."""
    global _multihead_attention
    if not isinstance(flag, bool):
        raise TypeError("set_multihead_attention takes True or False (got %r)" % (flag,))
    prev, _multihead_attention = _multihead_attention, flag
    return prev


def multihead_attention():
    """The current setting of set_multihead_attention()."""
    return _multihead_attention


def _mh_strides(t):
    """(batch stride, row stride) in floats as the kernels take them: a batch of one has no batch stride (torch reports an arbitrary one)."""
    return (0 if t.shape[0] == 1 else t.stride(0)), t.stride(1)


def _attention_mh_domain(q, k, v, num_heads):
    """The domain of forge_attention_mh_fwd / _bwd: fp32 q [B,Nq,H*64], k / v [B,Nk,H*64] on one HIP device, channel stride 1, the other strides
    multiples of 4 floats and the storage 16-byte aligned (float4 access), token counts multiples of 64."""
    if not (isinstance(num_heads, int) and not isinstance(num_heads, bool) and num_heads >= 1):
        return False
    if not all(torch.is_tensor(t) and t.dim() == 3 and t.is_cuda and t.dtype == torch.float32 and t.device == q.device and t.shape[-1] == 64 * num_heads
               for t in (q, k, v)):
        return False
    if not (q.shape[0] == k.shape[0] == v.shape[0] and k.shape[1] == v.shape[1] and q.shape[0] > 0
            and q.shape[1] > 0 and k.shape[1] > 0 and q.shape[1] % 64 == 0 and k.shape[1] % 64 == 0):
        return False
    return all(t.stride(2) == 1 and t.data_ptr() % 16 == 0 and all(s >= 0 and s % 4 == 0 for s in _mh_strides(t)) for t in (q, k, v))


def attention_mh_applies(q, k, v, num_heads, pad_mask=None, attn_mask=None, dropout_p=0.0, training=False):
    """The dispatch predicate of MultiHeadAttention: the switch (set_multihead_attention / FORGE_ATTENTION_MH=1) is on, q / k / v are in the
    kernels' domain (fp32 HIP tensors on one device, heads of 64 channels, token counts multiples of 64, float4-addressable strides), there is no
    key-padding mask and no attention mask, and dropout is inactive (p == 0, or the module is in eval mode)."""
    return (_multihead_attention and pad_mask is None and attn_mask is None and (dropout_p == 0 or not training)
            and _attention_mh_domain(q, k, v, num_heads))


def _mh_check(what, q, k, v, num_heads, scale):
    if (_attention_mh_domain(q, k, v, num_heads) and isinstance(scale, (int, float)) and not isinstance(scale, bool)
            and math.isfinite(scale) and scale > 0):
        return
    desc = lambda t: "%s %s strides %s %s" % (tuple(t.shape), str(t.dtype).replace("torch.", ""), tuple(t.stride()), t.device) if torch.is_tensor(t) else repr(t)
    raise RuntimeError("forge_amd: ops.%s needs fp32 q [B,Nq,H*64] and k, v [B,Nk,H*64] on the MI355X with heads of 64 channels, token counts that are "
                       "multiples of 64, channel stride 1, the other strides multiples of 4 floats, 16-byte aligned storage and a finite positive scale "
                       "(got num_heads %r, scale %r, q %s, k %s, v %s)" % (what, num_heads, scale, desc(q), desc(k), desc(v)))


def _mh_forward(q, k, v, num_heads, scale, want_lse):
    B, Nq, C = q.shape
    Nk = k.shape[1]
    out = torch.empty(B, Nq, C, dtype=torch.float32, device=q.device)
    lse = torch.empty(B, num_heads, Nq, dtype=torch.float32, device=q.device) if want_lse else None
    _lib.check(_lib.lib().forge_attention_mh_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), _lib.ptr(lse), B, num_heads, Nq, Nk, 64,
                                                 *_mh_strides(q), *_mh_strides(k), *_mh_strides(v), *_mh_strides(out), scale, _lib.current_stream()),
               "forge_attention_mh_fwd")
    return out, lse


@_lib.on_tensor_device
def attention_mh(q, k, v, num_heads, scale):
    """softmax(scale q_h k_h^T) v_h for every head h, heads side by side in the channels as the q / k / v projections write them and o_proj reads
    them: q [B,Nq,H*64], k / v [B,Nk,H*64] -> [B,Nq,H*64], without the head-split and head-merge copies and without the [B*H,Nq,Nk] matrix
    (forge_attention_mh_fwd). Strided views (slices of a wider projection) are taken as they are. Inference only (no autograd node); independent of
    the switch (that gates attention_mh_applies, the module's dispatch); outside the domain it raises."""
    _mh_check("attention_mh", q, k, v, num_heads, scale)
    return _mh_forward(q.detach(), k.detach(), v.detach(), num_heads, float(scale), False)[0]


class _AttentionMHTrain(torch.autograd.Function):
    """forge_attention_mh_fwd (with lse) / forge_attention_mh_bwd: saved for backward are q, k, v (as they came: views stay views), out and
    lse [B,H,Nq] - never a [B*H,Nq,Nk] matrix."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, q, k, v, num_heads, scale):
        out, lse = _mh_forward(q, k, v, num_heads, scale, True)
        ctx.num_heads, ctx.scale = num_heads, scale
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        B, Nq, C = q.shape
        Nk, H = k.shape[1], ctx.num_heads
        dout = dout.contiguous()
        mk = lambda n: torch.empty(B, n, C, dtype=torch.float32, device=q.device)     # dense, written in full by the kernels: no zero-fills
        dq, dk = mk(Nq), mk(Nk)
        dv = mk(Nk) if ctx.needs_input_grad[2] else None
        delta = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().forge_attention_mh_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(dout), _lib.ptr(dq),
                                                     _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(delta), B, H, Nq, Nk, 64, *_mh_strides(q), *_mh_strides(k),
                                                     *_mh_strides(v), *_mh_strides(out), ctx.scale, _lib.current_stream()), "forge_attention_mh_bwd")
        return dq, dk, dv, None, None


def attention_mh_train(q, k, v, num_heads, scale):
    """ops.attention_mh inside an autograd graph (same kernel, same bits) with a HIP backward that recomputes the softmax from the saved
    log-sum-exp: no [B*H,Nq,Nk] matrix forward or backward, no atomics (bitwise reproducible). Independent of the switch; outside the domain it
    raises."""
    _mh_check("attention_mh_train", q, k, v, num_heads, scale)
    return _AttentionMHTrain.apply(q, k, v, num_heads, float(scale))
