"""torch.autograd bindings of the HIP kernels in libforge_hip.so.

Host-side plumbing only: layout checks, output allocation, stream hand-off, autograd wiring.
All arithmetic of the hot path happens in forge_amd/csrc/*.hip. There is no CPU implementation
here: calling these ops with CPU tensors (or without the built library) raises.
"""
import ctypes
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
        ws_bytes = _lib.size_query("forge_render_bwd_ws_bytes", V, C, Hr, Wr, S, 0 if dcam is None else 1)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=feat_cl.device)   # per-sample (dL/dd_s, T_s d_s) of every ray: 8 V Hr Wr S bytes
        _lib.check(_lib.lib().forge_render_bwd(
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


class _Switch:
    """An opt-in path: off unless `env` is "1" (read once, at import) or the public function named `setter` turned it on."""

    def __init__(self, env, setter):
        self.on, self.setter = os.environ.get(env, "0") == "1", setter

    def set(self, flag):
        if not isinstance(flag, bool):
            raise TypeError("%s takes True or False (got %r)" % (self.setter, flag))
        prev, self.on = self.on, flag
        return prev


def _finite_scalar(x, lo, strict):
    """x is a finite int or float (never a bool), above lo (strict) or at least lo."""
    return isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x) and (x > lo if strict else x >= lo)


def _tensor_desc(t):
    """A tensor as this family's error messages show it; anything else by its repr."""
    return "%s %s strides %s %s" % (tuple(t.shape), str(t.dtype).replace("torch.", ""), tuple(t.stride()), t.device) if torch.is_tensor(t) else repr(t)


def _empty_f32(dev, *shape):
    """An fp32 tensor that a kernel writes in full: no zero-fill."""
    return torch.empty(*shape, dtype=torch.float32, device=dev)


def _bwd_workspace(query, dev, *args):
    """(workspace, its byte count) of a backward entry, sized by the entry's host size query; never an empty allocation."""
    nbytes = _lib.size_query(query, *args)
    return _empty_f32(dev, max(nbytes // 4, 4)), nbytes


def _attention_domain(q, k, v):
    """What forge_attention_fwd / _fwd_lse / _bwd take (attention_applies' docstring), whatever the grad mode."""
    return (q.is_cuda and k.device == q.device and v.device == q.device                 # raw pointers go to the kernel: all three on q's HIP device
            and q.dtype == torch.float32 and k.dtype == torch.float32 and v.dtype == torch.float32
            and q.dim() == 3 and k.dim() == 3 and v.dim() == 3 and q.shape[-1] == 64 and k.shape[-1] == 64 and v.shape[-1] == 64
            and q.shape[0] == k.shape[0] and v.shape[0] in (1, q.shape[0]) and v.shape[1] == k.shape[1]
            and q.shape[1] % 64 == 0 and k.shape[1] % 64 == 0 and q.shape[1] > 0 and k.shape[1] > 0)


def attention_applies(q, k, v):
    """forge_attention_fwd's domain: fp32 on the MI355X, no autograd graph wanted, one head of 64 channels, token counts multiples of 64,
    q / k [B,N,64] and v [B,Nk,64] or [1,Nk,64] (shared)."""
    return _attention_domain(q, k, v) and not torch.is_grad_enabled()


def _sh_forward(q, k, v, want_lse):
    """One forge_attention_fwd launch, or with want_lse one forge_attention_fwd_lse launch. Returns (out, lse or None, the contiguous operands,
    v_rows): v_rows is the kernels' batch stride of v in rows, 0 for a value table shared by the batch."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    B, Nq, d = q.shape
    Nk = k.shape[1]
    v_rows = 0 if v.shape[0] == 1 and B > 1 else Nk
    out = _empty_f32(q.device, B, Nq, d)
    lse = _empty_f32(q.device, B, Nq) if want_lse else None
    entry, outs = ("forge_attention_fwd_lse", (_lib.ptr(out), _lib.ptr(lse))) if want_lse else ("forge_attention_fwd", (_lib.ptr(out),))
    _lib.check(getattr(_lib.lib(), entry)(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), v_rows, *outs, B, Nq, Nk, d, _lib.current_stream()), entry)
    return out, lse, (q, k, v), v_rows


@_lib.on_tensor_device
def attention(q, k, v):
    """softmax(q k^T) v for one head (models/model_utils.py:207-229, unscaled) without materialising the [B,Nq,Nk] matrix: forge_attention_fwd.
    q [B,Nq,64], k [B,Nk,64], v [B,Nk,64] or [1,Nk,64] (one value table for every batch element) -> [B,Nq,64]. Inference only (no autograd node)."""
    if not attention_applies(q, k, v):
        raise RuntimeError("forge_amd: ops.attention needs fp32 [B,N,64] tensors on the MI355X with token counts that are multiples of 64, outside autograd "
                           "(got q %s, k %s, v %s, grad mode %s)" % (tuple(q.shape), tuple(k.shape), tuple(v.shape), torch.is_grad_enabled()))
    return _sh_forward(q, k, v, False)[0]


# ---- differentiable attention (training), opt-in: forge_attention_fwd_lse / forge_attention_bwd. Off by default - with the switch off nothing
# in the package calls the two entry points and every training attention stays on torch's differentiable ops, bit for bit as before.
_attention_training = _Switch("FORGE_ATTENTION_TRAIN", "set_attention_training")


def set_attention_training(flag):
    """True: attentions inside an autograd graph run ops.attention_train (where attention_train_applies holds); False (the default, or
    FORGE_ATTENTION_TRAIN unset at import): they keep torch's matmul - softmax - matmul. Returns the previous setting."""
    return _attention_training.set(flag)


def attention_training():
    """The current setting of set_attention_training()."""
    return _attention_training.on


def _attention_train_domain(q, k, v):
    """_attention_domain, plus: a value table shared by the batch (v [1,Nk,64], B > 1) is a constant - forge_attention_bwd does not sum a
    gradient over the batch for it."""
    return _attention_domain(q, k, v) and not (v.shape[0] == 1 and q.shape[0] > 1 and v.requires_grad)


def attention_train_applies(q, k, v):
    """ops.attention_train's domain, and the switch (set_attention_training / FORGE_ATTENTION_TRAIN=1) is on."""
    return _attention_training.on and _attention_train_domain(q, k, v)


class _AttentionTrain(torch.autograd.Function):
    """forge_attention_fwd_lse / forge_attention_bwd: saved for backward are q, k, v, out and lse [B,Nq] - never a [B,Nq,Nk] matrix."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, q, k, v):
        out, lse, qkv, ctx.v_rows = _sh_forward(q, k, v, True)
        ctx.save_for_backward(*qkv, out, lse)
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
        delta = _empty_f32(q.device, B, Nq)
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
_multihead_attention = _Switch("FORGE_ATTENTION_MH", "set_multihead_attention")


def set_multihead_attention(flag):
    """True: MultiHeadAttention (forge_amd/pose_estimator_2d.py) runs ops.attention_mh / ops.attention_mh_train where attention_mh_applies holds;
    False (the default, or FORGE_ATTENTION_MH unset at import): it keeps torch's head split - bmm - softmax - bmm - head merge. Returns the
    previous setting."""
    return _multihead_attention.set(flag)


def multihead_attention():
    """The current setting of set_multihead_attention()."""
    return _multihead_attention.on


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
    return (_multihead_attention.on and pad_mask is None and attn_mask is None and (dropout_p == 0 or not training)
            and _attention_mh_domain(q, k, v, num_heads))


def _mh_check(what, q, k, v, num_heads, scale):
    if _attention_mh_domain(q, k, v, num_heads) and _finite_scalar(scale, 0, True):
        return
    raise RuntimeError("forge_amd: ops.%s needs fp32 q [B,Nq,H*64] and k, v [B,Nk,H*64] on the MI355X with heads of 64 channels, token counts that are "
                       "multiples of 64, channel stride 1, the other strides multiples of 4 floats, 16-byte aligned storage and a finite positive scale "
                       "(got num_heads %r, scale %r, q %s, k %s, v %s)" % (what, num_heads, scale, _tensor_desc(q), _tensor_desc(k), _tensor_desc(v)))


def _mh_forward(q, k, v, num_heads, scale, want_lse):
    B, Nq, C = q.shape
    Nk = k.shape[1]
    out = _empty_f32(q.device, B, Nq, C)
    lse = _empty_f32(q.device, B, num_heads, Nq) if want_lse else None
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
        dq, dk = _empty_f32(q.device, B, Nq, C), _empty_f32(q.device, B, Nk, C)          # dense, written in full by the kernels: no zero-fills
        dv = _empty_f32(q.device, B, Nk, C) if ctx.needs_input_grad[2] else None
        delta = _empty_f32(q.device, B, H, Nq)
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


# ---- token-row layers (LayerNorm / Linear / GELU around the attention kernels of both pose estimators), opt-in: forge_token_linear_fwd / _bwd,
# forge_layer_norm_fwd / _bwd (csrc/token.hip). Off by default - with the switch off nothing in the package calls the entry points and the blocks
# run nn.LayerNorm / nn.Linear / nn.GELU, bit for bit as before. Independent of set_attention_training and set_multihead_attention.
_token_layers = _Switch("FORGE_TOKEN_LAYERS", "set_token_layers")


def set_token_layers(flag):
    """True: the transformer blocks of both pose estimators run their LayerNorm / Linear / GELU chains on ops.token_linear / ops.layer_norm where
    token_layers_applies holds; False (the default, or FORGE_TOKEN_LAYERS unset at import): they keep torch's modules. Returns the previous setting."""
    return _token_layers.set(flag)


def token_layers():
    """The current setting of set_token_layers()."""
    return _token_layers.on


TOKEN_MAX_CHANNELS, TOKEN_MAX_LN_CHANNELS = 1024, 256


def _token_rows(t):
    """(rows view [R,C], row stride in floats) of a [..., C] tensor whose leading dimensions collapse into one row stride, or None."""
    if not (torch.is_tensor(t) and t.dim() >= 2 and t.is_cuda and t.dtype == torch.float32 and t.stride(-1) == 1 and t.numel() > 0):
        return None
    try:
        v = t.view(-1, t.shape[-1])
    except RuntimeError:
        return None
    ld = v.stride(0) if v.shape[0] > 1 else v.shape[1]
    if ld % 4 or ld < v.shape[1] or v.data_ptr() % 16 or v.shape[0] >= 1 << 31:
        return None
    return v, ld


def _token_vec(t, n, dev):
    return torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.shape == (n,) and t.is_contiguous() and t.data_ptr() % 16 == 0


def _layer_norm_domain(x, gamma, beta, eps):
    rows = _token_rows(x)
    if rows is None:
        return False
    K = x.shape[-1]
    return (K % 64 == 0 and 64 <= K <= TOKEN_MAX_LN_CHANNELS and _token_vec(gamma, K, x.device) and _token_vec(beta, K, x.device)
            and _finite_scalar(eps, 0, False))


def _token_domain(x, weight, bias=None, ln=None, act=None, residual=None):
    """The domain of forge_token_linear_fwd / _bwd: fp32 x [...,K] on a HIP device with channel stride 1, leading dimensions that collapse into one
    row stride (a multiple of 4 floats), 16-byte aligned storage; weight [N,K] contiguous; K and N multiples of 64 up to 1024 (K <= 256 under a
    LayerNorm prologue ln = (gamma, beta, eps)); act None or "gelu"; bias [N]; residual [...,N] addressed like x."""
    if _token_rows(x) is None or act not in (None, "gelu"):
        return False
    K, dev = x.shape[-1], x.device
    if not (torch.is_tensor(weight) and weight.dim() == 2 and weight.is_cuda and weight.device == dev and weight.dtype == torch.float32
            and weight.shape[1] == K and weight.is_contiguous() and weight.data_ptr() % 16 == 0):
        return False
    N = weight.shape[0]
    if K % 64 or N % 64 or not (64 <= K <= TOKEN_MAX_CHANNELS and 64 <= N <= TOKEN_MAX_CHANNELS):
        return False
    if bias is not None and not _token_vec(bias, N, dev):
        return False
    if ln is not None and not (isinstance(ln, (tuple, list)) and len(ln) == 3 and _layer_norm_domain(x, *ln)):
        return False
    if residual is not None and not (_token_rows(residual) is not None and residual.device == dev and residual.shape == x.shape[:-1] + (N,)):
        return False
    return True


def token_layers_applies(x, weight=None, bias=None, ln=None, act=None, residual=None, dropout_p=0.0, training=False):
    """The dispatch predicate of the pose estimators' blocks: the switch (set_token_layers / FORGE_TOKEN_LAYERS=1) is on, dropout is inactive
    (p == 0, or the module is in eval mode) and the arguments are in the kernels' domain - of ops.token_linear, or with weight None of
    ops.layer_norm (ln = (gamma, beta, eps))."""
    if not _token_layers.on or (dropout_p != 0 and training):
        return False
    if weight is None:
        return isinstance(ln, (tuple, list)) and len(ln) == 3 and _layer_norm_domain(x, *ln)
    return _token_domain(x, weight, bias, ln, act, residual)


def _token_check(what, x, weight, bias, ln, act, residual):
    if _token_domain(x, weight, bias, ln, act, residual):
        return
    raise RuntimeError("forge_amd: ops.%s needs fp32 x [...,K] and weight [N,K] on the MI355X with K and N multiples of 64 up to %d (K <= %d under a "
                       "LayerNorm (gamma, beta, eps)), channel stride 1, one row stride that is a multiple of 4 floats, 16-byte aligned storage, act None "
                       "or 'gelu', bias [N] and residual [...,N] (got act %r, x %s, weight %s, bias %s, ln %s, residual %s)"
                       % (what, TOKEN_MAX_CHANNELS, TOKEN_MAX_LN_CHANNELS, act, _tensor_desc(x), _tensor_desc(weight), _tensor_desc(bias),
                          "(%s)" % ", ".join(_tensor_desc(t) for t in ln) if isinstance(ln, (tuple, list)) else repr(ln), _tensor_desc(residual)))


def _layer_norm_check(what, x, gamma, beta, eps):
    if _layer_norm_domain(x, gamma, beta, eps):
        return
    raise RuntimeError("forge_amd: ops.%s needs fp32 x [...,K] on the MI355X with K a multiple of 64 up to %d, channel stride 1, one row stride that is a "
                       "multiple of 4 floats, 16-byte aligned storage, gamma / beta [K] and a finite eps >= 0 (got x %s, gamma %s, beta %s, eps %r)"
                       % (what, TOKEN_MAX_LN_CHANNELS, _tensor_desc(x), _tensor_desc(gamma), _tensor_desc(beta), eps))


_TOKEN_ACT = {None: 0, "gelu": 1}


def _token_forward(x, weight, bias, ln, act, residual, out, want_saved):
    """One forge_token_linear_fwd launch. Returns (y, stats or None, pre or None); stats / pre only when want_saved (the autograd form)."""
    (xr, ldx), N = _token_rows(x), weight.shape[0]
    R, K = xr.shape
    y = _empty_f32(x.device, x.shape[:-1] + (N,)) if out is None else out
    yr, ldy = _token_rows(y)
    rr, ldr = _token_rows(residual) if residual is not None else (None, 0)
    gamma, beta, eps = ln if ln is not None else (None, None, 0.0)
    stats = _empty_f32(x.device, R, 2) if want_saved and ln is not None else None
    pre = _empty_f32(x.device, R, N) if want_saved and act is not None else None
    _lib.check(_lib.lib().forge_token_linear_fwd(_lib.ptr(xr), ldx, _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(gamma), _lib.ptr(beta), float(eps),
                                                 _lib.ptr(rr), ldr, _lib.ptr(yr), ldy, _lib.ptr(pre), _lib.ptr(stats), R, K, N, _TOKEN_ACT[act],
                                                 _lib.current_stream()), "forge_token_linear_fwd")
    return y, stats, pre


@_lib.on_tensor_device
def token_linear(x, weight, bias=None, ln=None, act=None, residual=None, out=None):
    """act(LN?(x) weight^T + bias) (+ residual) in one launch (forge_token_linear_fwd): x [...,K], weight [N,K] (nn.Linear's), ln = (gamma, beta,
    eps) a LayerNorm over the K channels in front of the product, act None or "gelu" (exact erf), residual [...,N] added last -> [...,N]. `out`:
    a preallocated [...,N] destination, possibly a slice of a wider tensor (a q|k|v slab); the bits do not depend on its strides. Inference only
    (no autograd node); independent of the switch (that gates token_layers_applies, the modules' dispatch); outside the domain it raises."""
    _token_check("token_linear", x, weight, bias, ln, act, residual)
    if out is not None and not (_token_rows(out) is not None and out.device == x.device and out.shape == x.shape[:-1] + (weight.shape[0],)):
        raise RuntimeError("forge_amd: ops.token_linear: out must be fp32 %s on x's device, addressed like x (got %s)"
                           % (tuple(x.shape[:-1] + (weight.shape[0],)), _tensor_desc(out)))
    det = lambda t: None if t is None else t.detach()
    y = _token_forward(x.detach(), weight.detach(), det(bias), None if ln is None else (ln[0].detach(), ln[1].detach(), ln[2]), act, det(residual),
                       det(out), False)[0]
    return y if out is None else out


class _TokenLinearTrain(torch.autograd.Function):
    """forge_token_linear_fwd / forge_token_linear_bwd: saved for backward are x (as it came), the parameters, stats [R,2] (with a LayerNorm) and the
    pre-activation (only with GELU) - never the normalised rows."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, x, weight, bias, gamma, beta, residual, eps, act):
        ln = None if gamma is None else (gamma, beta, eps)
        y, stats, pre = _token_forward(x, weight, bias, ln, act, residual, None, True)
        ctx.act, ctx.has_ln = act, ln is not None
        ctx.save_for_backward(x, weight, gamma, beta, stats, pre)
        return y

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, dy):
        x, weight, gamma, beta, stats, pre = ctx.saved_tensors
        need = ctx.needs_input_grad
        (xr, ldx), (N, K) = _token_rows(x), weight.shape
        R = xr.shape[0]
        dy = dy.contiguous()
        dyr = dy.view(R, N)
        dev = x.device
        dx = _empty_f32(dev, x.shape) if need[0] else None
        dw = _empty_f32(dev, N, K) if need[1] or need[2] else None                    # dbias is a by-product of the dW pass
        db = _empty_f32(dev, N) if need[2] else None
        dg = _empty_f32(dev, K) if ctx.has_ln and need[3] else None
        dbt = _empty_f32(dev, K) if ctx.has_ln and need[4] else None
        ws, nbytes = _bwd_workspace("forge_token_linear_bwd_ws_bytes", dev, R, K, N, int(ctx.has_ln))
        _lib.check(_lib.lib().forge_token_linear_bwd(_lib.ptr(dyr), N, _lib.ptr(xr), ldx, _lib.ptr(weight), _lib.ptr(gamma), _lib.ptr(beta),
                                                     _lib.ptr(stats), _lib.ptr(pre), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(dg), _lib.ptr(dbt),
                                                     _lib.ptr(ws), nbytes, R, K, N, _TOKEN_ACT[ctx.act], _lib.current_stream()), "forge_token_linear_bwd")
        return dx, (dw if need[1] else None), db, dg, dbt, (dy if need[5] else None), None, None


def token_linear_train(x, weight, bias=None, ln=None, act=None, residual=None):
    """ops.token_linear inside an autograd graph (same kernel, same bits) with the HIP backward forge_token_linear_bwd: gradients for x, weight,
    bias, the LayerNorm's gamma / beta and the residual; the normalised rows are recomputed, the sums over rows are chunked in a fixed order (no
    atomics: bitwise reproducible). Independent of the switch; outside the domain it raises."""
    _token_check("token_linear_train", x, weight, bias, ln, act, residual)
    gamma, beta, eps = ln if ln is not None else (None, None, 0.0)
    return _TokenLinearTrain.apply(x, weight, bias, gamma, beta, residual, float(eps), act)


def _layer_norm_forward(x, gamma, beta, eps, want_stats):
    xr, ldx = _token_rows(x)
    R, K = xr.shape
    y = _empty_f32(x.device, x.shape)
    stats = _empty_f32(x.device, R, 2) if want_stats else None
    _lib.check(_lib.lib().forge_layer_norm_fwd(_lib.ptr(xr), ldx, _lib.ptr(gamma), _lib.ptr(beta), float(eps), _lib.ptr(y), K, _lib.ptr(stats), R, K,
                                               _lib.current_stream()), "forge_layer_norm_fwd")
    return y, stats


@_lib.on_tensor_device
def layer_norm(x, gamma, beta, eps=1e-5):
    """F.layer_norm(x, (K,), gamma, beta, eps) over the last dimension of x [...,K] (forge_layer_norm_fwd: the LayerNorm prologue of
    ops.token_linear stand-alone, same bits). Inference only (no autograd node); independent of the switch; outside the domain it raises."""
    _layer_norm_check("layer_norm", x, gamma, beta, eps)
    return _layer_norm_forward(x.detach(), gamma.detach(), beta.detach(), eps, False)[0]


class _LayerNormTrain(torch.autograd.Function):
    """forge_layer_norm_fwd / forge_layer_norm_bwd: saved for backward are x, gamma and stats [R,2]."""

    @staticmethod
    @_lib.on_tensor_device
    def forward(ctx, x, gamma, beta, eps):
        y, stats = _layer_norm_forward(x, gamma, beta, eps, True)
        ctx.save_for_backward(x, gamma, stats)
        return y

    @staticmethod
    @_lib.on_tensor_device
    def backward(ctx, dy):
        x, gamma, stats = ctx.saved_tensors
        need = ctx.needs_input_grad
        xr, ldx = _token_rows(x)
        R, K = xr.shape
        dyr = dy.contiguous().view(R, K)
        dev = x.device
        dx, dg, dbt = (_empty_f32(dev, x.shape) if need[0] else None), (_empty_f32(dev, K) if need[1] else None), (_empty_f32(dev, K) if need[2] else None)
        ws, nbytes = _bwd_workspace("forge_layer_norm_bwd_ws_bytes", dev, R, K)
        _lib.check(_lib.lib().forge_layer_norm_bwd(_lib.ptr(dyr), K, _lib.ptr(xr), ldx, _lib.ptr(gamma), _lib.ptr(stats), _lib.ptr(dx), _lib.ptr(dg),
                                                   _lib.ptr(dbt), _lib.ptr(ws), nbytes, R, K, _lib.current_stream()), "forge_layer_norm_bwd")
        return dx, dg, dbt, None


def layer_norm_train(x, gamma, beta, eps=1e-5):
    """ops.layer_norm inside an autograd graph (same kernel, same bits) with the HIP backward forge_layer_norm_bwd (no atomics: bitwise
    reproducible). Independent of the switch; outside the domain it raises."""
    _layer_norm_check("layer_norm_train", x, gamma, beta, eps)
    return _LayerNormTrain.apply(x, gamma, beta, float(eps))


def token_rows_plan(R, K, N):
    """(chunks, chunk_rows) of forge_token_linear_bwd's sums over rows (dW, dbias): host arithmetic on the shape alone (forge_token_rows_plan)."""
    c, r = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().forge_token_rows_plan(int(R), int(K), int(N), ctypes.byref(c), ctypes.byref(r)), "forge_token_rows_plan")
    return c.value, r.value


def _plain_layer_norm(norm, K):
    """(gamma, beta, eps) of an nn.LayerNorm over the last K channels with both affine parameters, else None."""
    if (isinstance(norm, torch.nn.LayerNorm) and tuple(norm.normalized_shape) == (K,) and norm.weight is not None and norm.bias is not None):
        return norm.weight, norm.bias, norm.eps
    return None


# Call sites that stay on torch even with the switch on (names: the `site` arguments of the modules' dispatch - 2d.proj, 2d.o_proj, 2d.fc1,
# 2d.fc2, 2d.norm, 3d.qk, 3d.v, 3d.fc1, 3d.fc2). profiles/r16_token_layers_probe.txt: as a hipGraph replay at one scene PoseEstimator3D wins
# every alternated window with its sites on the kernels, PoseEstimator2D loses every window (2.65 ms against 2.39 ms) - rocBLAS is the faster
# GEMM at 1024 x 256 rows once the launches cost nothing - so the 2-D estimator's sites are listed here until their kernels win. Tests and
# tools/token_layers_probe.py empty the set to exercise and measure the 2-D wiring.
TOKEN_SITES_ON_TORCH = frozenset(("2d.proj", "2d.o_proj", "2d.fc1", "2d.fc2", "2d.norm"))


def module_token_linear(x, weight, bias, norm=None, act=None, residual=None, dropout_p=0.0, training=False, site=None):
    """The modules' dispatch of one `residual + act(linear(norm(x)))` site: the fused launch (ops.token_linear_train inside an autograd graph, else
    ops.token_linear) when token_layers_applies holds, else None - the caller then runs its stock statements. norm: an nn.LayerNorm or None; act: an
    nn.GELU (exact erf) or None."""
    if not _token_layers.on or site in TOKEN_SITES_ON_TORCH:
        return None
    ln = None
    if norm is not None:
        ln = _plain_layer_norm(norm, x.shape[-1]) if torch.is_tensor(x) and x.dim() >= 1 else None
        if ln is None:
            return None
    if act is not None and not (isinstance(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none"):
        return None
    a = None if act is None else "gelu"
    if not token_layers_applies(x, weight, bias, ln, a, residual, dropout_p=dropout_p, training=training):
        return None
    fn = token_linear_train if torch.is_grad_enabled() else token_linear
    return fn(x, weight, bias, ln=ln, act=a, residual=residual)


def module_layer_norm(x, norm, site=None):
    """The modules' dispatch of one stand-alone nn.LayerNorm site: ops.layer_norm(_train) when token_layers_applies holds, else None."""
    if not _token_layers.on or site in TOKEN_SITES_ON_TORCH or not torch.is_tensor(x) or x.dim() < 1:
        return None
    ln = _plain_layer_norm(norm, x.shape[-1])
    if ln is None or not token_layers_applies(x, ln=ln):
        return None
    return (layer_norm_train if torch.is_grad_enabled() else layer_norm)(x, *ln)


# ------------------------------------------------------------------------------------------------------------- camera synchronisation
POSE_SYNC_MASS, POSE_SYNC_RANK, POSE_SYNC_NONFINITE = 1, 2, 4      # status bits of forge_pose_sync
_pose_sync_pairs = {}                                              # (pair list, N, device) -> device int32 [E, 2]


def pose_sync_pairs(pairs, N, device=None):
    """The pair list of a synchronisation problem, checked as utils/sync_utils.py:104-114 checks it (i != j, no pair twice in either order, every
    view in some pair) plus both < N. Returns the list as a tuple of (i, j); with a device, the cached int32 [E, 2] tensor on it instead."""
    N = int(N)
    if not 3 <= N <= 8:
        raise ValueError("pose_sync: N=%d outside 3..8 (two views are plain chaining: utils/sync_utils.py:camera_chaining)" % N)
    key = tuple((int(i), int(j)) for i, j in pairs)
    seen = set()
    for i, j in key:
        if i == j:
            raise ValueError("pose_sync: pair (%d, %d) joins a view with itself" % (i, j))
        if not (0 <= i < N and 0 <= j < N):
            raise ValueError("pose_sync: pair (%d, %d) names a view outside 0..%d" % (i, j, N - 1))
        if (i, j) in seen or (j, i) in seen:
            raise ValueError("pose_sync: pair (%d, %d) is given twice (in either order)" % (i, j))
        seen.add((i, j))
    for v in range(N):
        if not any(v in p for p in key):
            raise ValueError("pose_sync: view %d is not in any pairwise views" % v)
    if device is None:
        return key
    ck = (key, N, str(device))
    if ck not in _pose_sync_pairs:
        if len(_pose_sync_pairs) >= 64:                            # a protocol uses one or two pair lists; never grow without bound
            _pose_sync_pairs.clear()
        _pose_sync_pairs[ck] = torch.tensor(key, dtype=torch.int32).reshape(len(key), 2).to(device)
    return _pose_sync_pairs[ck]


@_lib.on_tensor_device
def pose_sync(P, conf, pairs, N, squares=10, center_first_camera=False, rank_tol=1e-6, return_sv=False):
    """utils/sync_utils.py:camera_synchronization(Ps, confidence, N, squares, so3_projection=True, normalize_confidences=True, double=True,
    center_first_camera) as one launch of forge_pose_sync. P [B, E, 4, 4] float32: P[:, e] is the extrinsics pairs[e] = (i, j), i -> j;
    conf [B, E]; pairs: a host sequence of (i, j). Returns (out [B, N, 4, 4] float32, status [B] int32) and, with return_sv, the float64
    singular values [B, N, 3] of the rotation blocks before their projection. status bits: POSE_SYNC_MASS (the reference's assertion would have
    fired), POSE_SYNC_RANK (sigma_min / sigma_max < rank_tol for some view: that rotation is not determined), POSE_SYNC_NONFINITE. Nothing is
    read back: a caller that wants the reference's exception tests `status` itself. All arithmetic is float64 (the reference forms L in
    float32 first)."""
    if not torch.is_tensor(P) or not torch.is_tensor(conf):
        raise TypeError("pose_sync: P and conf must be tensors")
    _require_cuda(P, conf)
    if P.dim() != 4 or tuple(P.shape[2:]) != (4, 4) or conf.shape != P.shape[:2] or P.device != conf.device:
        raise ValueError("pose_sync: P [B, E, 4, 4] and conf [B, E] on one device, got %s and %s" % (tuple(P.shape), tuple(conf.shape)))
    if P.dtype != torch.float32 or conf.dtype != torch.float32:
        raise TypeError("pose_sync: float32 inputs (got %s, %s); they are widened to float64 on load" % (P.dtype, conf.dtype))
    B, E = int(P.shape[0]), int(P.shape[1])
    pairs_dev = pose_sync_pairs(pairs, N, P.device)
    if pairs_dev.shape[0] != E:
        raise ValueError("pose_sync: %d pairs for %d matrices" % (pairs_dev.shape[0], E))
    if B < 1:
        raise ValueError("pose_sync: empty batch")
    N = int(N)
    Pc, cc = P.detach().contiguous(), conf.detach().contiguous()
    out = torch.empty(B, N, 4, 4, dtype=torch.float32, device=P.device)
    status = torch.empty(B, dtype=torch.int32, device=P.device)
    sv = torch.empty(B, N, 3, dtype=torch.float64, device=P.device) if return_sv else None
    _lib.check(_lib.lib().forge_pose_sync(_lib.ptr(Pc), _lib.ptr(cc), _lib.ptr(pairs_dev), B, N, E, int(squares), 0 if center_first_camera else N // 2,
                                          float(rank_tol), _lib.ptr(out), _lib.ptr(sv), _lib.ptr(status), _lib.current_stream()), "forge_pose_sync")
    return (out, status, sv) if return_sv else (out, status)


# ------------------------------------------------------------------------------------------------------------------- mesh extraction
MESH_OVERFLOW = 1                                                  # status bit of forge_mesh_emit (FORGE_MESH_OVERFLOW)
MESH_TABLE_INTS = 154
_mesh_table = None


def mesh_case_table():
    """The marching-tetrahedra case table of csrc/mesh.hip (forge_mesh_case_table, host only: no device is touched), as int lists:
    tet_corner [6][4], tet_flip [6], tet_edge [6][2], case_ntri [16], case_tri [16][2][3] (include/forge_hip.h section g1)."""
    global _mesh_table
    if _mesh_table is None:
        buf = (ctypes.c_int * MESH_TABLE_INTS)()
        _lib.check(_lib.lib().forge_mesh_case_table(buf, MESH_TABLE_INTS), "forge_mesh_case_table")
        v = list(buf)
        _mesh_table = {
            "tet_corner": [v[4 * q:4 * q + 4] for q in range(6)],
            "tet_flip": v[24:30],
            "tet_edge": [v[30 + 2 * e:32 + 2 * e] for e in range(6)],
            "case_ntri": v[42:58],
            "case_tri": [[v[58 + 6 * m + 3 * t:61 + 6 * m + 3 * t] for t in range(2)] for m in range(16)],
        }
    return _mesh_table


def _check_tensors(fn, want, dev=None):
    """The one tensor-table check of the geometry wrappers. want: (name, tensor or None, shape, dtype). An int in place of a shape asks for a
    1-D tensor of at least that many elements, which may not be None (a workspace). Without dev, the device of the first tensor is the device
    of all. Returns that device."""
    if dev is None:
        dev = next(t for _, t, _, _ in want if t is not None).device
    for name, t, shape, dt in want:
        least = shape if isinstance(shape, int) else None
        if t is None and least is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor" % (fn, name))
        if t.dtype != dt:
            raise TypeError("%s: %s must be %s (got %s)" % (fn, name, dt, t.dtype))
        if (t.shape != shape if least is None else t.dim() != 1 or t.shape[0] < least) or not t.is_contiguous() or t.device != dev:
            raise ValueError("%s: %s must be a contiguous %s tensor on %s, got %s with strides %s on %s"
                             % (fn, name, tuple(shape) if least is None else "1-D, %d elements or more," % least, dev, tuple(t.shape), t.stride(), t.device))
    return dev


def _out_or_empty(fn, out, specs, dev):
    """The `out=` argument: specs is a list of (shape, dtype) or None (no such output). out None: fresh tensors; else out's tensors, checked."""
    if out is None:
        return [None if sp is None else torch.empty(sp[0], dtype=sp[1], device=dev) for sp in specs]
    for t, sp in zip(out, specs):
        if sp is not None and (not isinstance(t, torch.Tensor) or t.shape != sp[0] or t.dtype != sp[1] or not t.is_contiguous() or t.device != dev):
            raise ValueError("%s: every out tensor must be contiguous, here %s of shape %s on %s" % (fn, sp[1], tuple(sp[0]), dev))
    return [None if sp is None else t for t, sp in zip(out, specs)]


def _density_volume(fn, density, level=None):
    """density is a contiguous float32 [n,1,D,H,W] with n >= 1, level (when given) finite and > 0 -> (n, D, H, W, level). Shape, dtype, layout and
    level only: the device comes last (the caller's _require_cuda), so a wrong argument is named as what it is on any machine."""
    if not isinstance(density, torch.Tensor):
        raise TypeError("%s: density must be a tensor" % fn)
    if density.dim() != 5 or density.shape[1] != 1:
        raise ValueError("%s: density must be [n,1,D,H,W] (encoder_3d.get_density3D), got %s" % (fn, tuple(density.shape)))
    if density.dtype != torch.float32:
        raise TypeError("%s: float32 density (got %s)" % (fn, density.dtype))
    if not density.is_contiguous():
        raise ValueError("%s: density must be contiguous (strides %s)" % (fn, density.stride()))
    n, _, D, H, W = density.shape
    if n < 1:
        raise ValueError("%s: empty batch" % fn)
    if level is not None:
        level = float(level)
        if not (level > 0.0 and math.isfinite(level)):
            raise ValueError("%s: level=%r must be finite and > 0 (the virtual shell around the volume is zero)" % (fn, level))
    return n, D, H, W, level


def _row_lead(n, offsets):
    """Leading dimensions of mesh rows: [n, rows, ...] padded (offsets None), [rows, ...] packed."""
    return (n,) if offsets is None else ()


def _mesh_features(fn, features, density):
    """features [n,C,D,H,W], channels-last float32 on the density's device, C a positive multiple of 4 -> C (0 without features)."""
    if features is None:
        return 0
    if not torch.is_tensor(features):
        raise TypeError("%s: features must be a tensor" % fn)
    n, _, D, H, W = density.shape
    if features.dim() != 5 or features.shape[0] != n or tuple(features.shape[2:]) != (D, H, W) or features.device != density.device:
        raise ValueError("%s: features must be [%d,C,%d,%d,%d] on the density's device, got %s" % (fn, n, D, H, W, tuple(features.shape)))
    if features.dtype != torch.float32:
        raise TypeError("%s: float32 features (got %s)" % (fn, features.dtype))
    C = int(features.shape[1])
    if C < 4 or C % 4:
        raise ValueError("%s: C=%d feature channels must be a positive multiple of 4" % (fn, C))
    if not features.permute(0, 2, 3, 4, 1).is_contiguous():
        raise ValueError("%s: features must be channels-last (torch.channels_last_3d; ops.to_channels_last_3d), got strides %s" % (fn, features.stride()))
    return C


@_lib.on_tensor_device
def mesh_count(density, level=0.5):
    """forge_mesh_count: classify the cells of density [n,1,D,H,W] and scan. Returns (counts [n,2] int32 on the device: vertices and triangles
    per volume, workspace): the workspace goes to mesh_emit together with the same density and level. Nothing is read back."""
    n, D, H, W, level = _density_volume("mesh_count", density, level)
    _require_cuda(density)
    nbytes = _lib.size_query("forge_mesh_workspace_bytes", n, D, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=density.device)
    counts = torch.empty(n, 2, dtype=torch.int32, device=density.device)
    _lib.check(_lib.lib().forge_mesh_count(_lib.ptr(density.detach()), n, D, H, W, level, _lib.ptr(ws), nbytes, _lib.ptr(counts), _lib.current_stream()),
               "forge_mesh_count")
    return counts, ws


@_lib.on_tensor_device
def mesh_emit(density, workspace, counts, max_vertices, max_faces, level=0.5, volume_size=1.0, features=None, offsets=None, out=None):
    """forge_mesh_emit after mesh_count(density, level). offsets None: every volume gets max_vertices / max_faces rows, the result is
    vertices [n,max_vertices,3], normals [n,max_vertices,3], faces [n,max_faces,3] int32, vertex features [n,max_vertices,C] or None, status [n].
    offsets [n,2] int32 (the exclusive scan of counts over volumes): the volumes are packed one after the other into arrays of max_vertices /
    max_faces rows in all: vertices [max_vertices,3], ... Rows that no vertex or triangle lands in are left as they were. status carries
    MESH_OVERFLOW for a volume that did not fit; what fitted is the prefix of the full result. out: (vertices, normals, faces, features or None)
    to write into, instead of fresh tensors. Nothing is read back."""
    n, D, H, W, level = _density_volume("mesh_emit", density, level)
    C = _mesh_features("mesh_emit", features, density)
    max_vertices, max_faces = int(max_vertices), int(max_faces)
    if max_vertices < 0 or max_faces < 0:
        raise ValueError("mesh_emit: negative capacity (%d, %d)" % (max_vertices, max_faces))
    nbytes = _lib.size_query("forge_mesh_workspace_bytes", n, D, H, W)
    dev = density.device
    _check_tensors("mesh_emit", [("workspace", workspace, nbytes, torch.uint8), ("counts", counts, (n, 2), torch.int32),
                                 ("offsets", offsets, (n, 2), torch.int32)], dev)
    lead = _row_lead(n, offsets)
    vrows = (lead + (max_vertices, 3), torch.float32)
    specs = [vrows, vrows, (lead + (max_faces, 3), torch.int32), None if features is None else (lead + (max_vertices, C), torch.float32)]
    _require_cuda(density, features, workspace, counts, offsets)
    vertices, normals, faces, vfeat = _out_or_empty("mesh_emit", out, specs, dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().forge_mesh_emit(_lib.ptr(density.detach()), _lib.ptr(None if features is None else features.detach()), n, C, D, H, W, level,
                                          float(volume_size), _lib.ptr(workspace), nbytes, _lib.ptr(counts), _lib.ptr(offsets), max_vertices, max_faces,
                                          _lib.ptr(vertices), _lib.ptr(normals), _lib.ptr(faces), _lib.ptr(vfeat), _lib.ptr(status), _lib.current_stream()),
               "forge_mesh_emit")
    return vertices, normals, faces, vfeat, status


# ------------------------------------------------------------------------------------------------------------------- vertex colour bake
BAKE_MODES = {"blend": 0, "best": 1}


@_lib.on_tensor_device
def mesh_bake(vertices, normals, counts, density, images, cam, view2vol, *, offsets=None, view_weight=None, view_gain=None, half, S, step, offset,
              cos_power=2, z_near=1e-3, w_min=1e-3, mode="blend", fill=0.5, out=None):
    """forge_mesh_bake (include/forge_hip.h section g2): colours for the rows mesh_emit wrote, from posed images, weighted by facing and by the
    transmittance of the density field between the vertex and the camera. vertices / normals [n,max_vertices,3] with counts [n,2] (offsets None:
    every volume owns max_vertices rows) or [max_vertices,3] with offsets [n,2] (the volumes packed one after the other); density [n,1,D,H,W];
    images [V,C,Hi,Wi] (C in 1..4), cam [V,16] (R, T, fx, fy, cx, cy in pixels of `images`), view2vol [V] int32, view_weight [V,Hi,Wi] and
    view_gain [V] optional; half = (hx, hy, hz), the half extents of W, H, D. mode "blend" (weighted mean) or "best" (the best view's colour).
    Returns (colors [...,C], weight [...], best [...] int32), the rows laid out as vertices; rows past a volume's count are left as they were
    (out: the three tensors to write into). Nothing is read back."""
    tensors = (vertices, normals, counts, density, images, cam, view2vol)
    if not all(torch.is_tensor(t) for t in tensors) or not all(t is None or torch.is_tensor(t) for t in (offsets, view_weight, view_gain)):
        raise TypeError("mesh_bake: vertices, normals, counts, density, images, cam, view2vol (and offsets, view_weight, view_gain) must be tensors")
    n, D, H, W, _ = _density_volume("mesh_bake", density)
    dev = density.device
    lead = _row_lead(n, offsets)
    if vertices.dim() != len(lead) + 2 or tuple(vertices.shape[:len(lead)]) != lead or vertices.shape[-1] != 3 or normals.shape != vertices.shape:
        raise ValueError("mesh_bake: vertices and normals must both be %s, got %s and %s"
                         % ("[%d,max_vertices,3]" % n if offsets is None else "[max_vertices,3] (packed: offsets given)", tuple(vertices.shape), tuple(normals.shape)))
    max_vertices = int(vertices.shape[-2])
    if images.dim() != 4 or not 1 <= images.shape[1] <= 4 or images.shape[0] < 1:
        raise ValueError("mesh_bake: images must be [V,C,Hi,Wi] with C in 1..4 and V >= 1, got %s" % (tuple(images.shape),))
    V, C, Hi, Wi = (int(s) for s in images.shape)
    _check_tensors("mesh_bake", [("vertices", vertices, vertices.shape, torch.float32), ("normals", normals, vertices.shape, torch.float32),
                                 ("counts", counts, (n, 2), torch.int32), ("offsets", offsets, (n, 2), torch.int32),
                                 ("images", images, images.shape, torch.float32), ("cam", cam, (V, 16), torch.float32),
                                 ("view2vol", view2vol, (V,), torch.int32), ("view_weight", view_weight, (V, Hi, Wi), torch.float32),
                                 ("view_gain", view_gain, (V,), torch.float32)], dev)
    if mode not in BAKE_MODES:
        raise ValueError("mesh_bake: mode=%r (one of %s)" % (mode, sorted(BAKE_MODES)))
    hx, hy, hz = (float(h) for h in half)
    _require_cuda(*tensors, offsets, view_weight, view_gain)
    rows = lead + (max_vertices,)
    colors, weight, best = _out_or_empty("mesh_bake", out, [(rows + (C,), torch.float32), (rows, torch.float32), (rows, torch.int32)], dev)
    _lib.check(_lib.lib().forge_mesh_bake(_lib.ptr(vertices.detach()), _lib.ptr(normals.detach()), _lib.ptr(counts), _lib.ptr(offsets), n, max_vertices,
                                          _lib.ptr(density.detach()), D, H, W, hx, hy, hz, _lib.ptr(images.detach()), _lib.ptr(view_weight), C, Hi, Wi,
                                          _lib.ptr(cam.detach()), _lib.ptr(view2vol), _lib.ptr(view_gain), V, int(S), float(step), float(offset),
                                          int(cos_power), float(z_near), float(w_min), BAKE_MODES[mode], float(fill), _lib.ptr(colors), _lib.ptr(weight),
                                          _lib.ptr(best), _lib.current_stream()), "forge_mesh_bake")
    return colors, weight, best


# ------------------------------------------------------------------------------------------------------------------- surface metrics
GEOM_EMPTY = 1                                                     # status bit (FORGE_GEOM_EMPTY): a mesh without area, a pair with an empty side
GEOM_MAX_THRESHOLDS = 4
GEOM_OUT_DOUBLES = 18
GEOM_SCALARS = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff", "normal_consistency")      # out[:, 0..5]
GEOM_PER_THRESHOLD = (("precision", 6), ("recall", 10), ("fscore", 14))                                         # out[:, first + k]


def nn_constants():
    """(queries per workgroup, references per LDS tile) of forge_nn_points: host only, no device is touched."""
    L = _lib.lib()
    return int(L.forge_nn_queries_per_block()), int(L.forge_nn_tile_points())


@_lib.on_tensor_device
def surface_sample(vertices, faces, counts, n_samples, offsets=None):
    """forge_surface_sample (include/forge_hip.h section g3): n_samples deterministic, area-proportional points on each mesh. vertices
    [n,max_vertices,3] / faces [n,max_faces,3] int32 with counts [n,2] (offsets None: every mesh owns its rows, as mesh_emit pads them) or
    [max_vertices,3] / [max_faces,3] with offsets [n,2] (the meshes packed one after the other). Returns (points [n,n_samples,3], normals
    [n,n_samples,3], face [n,n_samples] int32, bary [n,n_samples,2], status [n] int32 with GEOM_EMPTY for a mesh without area). Nothing is read back."""
    tensors = (vertices, faces, counts)
    if not all(torch.is_tensor(t) for t in tensors) or not (offsets is None or torch.is_tensor(offsets)):
        raise TypeError("surface_sample: vertices, faces, counts (and offsets) must be tensors")
    _require_cuda(*tensors, offsets)
    if counts.dim() != 2 or counts.shape[0] < 1:
        raise ValueError("surface_sample: counts must be [n,2] with n >= 1, got %s" % (tuple(counts.shape),))
    n = int(counts.shape[0])
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError("surface_sample: n_samples=%d must be at least 1" % n_samples)
    lead = _row_lead(n, offsets)
    if vertices.dim() != len(lead) + 2 or faces.dim() != len(lead) + 2:
        raise ValueError("surface_sample: vertices and faces must be %s, got %s and %s"
                         % ("[%d,rows,3]" % n if offsets is None else "[rows,3] (packed: offsets given)", tuple(vertices.shape), tuple(faces.shape)))
    mv, mf = int(vertices.shape[-2]), int(faces.shape[-2])
    dev = _check_tensors("surface_sample", [("vertices", vertices, lead + (mv, 3), torch.float32), ("faces", faces, lead + (mf, 3), torch.int32),
                                         ("counts", counts, (n, 2), torch.int32), ("offsets", offsets, (n, 2), torch.int32)])
    nbytes = _lib.size_query("forge_surface_sample_workspace_bytes", n, mf, 0 if offsets is None else 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    points = torch.empty(n, n_samples, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(n, n_samples, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n, n_samples, dtype=torch.int32, device=dev)
    bary = torch.empty(n, n_samples, 2, dtype=torch.float32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().forge_surface_sample(_lib.ptr(vertices.detach()), _lib.ptr(faces), _lib.ptr(counts), _lib.ptr(offsets), n, mv, mf, n_samples,
                                               _lib.ptr(ws), nbytes, _lib.ptr(points), _lib.ptr(normals), _lib.ptr(face), _lib.ptr(bary), _lib.ptr(status),
                                               _lib.current_stream()), "forge_surface_sample")
    return points, normals, face, bary, status


@_lib.on_tensor_device
def nn_points(q, p, q_count=None, p_count=None, xf=None, return_transformed=False):
    """forge_nn_points (section g3): for every query q [B,Nq,3] the nearest of the references p [B,Np,3] of its pair, brute force and exact in fp32's
    difference form. q_count / p_count [B] int32 on the device (None: all rows); xf [B,12], a row-major 3x4 (s R | t) applied to the queries on
    load. Returns (d2 [B,Nq] float32, idx [B,Nq] int32): ties go to the lowest index; rows past q_count get (0, -1); no references: (+inf, -1).
    return_transformed: also the queries as they were scored, [B,Nq,3] (the references of the opposite direction). Nothing is read back."""
    if not all(torch.is_tensor(t) for t in (q, p)) or not all(t is None or torch.is_tensor(t) for t in (q_count, p_count, xf)):
        raise TypeError("nn_points: q, p (and q_count, p_count, xf) must be tensors")
    _require_cuda(q, p, q_count, p_count, xf)
    if q.dim() != 3 or p.dim() != 3 or q.shape[2] != 3 or p.shape[2] != 3 or q.shape[0] != p.shape[0] or min(q.shape[:2] + p.shape[:2]) < 1:
        raise ValueError("nn_points: q [B,Nq,3] and p [B,Np,3] with B, Nq, Np >= 1, got %s and %s" % (tuple(q.shape), tuple(p.shape)))
    B, Nq, Np = int(q.shape[0]), int(q.shape[1]), int(p.shape[1])
    dev = _check_tensors("nn_points", [("q", q, (B, Nq, 3), torch.float32), ("p", p, (B, Np, 3), torch.float32), ("q_count", q_count, (B,), torch.int32),
                                    ("p_count", p_count, (B,), torch.int32), ("xf", xf, (B, 12), torch.float32)])
    d2 = torch.empty(B, Nq, dtype=torch.float32, device=dev)
    idx = torch.empty(B, Nq, dtype=torch.int32, device=dev)
    q_xf = torch.empty(B, Nq, 3, dtype=torch.float32, device=dev) if return_transformed else None
    _lib.check(_lib.lib().forge_nn_points(_lib.ptr(q.detach()), _lib.ptr(p.detach()), _lib.ptr(q_count), _lib.ptr(p_count),
                                          _lib.ptr(None if xf is None else xf.detach()), B, Nq, Np, _lib.ptr(d2), _lib.ptr(idx), _lib.ptr(q_xf), _lib.current_stream()),
               "forge_nn_points")
    return (d2, idx, q_xf) if return_transformed else (d2, idx)


@_lib.on_tensor_device
def geom_metrics(d2_ab, idx_ab, d2_ba, idx_ba, normals_a=None, normals_b=None, a_count=None, b_count=None, thresholds=()):
    """forge_geom_metrics (section g3): the nn_points results of both directions (A against B: [B,Na]; B against A: [B,Nb]) reduced per pair in
    float64. normals_a [B,Na,3] and normals_b [B,Nb,3]: both or neither; thresholds: up to GEOM_MAX_THRESHOLDS finite numbers (host). Returns
    (out [B,GEOM_OUT_DOUBLES] float64, laid out as GEOM_SCALARS and GEOM_PER_THRESHOLD say, status [B] int32 with GEOM_EMPTY for a pair with an empty
    side). Nothing is read back."""
    tensors = (d2_ab, idx_ab, d2_ba, idx_ba)
    if not all(torch.is_tensor(t) for t in tensors) or not all(t is None or torch.is_tensor(t) for t in (normals_a, normals_b, a_count, b_count)):
        raise TypeError("geom_metrics: d2 / idx of both directions (and normals, counts) must be tensors")
    _require_cuda(*tensors, normals_a, normals_b, a_count, b_count)
    if d2_ab.dim() != 2 or d2_ba.dim() != 2 or d2_ab.shape[0] != d2_ba.shape[0] or min(tuple(d2_ab.shape) + tuple(d2_ba.shape)) < 1:
        raise ValueError("geom_metrics: d2_ab [B,Na] and d2_ba [B,Nb] with B, Na, Nb >= 1, got %s and %s" % (tuple(d2_ab.shape), tuple(d2_ba.shape)))
    if (normals_a is None) != (normals_b is None):
        raise ValueError("geom_metrics: give the normals of both sides, or of neither")
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > GEOM_MAX_THRESHOLDS or not all(math.isfinite(t) for t in thresholds):
        raise ValueError("geom_metrics: at most %d finite thresholds, got %r" % (GEOM_MAX_THRESHOLDS, thresholds))
    B, Na, Nb = int(d2_ab.shape[0]), int(d2_ab.shape[1]), int(d2_ba.shape[1])
    dev = _check_tensors("geom_metrics", [("d2_ab", d2_ab, (B, Na), torch.float32), ("idx_ab", idx_ab, (B, Na), torch.int32),
                                       ("d2_ba", d2_ba, (B, Nb), torch.float32), ("idx_ba", idx_ba, (B, Nb), torch.int32),
                                       ("normals_a", normals_a, (B, Na, 3), torch.float32), ("normals_b", normals_b, (B, Nb, 3), torch.float32),
                                       ("a_count", a_count, (B,), torch.int32), ("b_count", b_count, (B,), torch.int32)])
    npart = _lib.size_query("forge_geom_metrics_partial_doubles", B)
    partial = torch.empty(npart, dtype=torch.float64, device=dev)
    out = torch.empty(B, GEOM_OUT_DOUBLES, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    tau = (ctypes.c_double * GEOM_MAX_THRESHOLDS)(*thresholds)
    _lib.check(_lib.lib().forge_geom_metrics(_lib.ptr(d2_ab), _lib.ptr(idx_ab), _lib.ptr(d2_ba), _lib.ptr(idx_ba),
                                             _lib.ptr(None if normals_a is None else normals_a.detach()),
                                             _lib.ptr(None if normals_b is None else normals_b.detach()), _lib.ptr(a_count), _lib.ptr(b_count), B, Na, Nb,
                                             tau, len(thresholds), _lib.ptr(partial), _lib.ptr(out), _lib.ptr(status), _lib.current_stream()),
               "forge_geom_metrics")
    return out, status


def nn_tile_faces():
    """Faces per LDS tile of forge_nn_triangles: host only, no device is touched."""
    return int(_lib.lib().forge_nn_tile_faces())


@_lib.on_tensor_device
def nn_triangles(q, vertices, faces, counts, offsets=None, q_count=None, xf_q=None, xf_mesh=None, want_closest=False, want_normal=False,
                 workspace=None):
    """forge_nn_triangles (section g3b): for every query q [B,Nq,3] the closest triangle of mesh b, brute force and exact in fp32's closest-point
    form. The mesh rows as surface_sample takes them: vertices [B,max_vertices,3] / faces [B,max_faces,3] int32 with counts [B,2] (offsets None)
    or [max_vertices,3] / [max_faces,3] with offsets [B,2] (packed). q_count [B] int32 on the device (None: all rows); xf_q / xf_mesh [B,12],
    row-major 3x4 (s R | t) applied to the queries / to every vertex on load. Returns (d2 [B,Nq] float32, face [B,Nq] int32, closest [B,Nq,3] or
    None, normal [B,Nq,3] or None): ties go to the lowest face; rows past q_count get (0, -1); no candidate face: (+inf, -1); faces with a bad
    index or without area are never candidates. workspace: a uint8 tensor of forge_nn_triangles_workspace_bytes to stage the faces in (None: a
    fresh one). Nothing is read back."""
    tensors = (q, vertices, faces, counts)
    optional = (offsets, q_count, xf_q, xf_mesh, workspace)
    if not all(torch.is_tensor(t) for t in tensors) or not all(t is None or torch.is_tensor(t) for t in optional):
        raise TypeError("nn_triangles: q, vertices, faces, counts (and offsets, q_count, xf_q, xf_mesh, workspace) must be tensors")
    _require_cuda(*tensors, *optional)
    if q.dim() != 3 or q.shape[2] != 3 or min(q.shape[:2]) < 1:
        raise ValueError("nn_triangles: q must be [B,Nq,3] with B, Nq >= 1, got %s" % (tuple(q.shape),))
    B, Nq = int(q.shape[0]), int(q.shape[1])
    lead = _row_lead(B, offsets)
    if vertices.dim() != len(lead) + 2 or faces.dim() != len(lead) + 2:
        raise ValueError("nn_triangles: vertices and faces must be %s, got %s and %s"
                         % ("[%d,rows,3]" % B if offsets is None else "[rows,3] (packed: offsets given)", tuple(vertices.shape), tuple(faces.shape)))
    mv, mf = int(vertices.shape[-2]), int(faces.shape[-2])
    nbytes = _lib.size_query("forge_nn_triangles_workspace_bytes", B, mf, 0 if offsets is None else 1)
    want = [("q", q, (B, Nq, 3), torch.float32), ("vertices", vertices, lead + (mv, 3), torch.float32), ("faces", faces, lead + (mf, 3), torch.int32),
            ("counts", counts, (B, 2), torch.int32), ("offsets", offsets, (B, 2), torch.int32), ("q_count", q_count, (B,), torch.int32),
            ("xf_q", xf_q, (B, 12), torch.float32), ("xf_mesh", xf_mesh, (B, 12), torch.float32)]
    if workspace is not None:
        want.append(("workspace", workspace, nbytes, torch.uint8))
    dev = _check_tensors("nn_triangles", want)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rows3 = ((B, Nq, 3), torch.float32)
    d2, face, closest, normal = _out_or_empty("nn_triangles", None, [((B, Nq), torch.float32), ((B, Nq), torch.int32), rows3 if want_closest else None,
                                                                      rows3 if want_normal else None], dev)
    _lib.check(_lib.lib().forge_nn_triangles(_lib.ptr(q.detach()), _lib.ptr(q_count), _lib.ptr(None if xf_q is None else xf_q.detach()),
                                             _lib.ptr(vertices.detach()), _lib.ptr(faces), _lib.ptr(counts), _lib.ptr(offsets),
                                             _lib.ptr(None if xf_mesh is None else xf_mesh.detach()), B, Nq, mv, mf, _lib.ptr(workspace),
                                             int(workspace.numel()), _lib.ptr(d2), _lib.ptr(face), _lib.ptr(closest), _lib.ptr(normal),
                                             _lib.current_stream()), "forge_nn_triangles")
    return d2, face, closest, normal


@_lib.on_tensor_device
def winding_number(q, vertices, faces, counts, offsets=None, q_count=None, xf_q=None, xf_mesh=None, workspace=None):
    """forge_winding_number (section g3c): for every query q [B,Nq,3] the generalized winding number of mesh b - the signed solid angles of its
    triangles summed, over 4 pi: 1 inside a closed mesh wound as mesh_emit winds it, 0 outside, and defined for meshes with holes. The mesh rows,
    q_count, xf_q, xf_mesh and workspace (forge_winding_workspace_bytes) as nn_triangles takes them; faces with a bad index or without area add
    nothing. Returns w [B,Nq] float32; rows past q_count and meshes without a valid face get 0. Nothing is read back."""
    tensors = (q, vertices, faces, counts)
    optional = (offsets, q_count, xf_q, xf_mesh, workspace)
    if not all(torch.is_tensor(t) for t in tensors) or not all(t is None or torch.is_tensor(t) for t in optional):
        raise TypeError("winding_number: q, vertices, faces, counts (and offsets, q_count, xf_q, xf_mesh, workspace) must be tensors")
    _require_cuda(*tensors, *optional)
    if q.dim() != 3 or q.shape[2] != 3 or min(q.shape[:2]) < 1:
        raise ValueError("winding_number: q must be [B,Nq,3] with B, Nq >= 1, got %s" % (tuple(q.shape),))
    B, Nq = int(q.shape[0]), int(q.shape[1])
    lead = _row_lead(B, offsets)
    if vertices.dim() != len(lead) + 2 or faces.dim() != len(lead) + 2:
        raise ValueError("winding_number: vertices and faces must be %s, got %s and %s"
                         % ("[%d,rows,3]" % B if offsets is None else "[rows,3] (packed: offsets given)", tuple(vertices.shape), tuple(faces.shape)))
    mv, mf = int(vertices.shape[-2]), int(faces.shape[-2])
    nbytes = _lib.size_query("forge_winding_workspace_bytes", B, mf, 0 if offsets is None else 1)
    want = [("q", q, (B, Nq, 3), torch.float32), ("vertices", vertices, lead + (mv, 3), torch.float32), ("faces", faces, lead + (mf, 3), torch.int32),
            ("counts", counts, (B, 2), torch.int32), ("offsets", offsets, (B, 2), torch.int32), ("q_count", q_count, (B,), torch.int32),
            ("xf_q", xf_q, (B, 12), torch.float32), ("xf_mesh", xf_mesh, (B, 12), torch.float32)]
    if workspace is not None:
        want.append(("workspace", workspace, nbytes, torch.uint8))
    dev = _check_tensors("winding_number", want)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    w = torch.empty(B, Nq, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().forge_winding_number(_lib.ptr(q.detach()), _lib.ptr(q_count), _lib.ptr(None if xf_q is None else xf_q.detach()),
                                               _lib.ptr(vertices.detach()), _lib.ptr(faces), _lib.ptr(counts), _lib.ptr(offsets),
                                               _lib.ptr(None if xf_mesh is None else xf_mesh.detach()), B, Nq, mv, mf, _lib.ptr(workspace),
                                               int(workspace.numel()), _lib.ptr(w), _lib.current_stream()), "forge_winding_number")
    return w


@_lib.on_tensor_device
def geom_metrics_hits(d2_ab, hit_ab, d2_ba, hit_ba, normals_a=None, normals_b=None, a_count=None, b_count=None, thresholds=()):
    """forge_geom_metrics_hits (section g3b): geom_metrics with row-aligned "to" normals - hit_ab [B,Na,3] and hit_ba [B,Nb,3], the `normal` of
    nn_triangles, in place of idx_ab / idx_ba. normals_a, hit_ab, normals_b, hit_ba: all four or none (no normal consistency). Returns
    (out [B,GEOM_OUT_DOUBLES] float64, status [B] int32), laid out as geom_metrics'. Nothing is read back."""
    tensors = (d2_ab, d2_ba)
    optional = (hit_ab, hit_ba, normals_a, normals_b, a_count, b_count)
    if not all(torch.is_tensor(t) for t in tensors) or not all(t is None or torch.is_tensor(t) for t in optional):
        raise TypeError("geom_metrics_hits: d2 of both directions (and hits, normals, counts) must be tensors")
    _require_cuda(*tensors, *optional)
    if d2_ab.dim() != 2 or d2_ba.dim() != 2 or d2_ab.shape[0] != d2_ba.shape[0] or min(tuple(d2_ab.shape) + tuple(d2_ba.shape)) < 1:
        raise ValueError("geom_metrics_hits: d2_ab [B,Na] and d2_ba [B,Nb] with B, Na, Nb >= 1, got %s and %s" % (tuple(d2_ab.shape), tuple(d2_ba.shape)))
    if sum(t is not None for t in (hit_ab, hit_ba, normals_a, normals_b)) not in (0, 4):
        raise ValueError("geom_metrics_hits: give the normals and the hit normals of both sides, or none of the four")
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > GEOM_MAX_THRESHOLDS or not all(math.isfinite(t) for t in thresholds):
        raise ValueError("geom_metrics_hits: at most %d finite thresholds, got %r" % (GEOM_MAX_THRESHOLDS, thresholds))
    B, Na, Nb = int(d2_ab.shape[0]), int(d2_ab.shape[1]), int(d2_ba.shape[1])
    dev = _check_tensors("geom_metrics_hits", [("d2_ab", d2_ab, (B, Na), torch.float32), ("hit_ab", hit_ab, (B, Na, 3), torch.float32),
                                            ("d2_ba", d2_ba, (B, Nb), torch.float32), ("hit_ba", hit_ba, (B, Nb, 3), torch.float32),
                                            ("normals_a", normals_a, (B, Na, 3), torch.float32), ("normals_b", normals_b, (B, Nb, 3), torch.float32),
                                            ("a_count", a_count, (B,), torch.int32), ("b_count", b_count, (B,), torch.int32)])
    npart = _lib.size_query("forge_geom_metrics_partial_doubles", B)
    partial, out, status = _out_or_empty("geom_metrics_hits", None, [((npart,), torch.float64), ((B, GEOM_OUT_DOUBLES), torch.float64),
                                                                     ((B,), torch.int32)], dev)
    tau = (ctypes.c_double * GEOM_MAX_THRESHOLDS)(*thresholds)
    det = lambda t: None if t is None else t.detach()                                                               # noqa: E731
    _lib.check(_lib.lib().forge_geom_metrics_hits(_lib.ptr(d2_ab), _lib.ptr(det(hit_ab)), _lib.ptr(d2_ba), _lib.ptr(det(hit_ba)), _lib.ptr(det(normals_a)),
                                                  _lib.ptr(det(normals_b)), _lib.ptr(a_count), _lib.ptr(b_count), B, Na, Nb, tau, len(thresholds),
                                                  _lib.ptr(partial), _lib.ptr(out), _lib.ptr(status), _lib.current_stream()), "forge_geom_metrics_hits")
    return out, status


# ------------------------------------------------------------------------------------------------------------------------- alignment
ALIGN_EMPTY, ALIGN_RANK, ALIGN_NONFINITE, ALIGN_CONVERGED = 1, 2, 4, 8      # status bits (FORGE_ALIGN_*)
ALIGN_STATE_DOUBLES = 29
ALIGN_T, ALIGN_SCALE, ALIGN_RMSE, ALIGN_N_IN, ALIGN_N_VALID, ALIGN_CUT2, ALIGN_DELTA, ALIGN_ITERATIONS, ALIGN_SV, ALIGN_SCORE, ALIGN_CQ, ALIGN_CP = (
    0, 12, 13, 14, 15, 16, 17, 18, 19, 22, 23, 26)                           # columns of a state row (FORGE_ALIGN_*)
ALIGN_RANK_TOL = 1e-6


def align_blocks():
    """Workgroups per pair of forge_align_step's moments pass: host only, no device is touched."""
    return int(_lib.lib().forge_align_blocks())


def align_state(init, B, device):
    """The first state of forge_align_step (section g5) for B pairs, built on the device: T = init ([4,4], [3,4], [B,4,4] or [B,3,4], a similarity;
    None: the identity), SCALE = the length of T's first row, CUT2 = +inf (nothing is rejected in the first step), DELTA = +inf, RMSE = SCORE = NaN
    (a start that was never stepped never wins align_select), everything else 0. Returns (state [B,ALIGN_STATE_DOUBLES] float64, xf [B,12] float32,
    status [B] int32, zero). Nothing is read back."""
    B = int(B)
    if B < 1:
        raise ValueError("align_state: B=%d must be at least 1" % B)
    if init is None:
        T = torch.eye(4, dtype=torch.float64, device=device)[:3].expand(B, 3, 4)
    else:
        T = torch.as_tensor(init, device=device).to(torch.float64)
        if T.dim() == 2:
            T = T[None].expand(B, *T.shape)
        if T.dim() != 3 or T.shape[0] != B or tuple(T.shape[1:]) not in ((4, 4), (3, 4)):
            raise ValueError("align_state: init must be [4,4], [3,4], [%d,4,4] or [%d,3,4], got %s" % (B, B, tuple(T.shape)))
        T = T[:, :3, :]
    state = torch.zeros(B, ALIGN_STATE_DOUBLES, dtype=torch.float64, device=device)
    state[:, ALIGN_T:ALIGN_T + 12] = T.reshape(B, 12)
    state[:, ALIGN_SCALE] = (T[:, 0, 0] * T[:, 0, 0] + T[:, 0, 1] * T[:, 0, 1] + T[:, 0, 2] * T[:, 0, 2]).sqrt()
    state[:, ALIGN_CUT2] = math.inf
    state[:, ALIGN_DELTA] = math.inf
    state[:, ALIGN_RMSE] = math.nan
    state[:, ALIGN_SCORE] = math.nan
    return state, state[:, ALIGN_T:ALIGN_T + 12].to(torch.float32).contiguous(), torch.zeros(B, dtype=torch.int32, device=device)


@_lib.on_tensor_device
def align_step(q, p, state, xf, status, idx=None, d2=None, q_count=None, p_count=None, with_scale=False, update=True, reject=0.0, reject_floor=0.0,
               tol=0.0, rank_tol=ALIGN_RANK_TOL, clamp2=math.inf):
    """forge_align_step (section g5): one least-squares update of the similarity q -> p per pair, IN PLACE on state [B,ALIGN_STATE_DOUBLES] float64,
    xf [B,12] float32 and status [B] int32 (align_state makes the first ones). q [B,Nq,3], p [B,Np,3] float32; idx [B,Nq] int32 and d2 [B,Nq]
    float32 as nn_points returns them (idx None: row i matches row i; d2 None: zeros); q_count / p_count [B] int32 on the device. update False:
    statistics only. A pair whose status carries ALIGN_CONVERGED is left as it is. Returns (state, xf, status), the same tensors. Nothing is
    read back."""
    tensors = (q, p, state, xf, status)
    if not all(torch.is_tensor(t) for t in tensors) or not all(t is None or torch.is_tensor(t) for t in (idx, d2, q_count, p_count)):
        raise TypeError("align_step: q, p, state, xf, status (and idx, d2, q_count, p_count) must be tensors")
    _require_cuda(*tensors, idx, d2, q_count, p_count)
    if q.dim() != 3 or p.dim() != 3 or q.shape[2] != 3 or p.shape[2] != 3 or q.shape[0] != p.shape[0] or min(q.shape[:2] + p.shape[:2]) < 1:
        raise ValueError("align_step: q [B,Nq,3] and p [B,Np,3] with B, Nq, Np >= 1, got %s and %s" % (tuple(q.shape), tuple(p.shape)))
    B, Nq, Np = int(q.shape[0]), int(q.shape[1]), int(p.shape[1])
    dev = _check_tensors("align_step", [("q", q, (B, Nq, 3), torch.float32), ("p", p, (B, Np, 3), torch.float32),
                                     ("state", state, (B, ALIGN_STATE_DOUBLES), torch.float64), ("xf", xf, (B, 12), torch.float32),
                                     ("status", status, (B,), torch.int32), ("idx", idx, (B, Nq), torch.int32), ("d2", d2, (B, Nq), torch.float32),
                                     ("q_count", q_count, (B,), torch.int32), ("p_count", p_count, (B,), torch.int32)])
    scalars = [float(v) for v in (reject, reject_floor, tol, rank_tol, clamp2)]
    if not all(math.isfinite(v) and v >= 0.0 for v in scalars[:3]) or not 0.0 <= scalars[3] < 1.0 or not scalars[4] >= 0.0:
        raise ValueError("align_step: reject, reject_floor, tol >= 0 and finite, rank_tol in [0, 1), clamp2 >= 0; got %r" % (scalars,))
    npart = _lib.size_query("forge_align_partial_doubles", B)
    partial = torch.empty(npart, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().forge_align_step(_lib.ptr(q.detach()), _lib.ptr(p.detach()), _lib.ptr(q_count), _lib.ptr(p_count), _lib.ptr(idx), _lib.ptr(d2),
                                           B, Nq, Np, 1 if with_scale else 0, 1 if update else 0, *scalars, _lib.ptr(partial), _lib.ptr(state),
                                           _lib.ptr(xf), _lib.ptr(status), _lib.current_stream()), "forge_align_step")
    return state, xf, status


@_lib.on_tensor_device
def align_select(state, status, K):
    """forge_align_select (section g5): state [B*K,ALIGN_STATE_DOUBLES] and status [B*K], pair b's K starts in rows b K .. b K + K - 1 -> the start
    of lowest SCORE per pair (the lowest index on a tie; NaN, +inf and a start with ALIGN_EMPTY never win). Returns (T [B,4,4] float64, xf [B,12]
    float32, best [B] int32 (-1: none won, start 0 is reported), state [B,ALIGN_STATE_DOUBLES], status [B]). Nothing is read back."""
    if not torch.is_tensor(state) or not torch.is_tensor(status):
        raise TypeError("align_select: state and status must be tensors")
    _require_cuda(state, status)
    K = int(K)
    if K < 1 or state.dim() != 2 or state.shape[0] < K or state.shape[0] % K:
        raise ValueError("align_select: state must be [B*K,%d] with K=%d >= 1, got %s" % (ALIGN_STATE_DOUBLES, K, tuple(state.shape)))
    B = int(state.shape[0]) // K
    dev = _check_tensors("align_select", [("state", state, (B * K, ALIGN_STATE_DOUBLES), torch.float64), ("status", status, (B * K,), torch.int32)])
    T = torch.empty(B, 4, 4, dtype=torch.float64, device=dev)
    xf = torch.empty(B, 12, dtype=torch.float32, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    state_out = torch.empty(B, ALIGN_STATE_DOUBLES, dtype=torch.float64, device=dev)
    status_out = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().forge_align_select(_lib.ptr(state), _lib.ptr(status), B, K, _lib.ptr(T), _lib.ptr(xf), _lib.ptr(best), _lib.ptr(state_out),
                                             _lib.ptr(status_out), _lib.current_stream()), "forge_align_select")
    return T, xf, best, state_out, status_out


# ---------------------------------------------------------------------------------------------------------------- connected components
COMPONENTS_OVERFLOW = 1                                            # status bit of forge_components_stats (FORGE_COMPONENTS_OVERFLOW)


def components_tile():
    """T, the edge of the cubic tile one workgroup of forge_components_label unions in LDS (host only, no device is touched)."""
    return int(_lib.lib().forge_components_tile())


@_lib.on_tensor_device
def components_label(density, level=0.5, want_labels=True):
    """forge_components_label (include/forge_hip.h section g4): the connected components of `density > level` under the Kuhn adjacency. Returns
    (labels [n,D,H,W] int32 or None, counts [n] int32 on the device, workspace): the workspace (uint8) goes to components_stats and
    components_select together with the same density. Nothing is read back."""
    n, D, H, W, level = _density_volume("components_label", density, level)
    _require_cuda(density)
    nbytes = _lib.size_query("forge_components_workspace_bytes", n, D, H, W)
    dev = density.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty(n, D, H, W, dtype=torch.int32, device=dev) if want_labels else None
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().forge_components_label(_lib.ptr(density.detach()), n, D, H, W, level, _lib.ptr(ws), nbytes, _lib.ptr(labels), _lib.ptr(counts),
                                                 _lib.current_stream()), "forge_components_label")
    return labels, counts, ws


@_lib.on_tensor_device
def components_stats(density, workspace, max_components):
    """forge_components_stats after components_label(density, ...): per component, in label order, with max_components rows per volume:
    (sizes [n,Kmax] int32, bbox [n,Kmax,6] int32 = x0, y0, z0, x1, y1, z1 inclusive, coord_sum [n,Kmax,3] int64, status [n] int32 with
    COMPONENTS_OVERFLOW where a volume has more components than rows). Rows past a volume's count are zero. Nothing is read back."""
    n, D, H, W, _ = _density_volume("components_stats", density)
    kmax = int(max_components)
    if kmax < 0:
        raise ValueError("components_stats: max_components=%d must not be negative" % kmax)
    nbytes = _lib.size_query("forge_components_workspace_bytes", n, D, H, W)
    _check_tensors("components_stats", [("workspace", workspace, nbytes, torch.uint8)], density.device)
    _require_cuda(density, workspace)
    dev = density.device
    sizes = torch.empty(n, kmax, dtype=torch.int32, device=dev)
    bbox = torch.empty(n, kmax, 6, dtype=torch.int32, device=dev)
    coord_sum = torch.empty(n, kmax, 3, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    nz = kmax > 0
    _lib.check(_lib.lib().forge_components_stats(_lib.ptr(workspace), nbytes, n, D, H, W, kmax, _lib.ptr(sizes if nz else None), _lib.ptr(bbox if nz else None),
                                                 _lib.ptr(coord_sum if nz else None), _lib.ptr(status), _lib.current_stream()), "forge_components_stats")
    return sizes, bbox, coord_sum, status


@_lib.on_tensor_device
def components_select(density, workspace, keep_largest=True, min_voxels=1, min_fraction=0.0):
    """forge_components_select after components_label(density, ...): the density with the inside voxels of removed components set to +0.0 and every
    other voxel's bits copied. A component passes with size >= min_voxels and size >= ceil(min_fraction * largest size of its volume);
    keep_largest keeps only the largest passing one (ties: the lowest label). Nothing is read back."""
    n, D, H, W, _ = _density_volume("components_select", density)
    min_voxels, min_fraction = int(min_voxels), float(min_fraction)
    if min_voxels < 1:
        raise ValueError("components_select: min_voxels=%d must be at least 1" % min_voxels)
    if not 0.0 <= min_fraction <= 1.0:
        raise ValueError("components_select: min_fraction=%r must lie in [0, 1]" % min_fraction)
    nbytes = _lib.size_query("forge_components_workspace_bytes", n, D, H, W)
    _check_tensors("components_select", [("workspace", workspace, nbytes, torch.uint8)], density.device)
    _require_cuda(density, workspace)
    out = torch.empty_like(density)
    _lib.check(_lib.lib().forge_components_select(_lib.ptr(density.detach()), n, D, H, W, _lib.ptr(workspace), nbytes, 1 if keep_largest else 0, min_voxels,
                                                  min_fraction, _lib.ptr(out), _lib.current_stream()), "forge_components_select")
    return out
