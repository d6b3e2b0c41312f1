"""Executed-FLOP meter for the matrix-core launches of libforge_hip.so (measurement aid for bench.py / tools; not on the product path).

`with FlopMeter() as m: step()` wraps the ctypes entry points whose work runs on the fp32 MFMA pipe - forge_conv_igemm, forge_wino_gemm (_half, _dn, _dn4, _dn4h, _dn4hw),
forge_conv_wgrad, forge_wino_wgrad, forge_attention_fwd / _fwd_lse / _bwd / _mh_fwd / _mh_bwd, forge_token_linear_fwd / _bwd - for the duration of the block and sums the FLOPs each launch EXECUTES, computed from the call's own
arguments (2 M N taps Cin for a direct / data-gradient / weight-gradient convolution, 2 x 16 R N kd Cin for the 16 Winograd point problems).
Only eager launches made by this process are seen (a hipGraph replay makes no Python calls): meter one eager pass, time the replay.
"""
import torch

from . import _lib
from .convops import WINO_DN4H, WINO_DN4HW, WINO_FORMS


def _v(a):
    return a.value if hasattr(a, "value") else a


def _igemm(a):          # forge_conv_igemm(in1,C1,ld1,bs1,in2,C2,ld2,bs2,wp,bias,scale,shift,slope,residual,aux_h,aux_z,out,out2,out3,n,D,H,W,is,Di,Hi,Wi,Cout,ldo,taps,ntaps,...)
    C1, C2 = _v(a[1]), _v(a[5])
    n, D, H, W, Cout, ntaps = _v(a[19]), _v(a[20]), _v(a[21]), _v(a[22]), _v(a[27]), _v(a[30])
    return 2.0 * n * D * H * W * Cout * ntaps * (C1 + C2)          # merged transposed-conv phases: M rows x ntaps / P taps x P phases = the same product


def _wino_counter(form):    # forge_wino_gemm* (V1,C1,ld1,bs1,pt1,V2,C2,ld2,bs2,pt2,U,Mm,n,D,Ht,Wt,Cout,kd,[tile,]stream): 16 points x R rows x Cout x the form's
    def count(a):           # K loops of Cin per output plane (convops.WINO_FORMS: kd, 2 - four positions per PAIR of planes - or 3/2 - six per FOUR planes);
        loops = _v(a[17]) if form.kloops is None else form.kloops           # WINO_DN4H / WINO_DN4HW: 24 / 36 points on THEIR tile rows = 24 | 36 x 6 x Cin per four planes
        return float(2 * form.points * _v(a[12]) * _v(a[13]) * _v(a[14]) * _v(a[15]) * _v(a[16]) * loops * (_v(a[1]) + _v(a[6])))
    return count


def _wgrad(a):          # forge_conv_wgrad(dy,ldy,x1,C1,ld1,bs1,x2,C2,ld2,bs2,dwp,n,D,H,W,is,Di,Hi,Wi,Cout,taps,ntaps,stream)
    return 2.0 * _v(a[11]) * _v(a[12]) * _v(a[13]) * _v(a[14]) * _v(a[19]) * _v(a[21]) * (_v(a[3]) + _v(a[7]))


def _wino_wgrad(a):     # forge_wino_wgrad(dMm,V1,C1,bs1,pt1,V2,C2,bs2,pt2,dU,n,D,Ht,Wt,Cout,kd,stream)
    return 2.0 * 16 * _v(a[10]) * _v(a[11]) * _v(a[12]) * _v(a[13]) * _v(a[14]) * _v(a[15]) * (_v(a[2]) + _v(a[6]))


def _attention(a):      # forge_attention_fwd(q,k,v,v_batch_rows,out,B,Nq,Nk,d,stream): q k^T and p v
    return 4.0 * _v(a[5]) * _v(a[6]) * _v(a[7]) * _v(a[8])


def _attention_lse(a):  # forge_attention_fwd_lse(q,k,v,v_batch_rows,out,lse,B,Nq,Nk,d,stream): the same two contractions
    return 4.0 * _v(a[6]) * _v(a[7]) * _v(a[8]) * _v(a[9])


def _attention_bwd(a):  # forge_attention_bwd(q,k,v,v_batch_rows,out,lse,dout,dq,dk,dv,delta_ws,B,Nq,Nk,d,stream): S and dP in both passes, dQ, its
    dv = _v(a[9])       # row-residual correction P K, dK and (unless dv is NULL) dV: 8 or 7 contractions of 2 B Nq Nk d
    return (16.0 if dv else 14.0) * _v(a[11]) * _v(a[12]) * _v(a[13]) * _v(a[14])


def _attention_mh(a):   # forge_attention_mh_fwd(q,k,v,out,lse,B,H,Nq,Nk,d,<8 strides>,scale,stream): the two contractions, per head
    return 4.0 * _v(a[5]) * _v(a[6]) * _v(a[7]) * _v(a[8]) * _v(a[9])


def _attention_mh_bwd(a):   # forge_attention_mh_bwd(q,k,v,out,lse,dout,dq,dk,dv,delta_ws,B,H,Nq,Nk,d,<8 strides>,scale,stream): as _attention_bwd, per head
    return (16.0 if _v(a[8]) else 14.0) * _v(a[10]) * _v(a[11]) * _v(a[12]) * _v(a[13]) * _v(a[14])


def _token_fwd(a):      # forge_token_linear_fwd(x,ldx,w,bias,gamma,beta,eps,residual,ldr,y,ldy,pre,stats,R,K,N,act,stream): one R x N x K product
    return 2.0 * _v(a[13]) * _v(a[14]) * _v(a[15])


def _token_bwd(a):      # forge_token_linear_bwd(dy,lddy,x,ldx,w,gamma,beta,stats,pre,dx,dw,dbias,dgamma,dbeta,ws,ws_bytes,R,K,N,act,stream): g W (for dx or
    dxn = _v(a[9]) or _v(a[12]) or _v(a[13])        # the LayerNorm's gradients) and g^T xn (dw), each R x N x K, each only when asked for
    return 2.0 * _v(a[16]) * _v(a[17]) * _v(a[18]) * ((1 if dxn else 0) + (1 if _v(a[10]) else 0))


_ENTRIES = {"forge_conv_igemm": _igemm, **{f.gemm: _wino_counter(f) for f in (*WINO_FORMS.values(), WINO_DN4H, WINO_DN4HW)}, "forge_conv_wgrad": _wgrad, "forge_wino_wgrad": _wino_wgrad,
            "forge_attention_fwd": _attention, "forge_attention_fwd_lse": _attention_lse, "forge_attention_bwd": _attention_bwd,
            "forge_attention_mh_fwd": _attention_mh, "forge_attention_mh_bwd": _attention_mh_bwd,
            "forge_token_linear_fwd": _token_fwd, "forge_token_linear_bwd": _token_bwd}
_wino_gemm, _wino_gemm_dn, _wino_gemm_dn4 = (_ENTRIES[WINO_FORMS[k].gemm] for k in ("points", "dn", "dn4"))      # the counters by form, for the tests


class FlopMeter:
    def __init__(self):
        self.flops = {k: 0.0 for k in _ENTRIES}
        self.launches = {k: 0 for k in _ENTRIES}

    def __enter__(self):
        self._lib = _lib.lib()
        self._orig = {}
        for name, fn in _ENTRIES.items():
            orig = getattr(self._lib, name)
            self._orig[name] = orig

            def wrapped(*a, _orig=orig, _fn=fn, _name=name):
                self.flops[_name] += _fn(a)
                self.launches[_name] += 1
                return _orig(*a)
            setattr(self._lib, name, wrapped)          # instance attribute of the CDLL handle: what `_lib.lib().<name>` resolves to
        return self

    def __exit__(self, *exc):
        for name, orig in self._orig.items():
            setattr(self._lib, name, orig)
        return False

    @property
    def gflop(self):
        return sum(self.flops.values()) / 1e9

    def summary(self):
        return {"executed_gflop": self.gflop, "launches": dict(self.launches), "gflop_by_entry": {k: v / 1e9 for k, v in self.flops.items()}}


def stage_replay_ms(model, sample, dev, iters=20):
    from . import geo_utils
    from .graph import GraphedCall
    """{stage: ms per replay} for FORGE's inference step on `sample` (b scenes, 5 input views, V cameras)."""
    e3 = model.encoder_3d
    b = sample["images"].shape[0]
    t = 5
    with torch.no_grad():
        img = sample["images"][:, :t].reshape(b * t, 3, 256, 256).contiguous()
        lifted = e3._trunk_hip(img)
        feats = e3._conv1_hip(lifted).reshape(b, t, 128, 32, 32, 32)
        poses = sample["cam_poses_cv2_canonicalized"][:, :t].contiguous()
        rotated = model.rotate(voxels=feats, camPoses_cv2=poses, grid_size=32, order="distance")
        fused = e3.fuse(rotated)
        fv, dv = e3.heads(fused)
        V = sample["K_cv2"].shape[1]
        cams = geo_utils.camera_dict(sample["cam_extrinsics_cv2_canonicalized"], sample["K_cv2"])
        v2v = model._view2vol(b, V, dev)
    stages = {
        "encoder_resnet": lambda: e3._trunk_hip(img),
        "encoder_conv1": lambda: e3._conv1_hip(lifted),
        "rotate": lambda: model.rotate(voxels=feats, camPoses_cv2=poses, grid_size=32, order="distance"),
        "fuse": lambda: e3.fuse(rotated),
        "heads": lambda: e3.heads(fused),
        "render(+conv_rgb)": lambda: model.render(cams, fv, dv, return_origin_proj=True, view2vol=v2v),
    }
    out = {}
    for name, fn in stages.items():
        def call(fn=fn):
            with torch.no_grad():
                return fn()
        g = GraphedCall(call, dev, warmup=2)
        g()
        torch.cuda.synchronize()
        a, bq = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            g()
        bq.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(bq) / iters
        del g
    return out
