"""CPU: the multi-head attention pair forge_attention_mh_fwd / forge_attention_mh_bwd (forge_amd/csrc/attention.hip) - the C-ABI exports and
declares it and refuses bad arguments before any launch, the FLOP meter counts it per head, the Python switch (ops.set_multihead_attention) is
off by default and type-checked, and with the switch ON the attention modules of the 2-D pose estimator give, on host tensors, the bits they
give with it off (host tensors, masks and float64 are outside the kernels' domain: the stock statements run)."""
import ctypes
import os

import pytest
import torch

from forge_amd import _lib

NEW = ("forge_attention_mh_fwd", "forge_attention_mh_bwd")


def test_library_exports_and_header_and_signatures_agree(built_lib):
    h = ctypes.CDLL(built_lib)
    for name in NEW:
        assert hasattr(h, name), "libforge_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, name                                   # its types against the header: tests/test_abi_and_surface.py, for every symbol
    assert len(_lib.SIGNATURES["forge_attention_mh_fwd"]) == 20 and len(_lib.SIGNATURES["forge_attention_mh_bwd"]) == 25


def test_argument_refusals_before_any_launch(built_lib):
    """Through fake pointers (never dereferenced: every check runs before the first launch), with the codes of the single-head entry points:
    FORGE_EINVAL = -1, FORGE_ESHAPE = -2."""
    L, fake = _lib.lib(), 0x1000
    dense = lambda Nq, Nk, H: (Nq * H * 64, H * 64, Nk * H * 64, H * 64, Nk * H * 64, H * 64, Nq * H * 64, H * 64)

    def fwd(q=fake, lse=fake, B=1, H=4, Nq=64, Nk=64, d=64, strides=None, scale=0.125):
        return L.forge_attention_mh_fwd(q, fake, fake, fake, lse, B, H, Nq, Nk, d, *(strides or dense(Nq, Nk, H)), scale, None)

    def bwd(q=fake, dq=fake, dv=fake, B=1, H=4, Nq=64, Nk=64, d=64, strides=None, scale=0.125):
        return L.forge_attention_mh_bwd(q, fake, fake, fake, fake, fake, dq, fake, dv, fake, B, H, Nq, Nk, d, *(strides or dense(Nq, Nk, H)), scale, None)

    err = L.forge_last_error
    for call in (fwd, bwd):
        assert call(q=None) == -1 and b"null pointer" in err()
        assert call(d=32) == -2 and b"64 channels" in err()
        assert call(Nq=100) == -2 and b"multiples of 64" in err()
        assert call(Nk=96) == -2 and b"multiples of 64" in err()
        assert call(H=0) == -2 and b"heads" in err()
        for i in range(8):                                                     # every one of the eight strides
            st = list(dense(64, 64, 4))
            st[i] += 2
            assert call(strides=st) == -2 and b"multiples of 4" in err(), i
        assert call(q=fake + 8) == -1 and b"16-byte aligned" in err()
        for scale in (0.0, -0.125, float("inf"), float("nan")):
            assert call(scale=scale) == -1 and b"scale" in err(), scale
    assert bwd(dq=None) == -1 and b"null pointer" in err()
    st = list(dense(64, 64, 4))
    st[7] = 128                                                                # rows of out shorter than H * 64: they would overlap
    assert fwd(strides=st) == -2 and b"overlap" in err()


def test_flopmeter_counts_the_pair_per_head():
    from forge_amd import flopmeter as fm
    assert set(NEW) <= set(fm._ENTRIES)
    B, H, Nq, Nk = 5, 4, 1024, 256
    unit = B * H * Nq * Nk * 64
    strides = (0,) * 8
    assert fm._ENTRIES["forge_attention_mh_fwd"]((0, 0, 0, 0, 0, B, H, Nq, Nk, 64) + strides + (0.125, None)) == 4.0 * unit
    bwd = lambda dv: (0, 0, 0, 0, 0, 0, 0, 0, dv, 0, B, H, Nq, Nk, 64) + strides + (0.125, None)
    assert fm._ENTRIES["forge_attention_mh_bwd"](bwd(ctypes.c_void_p(0x1000))) == 16.0 * unit
    assert fm._ENTRIES["forge_attention_mh_bwd"](bwd(None)) == 14.0 * unit
    assert fm._ENTRIES["forge_attention_mh_fwd"]((0, 0, 0, 0, 0, B, 1, Nq, Nk, 64) + strides + (1.0, None)) * H == 4.0 * unit


def test_switch_is_off_by_default_type_checked_and_returns_the_previous_value():
    from forge_amd import ops
    if os.environ.get("FORGE_ATTENTION_MH", "0") != "1":
        assert ops.multihead_attention() is False                              # the default
    start = ops.multihead_attention()
    prev = ops.set_multihead_attention(True)
    try:
        assert prev is start and ops.multihead_attention() is True
        assert ops.set_multihead_attention(False) is True and ops.multihead_attention() is False
        for bad in (1, 0, None, "1"):
            with pytest.raises(TypeError):
                ops.set_multihead_attention(bad)
        assert ops.multihead_attention() is False                              # a refused value changes nothing
        before = ops.attention_training()                                      # independent of the single-head training switch
        ops.set_multihead_attention(True)
        assert ops.attention_training() is before
        ops.set_attention_training(not before)
        assert ops.multihead_attention() is True
        ops.set_attention_training(before)
    finally:
        ops.set_multihead_attention(prev)
    assert ops.multihead_attention() is start


def test_predicate_and_ops_refuse_host_tensors():
    from forge_amd import ops
    q = torch.zeros(1, 64, 256)
    prev = ops.set_multihead_attention(True)
    try:
        assert not ops.attention_mh_applies(q, q, q, 4)                        # a host tensor: the module keeps torch's own ops
        meta = torch.empty(1, 64, 256, device="meta")
        assert not ops.attention_mh_applies(meta, meta, meta, 4)
        for fn in (ops.attention_mh, ops.attention_mh_train):
            with pytest.raises(RuntimeError, match=r"on the MI355X.*q \(1, 64, 256\)"):
                fn(q, q, q, 4, 0.125)
    finally:
        ops.set_multihead_attention(prev)


def test_modules_on_host_tensors_give_the_same_bits_with_the_switch_on():
    from forge_amd import ops
    from forge_amd.pose_estimator_2d import CrossAttention, MultiHeadAttention, SelfAttention
    torch.manual_seed(1)
    mha, cross, selfa = MultiHeadAttention(4, 256, 256), CrossAttention(4, 256, 256, mlp_ratio=4), SelfAttention(4, 256, mlp_ratio=4)
    g = torch.Generator().manual_seed(2)
    feat, canon = torch.randn(2, 128, 256, generator=g), torch.randn(2, 64, 256, generator=g)
    mask = torch.zeros(2, 64, dtype=torch.bool)
    mask[:, 40:] = True

    def evaluate():
        outs = []
        for grad in (False, True):
            with torch.set_grad_enabled(grad):
                outs += [mha(feat, canon, canon), mha(feat, canon, canon, pad_mask=mask), cross(x_q=feat, x_k=canon, x_v=canon, residual=feat),
                         cross(x_q=feat, x_k=canon, x_v=canon, pad_mask=mask), selfa(feat), mha.double()(feat.double(), canon.double(), canon.double())]
                mha.float()
        return [o.detach() for o in outs]

    prev = ops.set_multihead_attention(False)
    try:
        off = evaluate()
        ops.set_multihead_attention(True)
        called = []
        orig = ops.attention_mh, ops.attention_mh_train
        ops.attention_mh = ops.attention_mh_train = lambda *a, **kw: called.append(a)
        try:
            on = evaluate()
            with pytest.raises(NotImplementedError):
                mha(feat, canon, canon, attn_mask=mask)                        # as with the switch off
        finally:
            ops.attention_mh, ops.attention_mh_train = orig
    finally:
        ops.set_multihead_attention(prev)
    assert not called
    assert len(on) == len(off) == 12 and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(on, off))
    assert not torch.equal(off[0], off[1])                                     # the mask is not ignored
