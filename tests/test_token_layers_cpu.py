"""CPU: the token-row layers forge_token_linear_fwd / _bwd and forge_layer_norm_fwd / _bwd (forge_amd/csrc/token.hip) - the C-ABI exports and
declares them and refuses bad arguments before any launch, the row-chunk plan and the workspace size are host arithmetic on the shape alone,
the FLOP meter counts the GEMM entry points, the Python switch (ops.set_token_layers) is off by default and type-checked, and with the switch ON the
blocks of both pose estimators give, on host tensors, the bits they give with it off (host tensors and float64 are outside the kernels' domain: the
stock statements run)."""
import ctypes
import os
import re

import pytest
import torch

from forge_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("forge_token_linear_fwd", "forge_layer_norm_fwd", "forge_token_rows_plan", "forge_token_linear_bwd_ws_bytes", "forge_token_linear_bwd",
       "forge_layer_norm_bwd_ws_bytes", "forge_layer_norm_bwd")
DET_SLAB_BYTES = 64 << 20                                                       # csrc/common.h


def test_library_exports_and_header_and_signatures_agree(built_lib):
    h = ctypes.CDLL(built_lib)
    for name in NEW:
        assert hasattr(h, name), "libforge_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, name                                   # its types against the header: tests/test_abi_and_surface.py, for every symbol
        assert name.endswith("_ws_bytes") == (name in _lib._LL_RESULTS), name   # the two byte counts are long long, the other five results int
    assert len(_lib.SIGNATURES["forge_token_linear_fwd"]) == 18 and len(_lib.SIGNATURES["forge_token_linear_bwd"]) == 21


def test_argument_refusals_before_any_launch(built_lib):
    """Through fake pointers (never dereferenced: every check runs before the first launch): FORGE_EINVAL = -1, FORGE_ESHAPE = -2."""
    L, fake = _lib.lib(), 0x1000
    err = L.forge_last_error

    def fwd(x=fake, w=fake, y=fake, gamma=None, stats=None, ldx=None, ldy=None, res=None, ldr=0, R=40, K=64, N=128, act=0, eps=1e-5):
        return L.forge_token_linear_fwd(x, K if ldx is None else ldx, w, fake, gamma, gamma, eps, res, ldr, y, N if ldy is None else ldy, None, stats,
                                        R, K, N, act, None)

    def bwd(dy=fake, x=fake, w=fake, gamma=None, pre=None, dx=fake, dw=fake, db=fake, dg=None, ws=fake, ws_bytes=1 << 40, lddy=None, R=40, K=64, N=128, act=0):
        return L.forge_token_linear_bwd(dy, N if lddy is None else lddy, x, K, w, gamma, gamma, gamma, pre, dx, dw, db, dg, dg, ws, ws_bytes, R, K, N, act, None)

    for call in (fwd, bwd):
        for arg in ("x", "w", "y" if call is fwd else "dy"):
            assert call(**{arg: None}) == -1 and b"null pointer" in err(), arg
        for bad in (dict(K=96), dict(N=100), dict(K=32), dict(K=1088), dict(N=2048)):
            assert call(**bad) == -2 and b"multiples of 64" in err(), bad
        assert call(K=320, gamma=fake) == -2 and b"LayerNorm over K=320" in err()              # a LayerNorm over more than 256 channels
        assert call(R=0) == -1 and b"rows" in err()
        assert call(R=-3) == -1 and b"rows" in err()
        assert call(act=2) == -1 and b"act=2" in err()
        assert call(x=fake + 8) == -1 and b"16-byte aligned" in err()
    assert fwd(ldx=66) == -2 and b"x row stride 66" in err()                                   # not a multiple of 4
    assert fwd(ldx=60) == -2 and b"x row stride" in err()                                      # shorter than the row
    assert fwd(ldy=130) == -2 and b"y row stride 130" in err()
    assert fwd(res=fake, ldr=126) == -2 and b"residual row stride" in err()
    assert fwd(stats=fake) == -1 and b"stats without" in err()
    assert fwd(gamma=fake, eps=float("nan")) == -1 and b"eps" in err()
    assert bwd(lddy=130) == -2 and b"dy row stride 130" in err()
    assert bwd(act=1) == -1 and b"pre-activation" in err()
    assert bwd(dg=fake) == -1 and b"without a LayerNorm" in err()
    assert bwd(dw=None) == -1 and b"by-product" in err()
    # a workspace smaller than the plan asks for (R = 16384: 128 chunks of dW and dbias; with the LayerNorm also dxn and its slabs)
    for ln in (0, 1):
        need = L.forge_token_linear_bwd_ws_bytes(16384, 64, 64, ln)
        assert need > 0
        g = fake if ln else None
        assert bwd(R=16384, N=64, gamma=g, ws_bytes=need - 4) == -1 and b"workspace" in err()
        assert bwd(R=16384, N=64, gamma=g, ws=None) == -1 and b"workspace" in err()
    # the stand-alone LayerNorm
    ln_fwd = lambda x=fake, ldx=64, R=40, K=64: L.forge_layer_norm_fwd(x, ldx, fake, fake, 1e-5, fake, K, None, R, K, None)
    ln_bwd = lambda dy=fake, dg=fake, ws=fake, ws_bytes=1 << 40, R=40, K=64: L.forge_layer_norm_bwd(dy, K, fake, K, fake, fake, fake, dg, dg, ws, ws_bytes, R, K, None)
    assert ln_fwd(x=None) == -1 and ln_fwd(K=320) == -2 and ln_fwd(K=96) == -2 and ln_fwd(ldx=66) == -2 and ln_fwd(R=0) == -1
    assert ln_bwd(dy=None) == -1 and ln_bwd(K=320) == -2 and ln_bwd(R=0) == -1
    assert ln_bwd(ws_bytes=L.forge_layer_norm_bwd_ws_bytes(40, 64) - 4) == -1 and b"workspace" in err()
    assert L.forge_token_linear_bwd_ws_bytes(40, 96, 64, 0) == -1 and L.forge_layer_norm_bwd_ws_bytes(40, 320) == -1


def test_row_plan_and_workspace_depend_on_the_shape_alone(built_lib):
    from forge_amd import ops
    L = _lib.lib()
    chunks, rows = ops.token_rows_plan(16384, 64, 64)                              # one scene's 3-D rows: cannot be one workgroup
    assert chunks > 1 and chunks * rows >= 16384 > (chunks - 1) * rows and rows % 32 == 0
    assert chunks * 64 * 64 * 4 <= DET_SLAB_BYTES
    c2, r2 = ops.token_rows_plan(1024, 256, 1024)                                  # the 2-D fc1: few chunks
    assert 1 <= c2 <= 8 and c2 * r2 >= 1024 and c2 * 1024 * 256 * 4 <= DET_SLAB_BYTES
    assert ops.token_rows_plan(128, 64, 64) == (1, 128) and ops.token_rows_plan(129, 64, 64) == (2, 128)     # the first multi-chunk row count
    assert ops.token_rows_plan(1, 64, 64) == (1, 128)
    for R in (1, 100, 1024, 4096, 16384, 65536):
        for K, N in ((64, 64), (64, 128), (256, 256), (256, 1024), (1024, 256), (1024, 1024)):
            c, r = ops.token_rows_plan(R, K, N)
            assert ops.token_rows_plan(R, K, N) == (c, r)                          # the same answer every time
            assert c >= 1 and r % 32 == 0 and c * r >= R > (c - 1) * r and (c == 1 or c * K * N * 4 <= DET_SLAB_BYTES), (R, K, N)
            plain, with_ln = L.forge_token_linear_bwd_ws_bytes(R, K, N, 0), (L.forge_token_linear_bwd_ws_bytes(R, K, N, 1) if K <= 256 else None)
            assert plain == (c * (N * K + N) * 4 if c > 1 else 0), (R, K, N)
            if with_ln is not None:
                assert with_ln == plain + R * K * 4 + L.forge_layer_norm_bwd_ws_bytes(R, K) and L.forge_layer_norm_bwd_ws_bytes(R, K) % (2 * K * 4) == 0
    with pytest.raises(RuntimeError, match="forge_token_rows_plan"):
        ops.token_rows_plan(0, 64, 64)


def test_flopmeter_counts_the_new_calls():
    from forge_amd import flopmeter as fm
    assert {"forge_token_linear_fwd", "forge_token_linear_bwd"} <= set(fm._ENTRIES)
    R, K, N = 1000, 256, 1024
    p = ctypes.c_void_p(0x1000)
    assert fm._ENTRIES["forge_token_linear_fwd"]((0, K, 0, 0, 0, 0, 1e-5, 0, 0, 0, N, 0, 0, R, K, N, 1, None)) == 2.0 * R * K * N
    bwd = lambda dx, dw, dg: (0, N, 0, K, 0, 0, 0, 0, 0, dx, dw, None, dg, None, 0, 0, R, K, N, 0, None)
    assert fm._ENTRIES["forge_token_linear_bwd"](bwd(p, p, None)) == 4.0 * R * K * N
    assert fm._ENTRIES["forge_token_linear_bwd"](bwd(None, p, None)) == 2.0 * R * K * N
    assert fm._ENTRIES["forge_token_linear_bwd"](bwd(None, None, p)) == 2.0 * R * K * N         # dgamma alone still needs g W
    assert fm._ENTRIES["forge_token_linear_bwd"](bwd(None, None, None)) == 0.0
    m = fm.FlopMeter()
    assert m.launches["forge_token_linear_fwd"] == 0 and m.flops["forge_token_linear_bwd"] == 0.0


def test_switch_is_off_by_default_type_checked_and_returns_the_previous_value():
    from forge_amd import ops
    if os.environ.get("FORGE_TOKEN_LAYERS", "0") != "1":
        assert ops.token_layers() is False                                     # the default
    start = ops.token_layers()
    prev = ops.set_token_layers(True)
    try:
        assert prev is start and ops.token_layers() is True
        assert ops.set_token_layers(False) is True and ops.token_layers() is False
        for bad in (1, 0, None, "1"):
            with pytest.raises(TypeError):
                ops.set_token_layers(bad)
        assert ops.token_layers() is False                                     # a refused value changes nothing
        before = ops.attention_training(), ops.multihead_attention()           # independent of the two attention switches
        ops.set_token_layers(True)
        assert (ops.attention_training(), ops.multihead_attention()) == before
        ops.set_attention_training(not before[0]), ops.set_multihead_attention(not before[1])
        assert ops.token_layers() is True
        ops.set_attention_training(before[0]), ops.set_multihead_attention(before[1])
    finally:
        ops.set_token_layers(prev)
    assert ops.token_layers() is start


def test_sites_left_on_torch_are_named_sites():
    from forge_amd import ops
    src = "".join(open(os.path.join(ROOT, "forge_amd", f)).read() for f in ("pose_estimator_2d.py", "pose_estimator_3d.py"))
    sites = set(re.findall(r'"([23]d\.[a-z_0-9]+)"', src))
    assert sites == {"2d.proj", "2d.o_proj", "2d.fc1", "2d.fc2", "2d.norm", "3d.qk", "3d.v", "3d.fc1", "3d.fc2"}
    assert isinstance(ops.TOKEN_SITES_ON_TORCH, frozenset) and ops.TOKEN_SITES_ON_TORCH <= sites


def test_predicate_and_ops_refuse_host_tensors():
    from forge_amd import ops
    x, w, b, g = torch.zeros(2, 40, 64), torch.zeros(128, 64), torch.zeros(128), torch.ones(64)
    prev = ops.set_token_layers(True)
    try:
        assert not ops.token_layers_applies(x, w, b) and not ops.token_layers_applies(x, w, b, (g, g, 1e-5), "gelu")
        assert not ops.token_layers_applies(x, ln=(g, g, 1e-5))
        meta = lambda *s: torch.empty(*s, device="meta")
        assert not ops.token_layers_applies(meta(2, 40, 64), meta(128, 64), meta(128))
        assert ops.module_token_linear(x, w, b) is None and ops.module_layer_norm(x, torch.nn.LayerNorm(64)) is None
        for fn in (ops.token_linear, ops.token_linear_train):
            with pytest.raises(RuntimeError, match=r"on the MI355X.*x \(2, 40, 64\) float32"):
                fn(x, w, b)
        for fn in (ops.layer_norm, ops.layer_norm_train):
            with pytest.raises(RuntimeError, match=r"on the MI355X.*x \(2, 40, 64\) float32"):
                fn(x, g, g)
    finally:
        ops.set_token_layers(prev)


def test_blocks_on_host_tensors_give_the_same_bits_with_the_switch_on(monkeypatch):
    from forge_amd import ops
    from forge_amd.pose_estimator_2d import CrossAttention, SelfAttention
    from forge_amd.pose_estimator_3d import Block
    torch.manual_seed(1)
    cross, selfa, blk = CrossAttention(4, 256, 256, mlp_ratio=4), SelfAttention(4, 256, mlp_ratio=4), Block(dim=64, mlp_ratio=2)
    g = torch.Generator().manual_seed(2)
    feat, canon = torch.randn(2, 128, 256, generator=g), torch.randn(2, 64, 256, generator=g)
    q3, k3 = torch.randn(2, 64, 128, generator=g), torch.randn(2, 64, 128, generator=g)
    mask = torch.zeros(2, 64, dtype=torch.bool)
    mask[:, 40:] = True

    def evaluate():
        outs = []
        for grad in (False, True):
            with torch.set_grad_enabled(grad):
                outs += [cross(x_q=feat, x_k=canon, x_v=canon, residual=feat), cross(x_q=feat, x_k=canon, x_v=canon, pad_mask=mask),
                         cross(x_q=feat, x_k=canon, x_v=canon, residual=True), selfa(feat), selfa.double()(feat.double()),
                         blk(q3, k3), blk.forward_tokens(q3.permute(0, 2, 1), k3.permute(0, 2, 1)), blk.get_attn(q3, k3)]
                selfa.float()
        return [o.detach() for o in outs]

    prev = ops.set_token_layers(False)
    try:
        off = evaluate()
        ops.set_token_layers(True)
        called = []
        for name in ("token_linear", "token_linear_train", "layer_norm", "layer_norm_train"):
            monkeypatch.setattr(ops, name, lambda *a, **kw: called.append(a))
        on = evaluate()
        with pytest.raises(NotImplementedError):
            cross(x_q=feat, x_k=canon, x_v=canon, attn_mask=mask)               # as with the switch off
    finally:
        ops.set_token_layers(prev)
    assert not called
    assert len(on) == len(off) == 16 and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(on, off))


def test_switch_off_never_reaches_the_library(monkeypatch):
    """With the switch off the dispatch helpers answer None before looking at their arguments."""
    from forge_amd import ops
    prev = ops.set_token_layers(False)
    try:
        monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was called"))
        assert ops.module_token_linear(object(), None, None) is None and ops.module_layer_norm(object(), None) is None
        assert not ops.token_layers_applies(object())
    finally:
        ops.set_token_layers(prev)
