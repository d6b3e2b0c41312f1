"""CPU: the differentiable attention pair forge_attention_fwd_lse / forge_attention_bwd (forge_amd/csrc/attention.hip) - the C-ABI exports and
declares it, the Python surface (ops.attention_train, ops.attention_train_applies, ops.set_attention_training) refuses what it cannot run, and
the algebra the kernels hard-code holds: a float64 restatement of their tile walks (32-key / 32-query tiles, base-2 online softmax and its
log-sum-exp, delta, dS = P o (dP - delta), the three accumulations with the parts of a split added in a fixed order, the row-residual correction) against torch's autograd
of softmax-then-matmul."""
import ctypes
import math
import os
import re

import pytest
import torch

from forge_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("forge_attention_fwd_lse", "forge_attention_bwd")


def test_library_exports_and_header_declares_the_pair(built_lib):
    h = ctypes.CDLL(built_lib)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "forge_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(h, name), "libforge_hip.so does not export %s" % name
        assert re.search(r"\bint\s+%s\s*\(" % name, src), "include/forge_hip.h does not declare %s" % name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["forge_attention_fwd_lse"]) == 11 and len(_lib.SIGNATURES["forge_attention_bwd"]) == 16
    # argument checks run before any launch: no GPU needed (the pointers are never dereferenced)
    L, fake = _lib.lib(), 0x1000
    assert L.forge_attention_fwd_lse(fake, fake, fake, 64, fake, None, 1, 64, 64, 64, None) == -1 and b"null pointer" in L.forge_last_error()
    assert L.forge_attention_fwd_lse(fake, fake, fake, 64, fake, fake, 1, 100, 64, 64, None) == -2 and b"multiples of 64" in L.forge_last_error()
    assert L.forge_attention_bwd(*([fake, fake, fake, 64] + [fake] * 7 + [1, 64, 100, 64, None])) == -2 and b"multiples of 64" in L.forge_last_error()
    assert L.forge_attention_bwd(*([fake, fake, fake, 64] + [fake] * 7 + [1, 64, 64, 32, None])) == -2 and b"64 channels" in L.forge_last_error()
    assert L.forge_attention_bwd(*([fake, fake, fake, 0] + [fake] * 7 + [2, 64, 64, 64, None])) == -1 and b"shared" in L.forge_last_error()


def test_flopmeter_counts_the_pair_by_what_it_executes():
    from forge_amd import flopmeter as fm
    assert set(NEW) <= set(fm._ENTRIES)
    B, Nq, Nk = 4, 4096, 2048
    unit = B * Nq * Nk * 64
    fwd = (0, 0, 0, Nk, 0, 0, B, Nq, Nk, 64, None)
    assert fm._ENTRIES["forge_attention_fwd_lse"](fwd) == 4.0 * unit
    bwd = lambda dv: (0, 0, 0, Nk, 0, 0, 0, 0, 0, dv, 0, B, Nq, Nk, 64, None)
    assert fm._ENTRIES["forge_attention_bwd"](bwd(ctypes.c_void_p(0x1000))) == 16.0 * unit
    assert fm._ENTRIES["forge_attention_bwd"](bwd(None)) == 14.0 * unit


def test_surface_is_off_by_default_and_refuses_cpu_tensors():
    from forge_amd import ops
    q = torch.zeros(1, 64, 64)
    if os.environ.get("FORGE_ATTENTION_TRAIN", "0") != "1":
        assert ops.attention_training() is False                               # the default
    prev = ops.set_attention_training(True)
    try:
        assert ops.attention_training() is True
        assert not ops.attention_train_applies(q, q, q)                        # a CPU tensor: the caller keeps torch's own ops
        with pytest.raises(RuntimeError, match="on the MI355X"):
            ops.attention_train(q, q, q)
        assert ops.set_attention_training(False) is True
        meta = torch.empty(2, 64, 64, device="meta")                           # switch off: False whatever the tensors
        assert not ops.attention_train_applies(q, q, q) and not ops.attention_train_applies(meta, meta, meta)
        with pytest.raises(TypeError):
            ops.set_attention_training(1)
    finally:
        ops.set_attention_training(prev)
    assert ops.attention_training() is prev


# ---- the kernels' walks in float64

LOG2E = 1.0 / math.log(2.0)


def acc_rows(tile):
    """The row order of a 32 x 32 fp32 MFMA accumulator: register r of half-wave h holds row 8 (r / 4) + 4 h + r % 4. The contractions that take an
    accumulator as their B operand run over the rows in this order (step r contracts the two halves' rows)."""
    return [tile + 8 * (r // 4) + 4 * h + r % 4 for r in range(16) for h in range(2)]


def tiled_forward(q, k, v, parts):
    """attention_fwd_kernel: per query tile and key part an online softmax in base 2 over 32-key tiles; the parts merged with their maxima; lse from
    the merged M and den."""
    Nq, Nk = q.shape[0], k.shape[0]
    out, lse = torch.empty(Nq, 64, dtype=q.dtype), torch.empty(Nq, dtype=q.dtype)
    for q0 in range(0, Nq, 32):
        q2 = q[q0:q0 + 32] * LOG2E
        state = []
        for p in range(parts):
            m, l, o = torch.full((32,), -math.inf, dtype=q.dtype), torch.zeros(32, dtype=q.dtype), torch.zeros(32, 64, dtype=q.dtype)
            for kt in range(p * Nk // parts, (p + 1) * Nk // parts, 32):
                s = q2 @ k[kt:kt + 32].T
                mn = torch.maximum(m, s.max(dim=1).values)
                sc = torch.exp2(m - mn)
                pt = torch.exp2(s - mn[:, None])
                l = l * sc + pt.sum(dim=1)
                rows = [r - kt for r in acc_rows(kt)]
                o = o * sc[:, None] + pt[:, rows] @ v[kt:kt + 32][rows]
                m = mn
            state.append((m, l, o))
        M = torch.stack([m for m, _, _ in state]).max(dim=0).values
        den = sum(l * torch.exp2(m - M) for m, l, _ in state)
        out[q0:q0 + 32] = sum(o * torch.exp2(m - M)[:, None] for m, _, o in state) / den[:, None]
        lse[q0:q0 + 32] = (M + torch.log2(den)) * math.log(2.0)
    return out, lse


def tiled_backward(q, k, v, out, lse, dout, parts_k, parts_q, want_dv):
    """attention_delta_kernel, attention_bwd_dq_kernel (query tiles walk key tiles) and attention_bwd_dkv_kernel (key tiles walk query tiles); the
    parts of a split are added in their order."""
    Nq, Nk = q.shape[0], k.shape[0]
    delta = (dout * out).sum(dim=1).clone()
    P = lambda s2, rows: torch.exp2(s2 - lse[rows][:, None] * LOG2E)           # the logits in base 2, as the forward has them
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(k) if want_dv else None
    for q0 in range(0, Nq, 32):
        rows, acc = slice(q0, q0 + 32), []
        for p in range(parts_k):
            a, bk, rs, zs = torch.zeros(32, 64, dtype=q.dtype), torch.zeros(32, 64, dtype=q.dtype), torch.zeros(32, dtype=q.dtype), torch.zeros(32, dtype=q.dtype)
            for kt in range(p * Nk // parts_k, (p + 1) * Nk // parts_k, 32):
                pt = P((q[rows] * LOG2E) @ k[kt:kt + 32].T, rows)
                ds = pt * (dout[rows] @ v[kt:kt + 32].T - delta[rows][:, None])
                order = [r - kt for r in acc_rows(kt)]
                a = a + ds[:, order] @ k[kt:kt + 32][order]
                bk = bk + pt[:, order] @ k[kt:kt + 32][order]
                rs, zs = rs + ds.sum(dim=1), zs + pt.sum(dim=1)
            acc.append((a, bk, rs, zs))
        a, bk, rs, zs = (sum(x[1:], x[0]) for x in zip(*acc))
        rho = rs / zs                                                           # the row residual of dS over its softmax mass: 0 in exact arithmetic
        dq[rows] = a - rho[:, None] * bk
        delta[rows] += rho                                                      # what the dK / dV pass reads
    for k0 in range(0, Nk, 32):
        keys, acc_k, acc_v = slice(k0, k0 + 32), [], []
        for p in range(parts_q):
            ak, av = torch.zeros(32, 64, dtype=q.dtype), torch.zeros(32, 64, dtype=q.dtype)
            for qt in range(p * Nq // parts_q, (p + 1) * Nq // parts_q, 32):
                rows = acc_rows(qt)                                             # lse and delta are indexed by accumulator register here
                pt = P((q[rows] * LOG2E) @ k[keys].T, rows)
                ds = pt * (dout[rows] @ v[keys].T - delta[rows][:, None])
                av = av + pt.T @ dout[rows]
                ak = ak + ds.T @ q[rows]
            acc_k.append(ak)
            acc_v.append(av)
        dk[keys] = sum(acc_k[1:], acc_k[0])
        if want_dv:
            dv[keys] = sum(acc_v[1:], acc_v[0])
    return dq, dk, dv


@pytest.mark.parametrize("B,Nq,Nk", [(2, 128, 192), (1, 64, 64)])
@pytest.mark.parametrize("shared", [False, True])
def test_tiled_algebra_matches_autograd_in_float64(B, Nq, Nk, shared):
    g = torch.Generator().manual_seed(B * 1000 + Nq + Nk + int(shared))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q, k, dout = (rnd(B, Nq, 64) * 0.5).requires_grad_(True), (rnd(B, Nk, 64) * 0.5).requires_grad_(True), rnd(B, Nq, 64)
    v = rnd(1 if shared else B, Nk, 64).requires_grad_(not shared)             # the shared table is a constant
    want = torch.matmul(torch.matmul(q, k.transpose(1, 2)).softmax(dim=-1), v)
    want_lse = torch.logsumexp(torch.matmul(q, k.transpose(1, 2)), dim=-1)
    grads = torch.autograd.grad(want, [q, k] + ([] if shared else [v]), dout)
    rel = lambda got, ref: ((got - ref).abs().max() / ref.abs().max()).item()
    parts_k = 4 if Nk % 128 == 0 else 2                                        # the launch rule at these sizes (few tiles: 4 parts where they divide)
    parts_q = 4 if Nq % 128 == 0 else 2
    with torch.no_grad():
        for b in range(B):
            vb = v[0 if shared else b]
            out, lse = tiled_forward(q[b], k[b], vb, parts_k)
            assert rel(out, want[b]) < 1e-12 and rel(lse, want_lse[b]) < 1e-12
            dq, dk, dv = tiled_backward(q[b], k[b], vb, out, lse, dout[b], parts_k, parts_q, not shared)
            assert rel(dq, grads[0][b]) < 1e-12 and rel(dk, grads[1][b]) < 1e-12
            assert dv is None if shared else rel(dv, grads[2][b]) < 1e-12
