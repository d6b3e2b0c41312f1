"""GPU (-m gpu): multi-head attention of the 2-D pose estimator on the project's kernels - ops.attention_mh / ops.attention_mh_train =
forge_attention_mh_fwd / forge_attention_mh_bwd (forge_amd/csrc/attention.hip), opt-in through ops.set_multihead_attention.

The addressing is pinned apart from the arithmetic: for power-of-two scales the forward equals the single-head kernel on head-split copies bit
for bit. The arithmetic: out, lse and dq / dk / dv against float64 evaluations of bmm - scale - softmax - bmm on the GPU with torch's fp32 ops as
the yardstick and the rule of tests/test_gpu_attention_bwd.py, error / max <= 2 x torch's + 1e-6. Then: bitwise reproducible in either determinism
mode, capturable into a hipGraph, no [B*H,Nq,Nk] matrix in peak memory, refusals outside the domain, and the wiring into MultiHeadAttention
(CrossAttention + SelfAttention gradients, the whole PoseEstimator2D).

FORGE_TEST_REPORT=1 prints every measured ratio."""
import copy
import os

import pytest
import torch

import forge_amd
from forge_amd import _lib, ops, synthetic as syn

pytestmark = pytest.mark.gpu

#        B, H, Nq,   Nk,   scale, q / k / v slices of one [B,N,3 H 64] tensor
CASES = [(1, 1, 64, 64, 1.0, False),           # the smallest tile: two key parts of 32
         (1, 4, 256, 256, 0.125, False),       # T = 2: the smallest shape the module produces
         (2, 3, 192, 128, 0.125, False),       # odd head count; four key parts forward, two query parts backward
         (1, 4, 1024, 256, 0.125, False),      # one scene's cross attention
         (1, 4, 1024, 1024, 0.125, False),     # one scene's self attention
         (8, 4, 1024, 256, 0.37, False),       # 512 query tiles: the two-part kernels; a scale that is not a power of two
         (2, 4, 128, 128, 0.125, True)]        # row stride 768, not H 64 = 256
IDS = ["%dx%dx%dx%d_s%g%s" % (B, H, Nq, Nk, s, "_sliced" if sl else "") for B, H, Nq, Nk, s, sl in CASES]
FACTOR = 2.0                                   # eh <= FACTOR * et + 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture()
def switch_on():
    prev = ops.set_multihead_attention(True)
    yield
    ops.set_multihead_attention(prev)


def report(line):
    if os.environ.get("FORGE_TEST_REPORT"):
        print("  " + line)


def rel(got, want):
    return (got.double() - want).abs().max().item() / want.abs().max().item()


def heads(x, H):
    """The [B*H,N,64] contiguous copy MultiHeadAttention._heads makes."""
    b, n, c = x.shape
    return x.reshape(b, n, H, c // H).permute(0, 2, 1, 3).reshape(b * H, n, -1)


def merge(o, H):
    """... and the head merge behind the second bmm: [B*H,N,64] -> [B,N,H*64]."""
    b = o.shape[0] // H
    return o.reshape(b, H, o.shape[1], -1).permute(0, 2, 1, 3).reshape(b, o.shape[1], -1)


def stock(q, k, v, H, scale):
    attn = (torch.bmm(heads(q, H), heads(k, H).transpose(1, 2)) * scale).softmax(dim=-1)
    return merge(torch.bmm(attn, heads(v, H)), H)


def stock_lse(q, k, H, scale):
    return torch.logsumexp(torch.bmm(heads(q, H), heads(k, H).transpose(1, 2)) * scale, dim=-1).reshape(q.shape[0], H, q.shape[1])


def inputs(dev, case):
    B, H, Nq, Nk, scale, sliced = case
    g = torch.Generator(device=dev).manual_seed(31 + CASES.index(case))
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    gain = scale ** -0.5                                                    # logits of the spread the module sees, whatever the scale
    if sliced:
        qkv = rnd(B, Nq, 3 * H * 64)
        q, k, v = (qkv[:, :, i * H * 64:(i + 1) * H * 64] for i in range(3))
        q, k = q * gain, k * gain * 0.5
        qkv = torch.cat([q, k, v], dim=2)
        q, k, v = (qkv[:, :, i * H * 64:(i + 1) * H * 64] for i in range(3))
        assert q.stride(1) == 3 * H * 64 and not q.is_contiguous()
    else:
        q, k, v = rnd(B, Nq, H * 64) * gain, rnd(B, Nk, H * 64) * gain * 0.5, rnd(B, Nk, H * 64)
    return q, k, v, rnd(B, Nq, H * 64)


_RUNS = {}


def run(dev, case):
    """One evaluation per case, shared by the tests and left unchanged: the kernels' out / lse / gradients, float64 and torch-fp32 references."""
    if case in _RUNS:
        return _RUNS[case]
    B, H, Nq, Nk, scale, sliced = case
    q, k, v, dout = inputs(dev, case)

    def leaves(dt):
        if sliced and dt == torch.float32:                                  # leaves that are views of one tensor, as a fused projection would hand over
            base = torch.cat([q, k, v], dim=2).requires_grad_(True)
            return base, [base[:, :, i * H * 64:(i + 1) * H * 64] for i in range(3)]
        ls = [t.clone().to(dt).requires_grad_(True) for t in (q, k, v)]
        return None, ls

    r = {"q": q, "k": k, "v": v, "dout": dout}
    base, ls = leaves(torch.float32)
    out = ops.attention_mh_train(*ls, H, scale)
    if base is None:
        r["grads"] = torch.autograd.grad(out, ls, dout)
    else:
        gb, = torch.autograd.grad(out, base, dout)
        r["grads"] = tuple(gb[:, :, i * H * 64:(i + 1) * H * 64] for i in range(3))
    r["out"] = out.detach()
    _, ls = leaves(torch.float64)
    out64 = stock(*ls, H, scale)
    r["grads64"] = torch.autograd.grad(out64, ls, dout.double())
    r["out64"] = out64.detach()
    ls = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out32 = stock(*ls, H, scale)
    r["grads32"] = torch.autograd.grad(out32, ls, dout)
    r["out32"] = out32.detach()
    with torch.no_grad():
        r["lse32"] = stock_lse(q, k, H, scale)
        r["lse64"] = stock_lse(q.double(), k.double(), H, scale)
    _RUNS[case] = r
    return r


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_is_the_single_head_kernel_on_head_split_copies_bitwise(dev, case):
    B, H, Nq, Nk, scale, sliced = case
    r = run(dev, case)
    with torch.no_grad():
        got = ops.attention_mh(r["q"], r["k"], r["v"], H, scale)
        assert got.shape == (B, Nq, H * 64) and got.is_contiguous()
        assert torch.equal(got, r["out"])                                               # with and without the lse store: the same bits
        if scale not in (1.0, 0.125):
            return                                                                      # not a power of two: q * scale rounds, the arithmetic tests cover it
        want = merge(ops.attention(heads(r["q"], H) * scale, heads(r["k"], H).contiguous(), heads(r["v"], H).contiguous()), H)
        assert torch.equal(got, want)
        if H == 1 and scale == 1.0:
            assert torch.equal(got, ops.attention(r["q"], r["k"], r["v"]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_lse_vs_float64(dev, case):
    B, H, Nq, Nk, scale, sliced = case
    r = run(dev, case)
    out, lse = ops._mh_forward(r["q"], r["k"], r["v"], H, scale, True)
    assert lse.shape == (B, H, Nq) and torch.equal(out, r["out"])
    for name, got, t32, want in (("out", out, r["out32"], r["out64"]), ("lse", lse, r["lse32"], r["lse64"])):
        eh, et = rel(got, want), rel(t32, want)
        report("attention_mh %s %s: hip/f64 %.2e torch/f64 %.2e" % (IDS[CASES.index(case)], name, eh, et))
        assert eh <= FACTOR * et + 1e-6, (case, name, eh, et)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_vs_float64_with_torch_fp32_as_yardstick(dev, case):
    r = run(dev, case)
    bad = []
    for name, got, t32, want in zip(("dq", "dk", "dv"), r["grads"], r["grads32"], r["grads64"]):
        eh, et = rel(got, want), rel(t32, want)
        report("attention_mh_train %s %s: hip/f64 %.2e torch/f64 %.2e ratio %.2f (of bound %.2f)" % (IDS[CASES.index(case)], name, eh, et, eh / et,
                                                                                                     eh / (FACTOR * et + 1e-6)))
        if not (got.shape == want.shape and eh <= FACTOR * et + 1e-6):
            bad.append((name, eh, et))
    assert not bad, (case, bad)


@pytest.mark.parametrize("det", [True, False])
def test_backward_is_bitwise_reproducible_in_either_mode(dev, det):
    prev = forge_amd.determinism.get_deterministic_setting()
    forge_amd.set_deterministic(det)
    try:
        for case in CASES[:4] + CASES[6:]:
            B, H, Nq, Nk, scale, sliced = case
            q, k, v, dout = inputs(dev, case)
            both = []
            for _ in range(2):
                ls = [t.clone().requires_grad_(True) for t in (q, k, v)]
                both.append(torch.autograd.grad(ops.attention_mh_train(*ls, H, scale), ls, dout))
            assert all(torch.equal(a, b) for a, b in zip(*both)), case
            assert all(torch.equal(a, b) for a, b in zip(both[0], run(dev, case)["grads"])), case     # the same bits in the other mode, and from views
    finally:
        forge_amd.set_deterministic(prev)


def test_forward_and_backward_capture_into_one_graph(dev):
    from forge_amd.graph import GraphedCall
    g = torch.Generator(device=dev).manual_seed(5)
    q, k, v = (torch.randn(2, n, 256, device=dev, generator=g).requires_grad_(True) for n in (128, 256, 256))
    dout = torch.randn(2, 128, 256, device=dev, generator=g)

    def step():
        out = ops.attention_mh_train(q, k, v, 4, 0.125)
        return (out,) + torch.autograd.grad(out, (q, k, v), dout)

    eager = [t.detach().clone() for t in step()]
    graphed = GraphedCall(step, dev, warmup=2)
    for _ in range(2):
        for t in graphed():
            t.detach().fill_(float("nan"))                                            # a replay has to write every output again
        got = graphed()
        torch.cuda.synchronize()
        assert all(torch.equal(a.detach(), b) for a, b in zip(got, eager))


def test_peak_memory_stays_below_one_attention_matrix(dev):
    """Forward + backward at (1, 4, 2048, 2048): the op's own tensors (out, lse, dout's copy, dq, dk, dv, delta: ~16 MB) and nothing of size
    [B*H,Nq,Nk] (64 MB) - a condition the stock path cannot meet (it saves one such matrix and allocates more in its backward)."""
    B, H, N = 1, 4, 2048
    matrix = B * H * N * N * 4
    g = torch.Generator(device=dev).manual_seed(9)
    q, k, v = (torch.randn(B, N, H * 64, device=dev, generator=g).requires_grad_(True) for _ in range(3))
    dout = torch.randn(B, N, H * 64, device=dev, generator=g)
    rise = {}
    for name, fn in (("hip", lambda: ops.attention_mh_train(q, k, v, H, 0.125)), ("stock", lambda: stock(q, k, v, H, 0.125))):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        grads = torch.autograd.grad(fn(), (q, k, v), dout)
        torch.cuda.synchronize()
        rise[name] = torch.cuda.max_memory_allocated(dev) - base
        assert all(torch.isfinite(t).all() for t in grads)
        del grads
    report("attention_mh_train (1,4,2048,2048) forward + backward peak rise: hip %.1f MB, stock %.1f MB (one [B*H,Nq,Nk] matrix %.1f MB)"
           % (rise["hip"] / 1e6, rise["stock"] / 1e6, matrix / 1e6))
    assert rise["hip"] < matrix < rise["stock"], rise


def test_refusals(dev, switch_on):
    t = lambda *s: torch.randn(*s, device=dev)
    ok = t(2, 128, 256)
    assert ops.attention_mh_applies(ok, ok, ok, 4)
    mask = torch.zeros(2, 128, dtype=torch.bool, device=dev)
    wide = t(2, 128, 260)
    refused = {"100 tokens": ((t(2, 100, 256),) * 3, 4),
               "head width 32": ((t(2, 128, 128),) * 3, 4),
               "float64": ((ok.double(),) * 3, 4),
               "a row stride that is no multiple of 4": ((t(2, 128, 258)[:, :, :256],) * 3, 4),
               "a base that is not 16-byte aligned": ((wide[:, :, 2:258],) * 3, 4),
               "a host tensor": ((ok.cpu(),) * 3, 4)}
    for what, ((q, k, v), H) in refused.items():
        assert not ops.attention_mh_applies(q, k, v, H), what
        for fn in (ops.attention_mh, ops.attention_mh_train):
            with pytest.raises(RuntimeError, match=r"multiples of 64.*got num_heads 4.*q \(2, \d+, \d+\)"):
                fn(q, k, v, H, 0.125)
    assert ops.attention_mh_applies(wide[:, :, 4:260], ok, ok, 4)                       # a 16-byte aligned slice of a wider row is in the domain
    # a mask or active dropout: the module keeps torch's ops (the op itself has no such argument: nothing to raise on)
    assert not ops.attention_mh_applies(ok, ok, ok, 4, pad_mask=mask)
    assert not ops.attention_mh_applies(ok, ok, ok, 4, attn_mask=mask)
    assert not ops.attention_mh_applies(ok, ok, ok, 4, dropout_p=0.1, training=True)
    assert ops.attention_mh_applies(ok, ok, ok, 4, dropout_p=0.1, training=False)       # eval mode: dropout is the identity
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="finite positive scale"):
            ops.attention_mh(ok, ok, ok, 4, scale)
    from forge_amd.pose_estimator_2d import MultiHeadAttention
    torch.manual_seed(2)
    m = MultiHeadAttention(4, 256, 256, dropout=0.1).to(dev)
    calls = []
    orig = ops.attention_mh_train
    ops.attention_mh_train = lambda *a: calls.append(1) or orig(*a)
    try:
        m(ok, ok, ok, pad_mask=mask)                                                    # stock path: masked
        m(ok, ok, ok)                                                                   # stock path: dropout active
        assert not calls
        m.eval()
        m(ok, ok, ok)
        assert len(calls) == 1
    finally:
        ops.attention_mh_train = orig
    ops.set_multihead_attention(False)
    assert not ops.attention_mh_applies(ok, ok, ok, 4)                                  # off: the module keeps torch's ops
    assert ops.attention_mh(ok, ok, ok, 4, 0.125).shape == (2, 128, 256)                # the op itself does not depend on the switch
    # the C ABI refuses the same, with its codes
    L, p, st = _lib.lib(), _lib.ptr(ok), _lib.current_stream()
    o, l = _lib.ptr(torch.empty_like(ok)), _lib.ptr(torch.empty(2, 4, 128, device=dev))
    dense = (128 * 256, 256) * 4
    assert L.forge_attention_mh_fwd(p, p, p, o, l, 2, 4, 100, 128, 64, *dense, 0.125, st) == -2 and b"multiples of 64" in L.forge_last_error()
    assert L.forge_attention_mh_fwd(p, p, p, o, l, 2, 4, 128, 128, 32, *dense, 0.125, st) == -2 and b"64 channels" in L.forge_last_error()
    assert L.forge_attention_mh_fwd(p, p, p, o, l, 2, 4, 128, 128, 64, 128 * 256, 258, *dense[2:], 0.125, st) == -2 and b"stride" in L.forge_last_error()
    assert L.forge_attention_mh_fwd(p, p, p, o, l, 2, 4, 128, 128, 64, *dense, -1.0, st) == -1 and b"scale" in L.forge_last_error()
    torch.cuda.synchronize()


# ---- the wiring: CrossAttention + SelfAttention, then the whole estimator

def blocks(dev, dtype=torch.float32):
    from forge_amd.pose_estimator_2d import CrossAttention, SelfAttention
    torch.manual_seed(7)
    cross, selfa = CrossAttention(4, 256, 256, mlp_ratio=4), SelfAttention(4, 256, mlp_ratio=4)
    g = torch.Generator().manual_seed(8)
    feat, canon, w = (torch.randn(1, n, 256, generator=g) for n in (512, 256, 512))
    return cross.to(dev).to(dtype), selfa.to(dev).to(dtype), feat.to(dev).to(dtype), canon.to(dev).to(dtype), w.to(dev).to(dtype)


def block_grads(cross, selfa, feat, canon, w):
    feat, canon = feat.clone().requires_grad_(True), canon.clone().requires_grad_(True)
    out = selfa(cross(x_q=feat, x_k=canon, x_v=canon, residual=feat))
    params = list(cross.parameters()) + list(selfa.parameters())
    return out.detach(), torch.autograd.grad((out * w).sum(), [feat, canon] + params)


_BLOCKS = {}


def block_runs(dev):
    if not _BLOCKS:
        cross, selfa, feat, canon, w = blocks(dev)
        names = ["feat", "canon"] + ["cross." + n for n, _ in cross.named_parameters()] + ["self." + n for n, _ in selfa.named_parameters()]
        from forge_amd.flopmeter import FlopMeter
        prev = ops.set_multihead_attention(False)
        try:
            block_grads(cross, selfa, feat, canon, w)                                  # warm-up: the BLAS library settles its kernel choice on first use
            with FlopMeter() as fm_off:
                off = block_grads(cross, selfa, feat, canon, w)
            off2, off3 = block_grads(cross, selfa, feat, canon, w), block_grads(cross, selfa, feat, canon, w)
            ops.set_multihead_attention(True)
            with FlopMeter() as fm_on:
                on = block_grads(cross, selfa, feat, canon, w)
        finally:
            ops.set_multihead_attention(prev)
        f64 = block_grads(*blocks(dev, torch.float64))
        _BLOCKS.update(names=names, off=off, off2=off2, off3=off3, on=on, f64=f64, launches={"off": fm_off.launches, "on": fm_on.launches},
                       flops=fm_on.flops)
    return _BLOCKS


def test_blocks_take_the_kernels_only_with_the_switch(dev):
    r = block_runs(dev)
    new = ("forge_attention_mh_fwd", "forge_attention_mh_bwd")
    assert [r["launches"]["off"][n] for n in new] == [0, 0] and [r["launches"]["on"][n] for n in new] == [2, 2]
    unit = 4 * 512 * 64 * (256 + 512)                                                  # B H Nq d (Nk of the cross block + Nk of the self block)
    assert r["flops"]["forge_attention_mh_fwd"] == 4.0 * unit and r["flops"]["forge_attention_mh_bwd"] == 16.0 * unit
    # off: the stock statements. The output repeats its bits, and every gradient does wherever torch's own backward repeats its bits (where two
    # switch-off runs differ - atomics in torch's LayerNorm / GEMM gradients - a third has to be as close as 4 x their distance).
    assert torch.equal(r["off"][0], r["off2"][0]) and torch.equal(r["off"][0], r["off3"][0])
    for name, a, b, c in zip(r["names"], r["off"][1], r["off2"][1], r["off3"][1]):
        sp, d = (b - c).abs().max().item(), (a - b).abs().max().item()
        if sp or d:
            report("blocks switch off, run 1 vs 2 d/d %-36s max-abs diff %.2e, run 2 vs 3 %.2e (of max %.2e)" % (name, d, sp, b.abs().max().item()))
        assert torch.equal(a, b) if sp == 0.0 else d <= 4.0 * sp, name
    assert any(not torch.equal(a, b) for a, b in zip(r["on"][1], r["off"][1]))          # on: other bits, the same function (next test)


def test_blocks_output_and_gradients_vs_float64(dev):
    """Output, input gradients and every parameter gradient of CrossAttention -> SelfAttention with the switch on against the same modules in
    float64, the switch-off fp32 run as yardstick, rule eh <= 2 et + 1e-6 per tensor (errors relative to the tensor's float64 maximum; the two
    k_proj biases, whose exact gradient is zero - a key bias shifts every logit of a row alike - relative to their weight's gradient, the scale of
    what cancels)."""
    r = block_runs(dev)
    names, f64 = r["names"], r["f64"][1]
    eh, et = rel(r["on"][0], r["f64"][0]), rel(r["off"][0], r["f64"][0])
    report("blocks output: hip/f64 %.2e torch/f64 %.2e" % (eh, et))
    bad = [] if eh <= FACTOR * et + 1e-6 else [("output", eh, et)]
    assert len(names) == len(f64) == len(r["on"][1])
    for name, got, t32, want in zip(names, r["on"][1], r["off"][1], f64):
        scale = want.abs().max().item()
        if name.endswith("k_proj.bias"):
            scale = max(scale, f64[names.index(name[:-4] + "weight")].abs().max().item())
        eh, et = (got.double() - want).abs().max().item() / scale, (t32.double() - want).abs().max().item() / scale
        report("blocks d/d %-36s hip/f64 %.2e torch/f64 %.2e ratio %.2f" % (name, eh, et, eh / max(et, 1e-30)))
        if not eh <= FACTOR * et + 1e-6:
            bad.append((name, eh, et))
    assert not bad, bad


def test_whole_estimator_calls_and_eval_features_vs_float64(dev):
    """PoseEstimator2D on [1,3,3,256,256]: six ops.attention_mh calls under no_grad in eval mode and six ops.attention_mh_train calls in grad mode
    with the switch on, none with it off; the eval features against the float64 stock evaluation on the CPU within the bound
    tests/test_gpu_configs.py uses for this module, 3 x the switch-off stock GPU path's distance + 2e-5."""
    import stock_pose
    from forge_amd.pose_estimator_2d import PoseEstimator2D
    torch.manual_seed(5)
    mod = PoseEstimator2D()
    sd = syn.seeded_state_dict({"m." + k: v for k, v in mod.state_dict().items()}, 13)
    mod.load_state_dict({k[2:]: v for k, v in sd.items()})
    mod.eval()
    x = torch.rand(1, 3, 3, 256, 256)
    ref_mod = copy.deepcopy(mod).double()
    for m in ref_mod.modules():
        for k, v in list(vars(m).items()):
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(m, k, v.double())
    g, xd = copy.deepcopy(mod).to(dev), x.to(dev)
    calls = {"attention_mh": 0, "attention_mh_train": 0}
    orig = {n: getattr(ops, n) for n in calls}

    def counting(n):
        def fn(*a, **kw):
            calls[n] += 1
            return orig[n](*a, **kw)
        return fn

    prev = ops.set_multihead_attention(False)
    try:
        for n in calls:
            setattr(ops, n, counting(n))
        with torch.no_grad():
            ref = stock_pose.stock_forward(ref_mod)(x.double(), return_features=True)
            stock_ = stock_pose.stock_forward(copy.deepcopy(mod).to(dev))(xd, return_features=True)
            off = g(xd, return_features=True)
        g(xd, return_features=True)
        assert calls == {"attention_mh": 0, "attention_mh_train": 0}
        ops.set_multihead_attention(True)
        with torch.no_grad():
            on = g(xd, return_features=True)
        assert calls == {"attention_mh": 6, "attention_mh_train": 0}
        on_grad = g(xd, return_features=True)
        assert calls == {"attention_mh": 6, "attention_mh_train": 6}
    finally:
        for n, fn in orig.items():
            setattr(ops, n, fn)
        ops.set_multihead_attention(prev)
    relc = lambda got, want: (got.detach().double().cpu() - want).abs().max().item() / want.abs().max().item()
    eh, eg, eo, es = relc(on, ref), relc(on_grad, ref), relc(off, ref), relc(stock_, ref)
    report("PoseEstimator2D eval features: switch on/f64 %.2e (grad mode %.2e), switch off/f64 %.2e, stock/f64 %.2e" % (eh, eg, eo, es))
    assert eh <= 3.0 * es + 2e-5 and eg <= 3.0 * es + 2e-5, (eh, eg, es)
