"""GPU (-m gpu): the differentiable attention of pose-estimator training - ops.attention_train = forge_attention_fwd_lse + forge_attention_bwd
(forge_amd/csrc/attention.hip), opt-in through ops.set_attention_training.

Forward: `out` is ops.attention's bit for bit, lse is the float64 logsumexp. Gradients: dq, dk, dv against float64 autograd of matmul - softmax -
matmul on the GPU, with torch's fp32 autograd of the same three ops as the yardstick and the forward test's rule (tests/test_gpu_parity.py
test_attention_vs_float64_and_torch): error / max <= 2 x torch's + 1e-6. Bitwise reproducible in either determinism mode, capturable into a hipGraph,
refusals outside the domain, and the wiring into PoseTransformer (gradients, the branch taken, the [B,N,N] matrices gone from peak memory).

FORGE_TEST_REPORT=1 prints every measured ratio."""
import os

import pytest
import torch

import forge_amd
from forge_amd import _lib, ops

pytestmark = pytest.mark.gpu

#        B, Nq,   Nk,   shared_v, gain
CASES = [(1, 64, 64, False, 1.0),
         (3, 128, 192, False, 1.0),          # ragged: 2 key parts in the dQ pass, 4 query parts in the dK/dV pass
         (2, 192, 128, False, 6.0),          # peaky logits; 4 key parts, 2 query parts
         (2, 128, 256, True, 1.0),           # 4 parts both ways, one value table for the batch: no dv
         (1, 4096, 4096, False, 2.5)]        # the estimator's size, once
IDS = ["%dx%dx%d%s_g%g" % (B, Nq, Nk, "_shared" if sh else "", g) for B, Nq, Nk, sh, g in CASES]
FACTOR = 2.0                                 # eh <= FACTOR * et + 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def report(line):
    if os.environ.get("FORGE_TEST_REPORT"):
        print("  " + line)


def rel(got, want):
    return (got.double() - want).abs().max().item() / want.abs().max().item()


def stock(q, k, v):
    return torch.matmul(torch.matmul(q, k.transpose(1, 2)).softmax(dim=-1), v)


def inputs(dev, case):
    B, Nq, Nk, shared, gain = case
    g = torch.Generator(device=dev).manual_seed(17 + CASES.index(case))
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    return rnd(B, Nq, 64) * gain * 0.5, rnd(B, Nk, 64) * 0.5, rnd(1 if shared else B, Nk, 64), rnd(B, Nq, 64)


_RUNS = {}


def run(dev, case):
    """One evaluation per case, shared by the tests and left unchanged: the kernels' out / lse / gradients, float64 and torch-fp32 references."""
    if case in _RUNS:
        return _RUNS[case]
    shared = case[3]
    q, k, v, dout = inputs(dev, case)
    leaves = lambda dt: [t.clone().to(dt).requires_grad_(g) for t, g in ((q, True), (k, True), (v, not shared))]
    grads = lambda out, ls, dt: torch.autograd.grad(out, ls[:2] if shared else ls, dout.to(dt))
    r = {"q": q, "k": k, "v": v, "dout": dout}
    ls = leaves(torch.float32)
    r["out"] = ops.attention_train(*ls)
    r["grads"] = grads(r["out"], ls, torch.float32)
    r["out"] = r["out"].detach()
    ls = leaves(torch.float32)
    r["grads32"] = grads(stock(*ls), ls, torch.float32)
    ls = leaves(torch.float64)
    r["grads64"] = grads(stock(*ls), ls, torch.float64)
    with torch.no_grad():
        r["lse32"] = torch.logsumexp(torch.matmul(q, k.transpose(1, 2)), dim=-1)
        r["lse64"] = torch.logsumexp(torch.matmul(q.double(), k.double().transpose(1, 2)), dim=-1)
    _RUNS[case] = r
    return r


def call_fwd_lse(q, k, v):
    B, Nq, _ = q.shape
    Nk = k.shape[1]
    out, lse = torch.empty_like(q), torch.empty(B, Nq, device=q.device)
    _lib.check(_lib.lib().forge_attention_fwd_lse(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 0 if v.shape[0] == 1 and B > 1 else Nk, _lib.ptr(out),
                                                  _lib.ptr(lse), B, Nq, Nk, 64, _lib.current_stream()), "forge_attention_fwd_lse")
    return out, lse


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_is_ops_attention_bitwise_and_lse_is_logsumexp(dev, case):
    r = run(dev, case)
    with torch.no_grad():
        want = ops.attention(r["q"], r["k"], r["v"])
    out, lse = call_fwd_lse(r["q"], r["k"], r["v"])
    assert torch.equal(r["out"], want) and torch.equal(out, want)                      # both key splits occur among the cases
    eh, et = rel(lse, r["lse64"]), rel(r["lse32"], r["lse64"])
    report("attention_train %s lse: hip/f64 %.2e torch/f64 %.2e" % (IDS[CASES.index(case)], eh, et))
    assert eh <= FACTOR * et + 1e-6, (case, eh, et)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_vs_float64_with_torch_fp32_as_yardstick(dev, case):
    r = run(dev, case)
    assert len(r["grads"]) == (2 if case[3] else 3)
    bad = []
    for name, got, t32, want in zip(("dq", "dk", "dv"), r["grads"], r["grads32"], r["grads64"]):
        eh, et = rel(got, want), rel(t32, want)
        report("attention_train %s %s: hip/f64 %.2e torch/f64 %.2e ratio %.2f (of bound %.2f)" % (IDS[CASES.index(case)], name, eh, et, eh / et,
                                                                                                  eh / (FACTOR * et + 1e-6)))
        if not (got.shape == want.shape and eh <= FACTOR * et + 1e-6):
            bad.append((name, eh, et))
    assert not bad, (case, bad)


@pytest.mark.parametrize("det", [True, False])
def test_backward_is_bitwise_reproducible_in_either_mode(dev, det):
    prev = forge_amd.determinism.get_deterministic_setting()
    forge_amd.set_deterministic(det)
    try:
        for case in CASES[:4]:
            q, k, v, dout = inputs(dev, case)
            both = []
            for _ in range(2):
                ls = [q.clone().requires_grad_(True), k.clone().requires_grad_(True), v.clone().requires_grad_(not case[3])]
                both.append(torch.autograd.grad(ops.attention_train(*ls), ls[:2] if case[3] else ls, dout))
            assert all(torch.equal(a, b) for a, b in zip(*both)), case
            assert all(torch.equal(a, b) for a, b in zip(both[0], run(dev, case)["grads"])), case     # and the same bits in the other mode
    finally:
        forge_amd.set_deterministic(prev)


def test_refusals(dev):
    q = torch.randn(2, 100, 64, device=dev)
    prev = ops.set_attention_training(True)
    try:
        assert not ops.attention_train_applies(q, q, q)                                # 100 tokens: not a multiple of 64
        with pytest.raises(RuntimeError, match="multiples of 64"):
            ops.attention_train(q, q, q)
        q64, q32 = q[:, :64].contiguous(), q[:, :64, :32].contiguous()
        assert ops.attention_train_applies(q64, q64, q64) and not ops.attention_train_applies(q32, q32, q32)
        with pytest.raises(RuntimeError, match="multiples of 64"):
            ops.attention_train(q32, q32, q32)                                         # 32 channels
        table = q64[:1].clone()
        assert ops.attention_train_applies(q64, q64, table)                            # one table for the batch, a constant
        assert not ops.attention_train_applies(q64, q64, table.requires_grad_(True))   # ... that wants a gradient: not this kernel
        with pytest.raises(RuntimeError, match="must not require grad"):
            ops.attention_train(q64, q64, table)
        ops.set_attention_training(False)
        assert not ops.attention_train_applies(q64, q64, q64)                          # off: the models keep torch's ops
        assert ops.attention_train(q64, q64, q64).shape == (2, 64, 64)                 # the op itself does not depend on the switch
    finally:
        ops.set_attention_training(prev)
    L, p, st = _lib.lib(), _lib.ptr(q), _lib.current_stream()
    a, b, c, d = (_lib.ptr(w) for w in torch.empty(4, 2, 64, 64, device=dev))
    assert L.forge_attention_bwd(p, p, p, 64, p, p, p, a, b, c, d, 1, 100, 64, 64, st) != 0 and b"multiples of 64" in L.forge_last_error()
    assert L.forge_attention_bwd(p, p, p, 64, p, p, p, a, b, c, d, 1, 64, 64, 32, st) != 0 and b"64 channels" in L.forge_last_error()
    assert L.forge_attention_fwd_lse(p, p, p, 64, a, b, 1, 100, 64, 64, st) != 0 and b"multiples of 64" in L.forge_last_error()
    assert L.forge_attention_fwd_lse(p, p, p, 64, a, b, 1, 64, 64, 32, st) != 0 and b"64 channels" in L.forge_last_error()
    rc = L.forge_attention_bwd(p, p, p, 0, p, p, p, a, b, c, d, 2, 64, 64, 64, st)     # shared v and a non-null dv
    assert rc != 0 and b"shared" in L.forge_last_error()
    torch.cuda.synchronize()


def test_forward_and_backward_capture_into_one_graph(dev):
    from forge_amd.graph import GraphedCall
    case = (2, 128, 256, False, 1.0)
    g = torch.Generator(device=dev).manual_seed(5)
    q, k, v = (torch.randn(2, n, 64, device=dev, generator=g).requires_grad_(True) for n in (128, 256, 256))
    dout = torch.randn(2, 128, 64, device=dev, generator=g)

    def step():
        out = ops.attention_train(q, k, v)
        return (out,) + torch.autograd.grad(out, (q, k, v), dout)

    eager = [t.detach().clone() for t in step()]
    graphed = GraphedCall(step, dev, warmup=2)
    for _ in range(2):
        for t in graphed():
            t.detach().fill_(float("nan"))                                            # a replay has to write every output again
        got = graphed()
        torch.cuda.synchronize()
        assert all(torch.equal(a.detach(), b) for a, b in zip(got, eager)), case


# ---- the wiring: PoseTransformer takes the branch with the switch on, and only then

def stock_pose_transformer(m, q, k):
    """PoseTransformer.forward on torch's differentiable ops alone (what training ran before the switch existed)."""
    ct, st = m.cross_transformer, m.self_transformer
    qn, kn = ct._qk(q, k, None, None)
    coord = torch.matmul(torch.matmul(qn, kn.transpose(-2, -1)).softmax(dim=-1), m._pos_embed(q)).permute(0, 2, 1)
    b = coord.shape[0]
    sq, sk = st._qk(coord, coord, None, None)
    sv = st.encode_value(coord).permute(0, 2, 1)
    x = coord.permute(0, 2, 1)
    x = x + torch.matmul(torch.matmul(sq, sk.transpose(-2, -1)).softmax(dim=-1), sv)
    x = x + st.mlp(st.norm2(x))
    return x.permute(0, 2, 1).contiguous().view(b, st.channels, -1)


def pose_transformer(dev, res, dtype=torch.float32):
    from forge_amd.pose_estimator_3d import PoseTransformer
    torch.manual_seed(3)
    m = PoseTransformer(inp_res=res).to(dev).to(dtype)
    g = torch.Generator(device=dev).manual_seed(4)
    n = res ** 3
    q, k, w = (torch.randn(2, 64, n, device=dev, generator=g).to(dtype) for _ in range(3))
    return m, q, k, w


def module_grads(m, q, k, w, fn=None):
    q, k = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    out = (fn or (lambda a, b: m(q=a, k=b)))(q, k)
    # (the cross block's value encoder and MLP are not part of PoseTransformer.forward: None)
    return out.detach(), torch.autograd.grad((out * w).sum(), [q, k] + list(m.parameters()), allow_unused=True)


_MODULE = {}


def module_runs(dev):
    """PoseTransformer(inp_res=8), B = 2, one scalar loss: gradients with the switch off, of the stock restatement, with the switch on, and in float64."""
    if not _MODULE:
        m, q, k, w = pose_transformer(dev, 8)
        names = ["q", "k"] + [n for n, _ in m.named_parameters()]
        from forge_amd.flopmeter import FlopMeter
        prev = ops.set_attention_training(False)
        try:
            module_grads(m, q, k, w)                                                   # warm-up: the BLAS library settles its kernel choice on first use
            with FlopMeter() as fm_off:
                off = module_grads(m, q, k, w)
            stock_ = module_grads(m, q, k, w, lambda a, b: stock_pose_transformer(m, a, b))
            stock2 = module_grads(m, q, k, w, lambda a, b: stock_pose_transformer(m, a, b))
            ops.set_attention_training(True)
            with FlopMeter() as fm_on:
                on = module_grads(m, q, k, w)
        finally:
            ops.set_attention_training(prev)
        f64 = module_grads(m.double(), q.double(), k.double(), w.double())
        used = [i for i, g in enumerate(f64[1]) if g is not None]
        assert len(used) == 2 + 20 and all((r[1][i] is None) == (f64[1][i] is None) for r in (off, stock_, stock2, on) for i in range(len(names)))
        pick = lambda r: (r[0], [r[1][i] for i in used])
        _MODULE.update(names=[names[i] for i in used], off=pick(off), stock=pick(stock_), stock2=pick(stock2), on=pick(on), f64=pick(f64),
                       launches={"off": fm_off.launches, "on": fm_on.launches})
    return _MODULE


def test_pose_transformer_takes_the_kernels_only_with_the_switch(dev):
    r = module_runs(dev)
    new = ("forge_attention_fwd", "forge_attention_fwd_lse", "forge_attention_bwd")
    # off: the stock branch - not one launch of the attention entry points, the output of torch's ops bit for bit, and every gradient bit for bit
    # wherever torch's own backward repeats its bits. It does not always: on the MI355X two runs of the stock restatement, both after a warm-up
    # pass, have differed in some parameter gradients (atomics in torch's LayerNorm / GEMM gradients; FORGE_TEST_REPORT names the tensors, and
    # profiles/r12_attention_bwd_probe.txt records a run). For such a tensor "the parent's bits" are not defined; the switch-off run then has to be
    # as close to one stock run as 4 x the distance between the two.
    assert [r["launches"]["off"][n] for n in new] == [0, 0, 0]
    assert torch.equal(r["off"][0], r["stock"][0])
    for name, a, b, c in zip(r["names"], r["off"][1], r["stock"][1], r["stock2"][1]):
        sp, d = (b - c).abs().max().item(), (a - b).abs().max().item()
        if sp or d:
            report("PoseTransformer(8) switch off vs stock d/d %-36s max-abs diff %.2e, stock vs stock %.2e (of max %.2e)" % (name, d, sp, b.abs().max().item()))
        assert torch.equal(a, b) if sp == 0.0 else d <= 4.0 * sp, name
    # on: both attentions (cross with the shared table, self) ran the kernels forward and backward - other bits in the gradients, the same function
    assert [r["launches"]["on"][n] for n in new] == [0, 2, 2]
    assert any(not torch.equal(a, b) for a, b in zip(r["on"][1], r["off"][1]))
    assert rel(r["on"][0], r["f64"][0]) <= FACTOR * rel(r["off"][0], r["f64"][0]) + 1e-6


def test_pose_transformer_gradients_vs_float64(dev):
    """Input and parameter gradients of PoseTransformer(8) with the switch on against the float64 run of the module, the switch-off fp32 run as
    yardstick, rule eh <= 2 et + 1e-6 per tensor (errors relative to the tensor's float64 maximum; the two key-encoder biases, whose exact gradient is
    zero - a key bias shifts every logit of a row alike - relative to their weight's gradient, the scale of what cancels).

    The module's self attention is the hard case for a backward that takes delta = dout . out: nearly uniform (softmax max 0.019 over 512 keys) over
    nearly equal keys (token spread / mean 0.25), so dq_i = sum_j dS_ij k_j is the small remainder of cancelling terms and only survives if every
    row of dS sums to zero to rounding. Without the row-residual correction of the dQ pass (csrc/attention.hip) the six tensors behind that
    attention's queries and keys were at 4.1 - 9.7 x torch's error on the MI355X (self_transformer.norm.weight 2.05e-05 against 2.72e-06)."""
    r = module_runs(dev)
    names, f64 = r["names"], r["f64"][1]
    bad = []
    for i, (name, got, t32, want) in enumerate(zip(names, r["on"][1], r["off"][1], f64)):
        scale = want.abs().max().item()
        if name.endswith("encode_key.bias"):
            scale = max(scale, f64[names.index(name[:-4] + "weight")].abs().max().item())
        eh, et = (got.double() - want).abs().max().item() / scale, (t32.double() - want).abs().max().item() / scale
        report("PoseTransformer(8) d/d %-36s hip/f64 %.2e torch/f64 %.2e ratio %.2f" % (name, eh, et, eh / max(et, 1e-30)))
        if not eh <= FACTOR * et + 1e-6:
            bad.append((name, eh, et))
    assert not bad, bad


def test_pose_transformer_peak_memory_at_4096_tokens(dev):
    m, q, k, w = pose_transformer(dev, 16)
    matrix = 2 * 4096 * 4096 * 4                                                       # one [B,N,N] fp32 matrix: 134 MB
    rise = {}
    prev = ops.set_attention_training(False)
    try:
        for on in (True, False):
            ops.set_attention_training(on)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            out, grads = module_grads(m, q, k, w)
            torch.cuda.synchronize()
            rise[on] = torch.cuda.max_memory_allocated(dev) - base
            assert all(torch.isfinite(g).all() for g in grads if g is not None)
            del out, grads
    finally:
        ops.set_attention_training(prev)
    report("PoseTransformer(16) B=2 forward + backward peak rise: switch on %.1f MB, off %.1f MB (one [B,N,N] matrix %.1f MB)"
           % (rise[True] / 1e6, rise[False] / 1e6, matrix / 1e6))
    assert rise[True] < matrix < rise[False], rise
