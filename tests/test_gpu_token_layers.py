"""GPU (-m gpu): the token-row layers of both pose estimators on the project's kernels - ops.token_linear / ops.token_linear_train =
forge_token_linear_fwd / forge_token_linear_bwd and ops.layer_norm / ops.layer_norm_train = forge_layer_norm_fwd / forge_layer_norm_bwd
(forge_amd/csrc/token.hip), opt-in through ops.set_token_layers.

The arithmetic: y, the saved (mean, rstd) and every gradient against float64 evaluations of F.layer_norm - F.linear - F.gelu - add on the GPU with
torch's fp32 ops on the same inputs as the yardstick and the rule of tests/test_gpu_attention_bwd.py, error / max <= 2 x torch's + 1e-6. The
addressing is pinned apart from it, bit for bit: LN-prologue + linear equals ops.layer_norm followed by the plain linear, a strided y equals a dense
one, the inference and the autograd form agree, a backward with some outputs left out gives the bits of the full one. Then: bitwise reproducible in
either determinism mode, capturable into a hipGraph, refusals outside the domain, and the wiring into the blocks of both estimators.

The LayerNorm rows have mean 3 (three standard deviations): a one-pass variance E[x^2] - mean^2 would lose the bound. The GELU cases' pre-activations
have a standard deviation of about 1.6: |v| from 0 to beyond 4.

FORGE_TEST_REPORT=1 prints every measured ratio."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import forge_amd
from forge_amd import _lib, ops, synthetic as syn

pytestmark = pytest.mark.gpu

#        R,   K,    N,    LN,    act,    residual (False, True = dense, 2 = rows of a wider tensor), y row stride (0 = dense)
CASES = [(1, 64, 64, True, None, False, 0),             # one row: the tile mask at its extreme
         (33, 64, 128, True, "gelu", False, 0),         # the 3-D fc1; a ragged second tile
         (200, 128, 64, False, None, True, 0),          # the 3-D fc2
         (64, 256, 256, True, None, False, 768),        # a 2-D projection into a q|k|v slab
         (96, 256, 1024, True, "gelu", False, 0),       # the 2-D fc1; the widest N
         (96, 1024, 256, False, None, 2, 0),            # the 2-D fc2; the longest K (four LDS chunks); the residual with its own stride
         (129, 64, 64, True, "gelu", True, 0),          # the plan's first multi-chunk row count: two chunks, the last of one row
         (16384, 64, 64, True, None, False, 0)]         # one scene's 3-D rows
IDS = ["%dx%dx%d%s%s%s%s" % (R, K, N, "_ln" if ln else "", "_gelu" if act else "", "_res" if res else "", "_ldy%d" % ldy if ldy else "")
       for R, K, N, ln, act, res, ldy in CASES]
FACTOR = 2.0                                            # eh <= FACTOR * et + 1e-6
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture()
def switch_on():
    prev = ops.set_token_layers(True)
    yield
    ops.set_token_layers(prev)


def report(line):
    if os.environ.get("FORGE_TEST_REPORT"):
        print("  " + line)


def rel(got, want):
    return (got.double() - want).abs().max().item() / want.abs().max().item()


def stock(x, w, b, gamma, beta, res, act):
    h = x if gamma is None else F.layer_norm(x, (x.shape[-1],), gamma, beta, EPS)
    y = F.linear(h, w, b)
    if act:
        y = F.gelu(y)
    return y if res is None else res + y


def stock_stats(x):
    return torch.stack([x.mean(-1), 1.0 / torch.sqrt(x.var(-1, unbiased=False) + EPS)], dim=-1)


def inputs(dev, case):
    """{name: tensor} of one case; absent operands are None."""
    R, K, N, ln, act, res, ldy = case
    g = torch.Generator(device=dev).manual_seed(77 + CASES.index(case))
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    t = {"x": 3.0 + rnd(R, K) if ln else rnd(R, K), "w": rnd(N, K) * (1.5 / K ** 0.5), "b": rnd(N) * 0.5,
         "gamma": 1.0 + 0.5 * rnd(K) if ln else None, "beta": 0.5 * rnd(K) if ln else None, "res": None, "dy": rnd(R, N)}
    if res is True:
        t["res"] = rnd(R, N)
    elif res == 2:
        t["res"] = rnd(R, N + 64)[:, 32:32 + N]
        assert t["res"].stride(0) == N + 64 and t["res"].data_ptr() % 16 == 0
    return t


NAMES = ("x", "w", "b", "gamma", "beta", "res")
_RUNS = {}


def hip_train(t, act):
    return ops.token_linear_train(t["x"], t["w"], t["b"], ln=None if t["gamma"] is None else (t["gamma"], t["beta"], EPS), act=act, residual=t["res"])


def run(dev, case):
    """One evaluation per case, shared by the tests and left unchanged: the kernels' y / stats / gradients, float64 and torch-fp32 references."""
    if case in _RUNS:
        return _RUNS[case]
    R, K, N, ln, act, res, ldy = case
    t = inputs(dev, case)
    r = {"t": t}
    for tag, dt in (("hip", torch.float32), ("32", torch.float32), ("64", torch.float64)):
        ls = {n: (None if t[n] is None else t[n].detach().clone().to(dt).requires_grad_(True)) for n in NAMES}
        if tag == "hip" and res == 2:                                       # a leaf that is rows of a wider tensor, as a block would hand over
            wide = torch.zeros(R, N + 64, device=dev)
            wide[:, 32:32 + N] = t["res"]
            wide.requires_grad_(True)
            ls["res"] = wide[:, 32:32 + N]
        y = hip_train(ls, act) if tag == "hip" else stock(ls["x"], ls["w"], ls["b"], ls["gamma"], ls["beta"], ls["res"], act)
        wrt = [n for n in NAMES if ls[n] is not None]
        r["grads" + tag] = dict(zip(wrt, torch.autograd.grad(y, [ls[n] for n in wrt], t["dy"].to(dt))))
        r["y" + tag] = y.detach()
    if ln:
        with torch.no_grad():
            r["stats32"], r["stats64"] = stock_stats(t["x"]), stock_stats(t["x"].double())
    _RUNS[case] = r
    return r


def test_the_cases_cover_the_plan(dev):
    """The split reductions: 128 rows are one chunk, 129 two (the last of one row); one scene's 3-D rows are many chunks; the 2-D fc1 few."""
    assert ops.token_rows_plan(128, 64, 64) == (1, 128) and ops.token_rows_plan(129, 64, 64) == (2, 128)
    assert ops.token_rows_plan(16384, 64, 64) == (128, 128) and ops.token_rows_plan(1024, 256, 1024) == (8, 128)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_stats_vs_float64(dev, case):
    R, K, N, ln, act, res, ldy = case
    r, t = run(dev, case), run(dev, case)["t"]
    lnarg = (t["gamma"], t["beta"], EPS) if ln else None
    y, stats, pre = ops._token_forward(t["x"], t["w"], t["b"], lnarg, act, t["res"], None, True)
    assert y.shape == (R, N) and torch.equal(y, r["yhip"])
    checks = [("y", y, r["y32"], r["y64"])]
    if ln:
        checks += [("mean", stats[:, 0], r["stats32"][:, 0], r["stats64"][:, 0]), ("rstd", stats[:, 1], r["stats32"][:, 1], r["stats64"][:, 1])]
    else:
        assert stats is None
    if act:
        with torch.no_grad():
            h32, h64 = (F.linear(F.layer_norm(x, (K,), g, b, EPS), w, bb) for x, g, b, w, bb in
                        ((t["x"], t["gamma"], t["beta"], t["w"], t["b"]), tuple(v.double() for v in (t["x"], t["gamma"], t["beta"], t["w"], t["b"]))))
        checks.append(("pre", pre, h32, h64))
        assert h64.abs().max().item() > 4.0 and h64.abs().min().item() < 0.01             # GELU inputs from 0 to beyond 4
    else:
        assert pre is None
    for name, got, t32, want in checks:
        eh, et = rel(got, want), rel(t32, want)
        report("token_linear %s %s: hip/f64 %.2e torch/f64 %.2e" % (IDS[CASES.index(case)], name, eh, et))
        assert eh <= FACTOR * et + 1e-6, (case, name, eh, et)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_vs_float64_with_torch_fp32_as_yardstick(dev, case):
    r = run(dev, case)
    bad = []
    assert list(r["gradship"]) == list(r["grads64"])
    for name, want in r["grads64"].items():
        got, t32 = r["gradship"][name], r["grads32"][name]
        eh, et = rel(got, want), rel(t32, want)
        report("token_linear_train %s d%s: hip/f64 %.2e torch/f64 %.2e ratio %.2f (of bound %.2f)" % (IDS[CASES.index(case)], name, eh, et, eh / max(et, 1e-30),
                                                                                                     eh / (FACTOR * et + 1e-6)))
        if not (got.shape == want.shape and eh <= FACTOR * et + 1e-6):
            bad.append((name, eh, et))
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_addressing_is_pinned_bitwise(dev, case):
    R, K, N, ln, act, res, ldy = case
    r, t = run(dev, case), run(dev, case)["t"]
    lnarg = (t["gamma"], t["beta"], EPS) if ln else None
    with torch.no_grad():
        y = ops.token_linear(t["x"], t["w"], t["b"], ln=lnarg, act=act, residual=t["res"])
        assert torch.equal(y, r["yhip"])                                                # the inference and the autograd form
        slab = torch.full((R, ldy or 3 * N), float("nan"), device=dev)
        out = slab[:, N:2 * N]
        assert ops.token_linear(t["x"], t["w"], t["b"], ln=lnarg, act=act, residual=t["res"], out=out) is out
        assert torch.equal(out, y) and torch.isnan(slab[:, :N]).all() and torch.isnan(slab[:, 2 * N:]).all()      # a strided y, and nothing beside it
        xs = torch.zeros(R, K + 64, device=dev)[:, 32:32 + K].copy_(t["x"])             # x as rows of a wider tensor
        assert torch.equal(ops.token_linear(xs, t["w"], t["b"], ln=lnarg, act=act, residual=t["res"]), y)
        if ln:
            xn = ops.layer_norm(t["x"], t["gamma"], t["beta"], EPS)
            assert torch.equal(ops.token_linear(xn, t["w"], t["b"], act=act, residual=t["res"]), y)     # LN prologue = ops.layer_norm, then the plain linear


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_with_outputs_left_out_gives_the_same_bits(dev, case):
    R, K, N, ln, act, res, ldy = case
    r, t = run(dev, case), run(dev, case)["t"]
    subsets = [("x",), ("w",), ("w", "b"), ("b",)] + ([("x", "w", "b", "beta"), ("gamma",), ("x", "gamma", "beta")] if ln else []) + ([("res",)] if res else [])
    for wrt in subsets:
        ls = {n: (None if t[n] is None else t[n].detach().clone().requires_grad_(n in wrt)) for n in NAMES}
        got = torch.autograd.grad(hip_train(ls, act), [ls[n] for n in wrt], t["dy"])
        for n, g in zip(wrt, got):
            assert torch.equal(g, r["gradship"][n]), (case, wrt, n)


@pytest.mark.parametrize("case", [c for c in CASES if c[3]], ids=[i for c, i in zip(CASES, IDS) if c[3]])
def test_stand_alone_layer_norm_vs_float64(dev, case):
    R, K = case[:2]
    t = run(dev, case)["t"]
    dy = torch.randn(R, K, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    res = {}
    for tag, dt in (("hip", torch.float32), ("32", torch.float32), ("64", torch.float64)):
        ls = [t[n].detach().clone().to(dt).requires_grad_(True) for n in ("x", "gamma", "beta")]
        y = ops.layer_norm_train(*ls, EPS) if tag == "hip" else F.layer_norm(ls[0], (K,), ls[1], ls[2], EPS)
        res[tag] = (y.detach(),) + torch.autograd.grad(y, ls, dy.to(dt))
    with torch.no_grad():
        assert torch.equal(ops.layer_norm(t["x"], t["gamma"], t["beta"], EPS), res["hip"][0])
    ls = [t[n].detach().clone().requires_grad_(n != "gamma") for n in ("x", "gamma", "beta")]            # no dgamma: the same dx and dbeta
    gx, gb = torch.autograd.grad(ops.layer_norm_train(*ls, EPS), [ls[0], ls[2]], dy)
    assert torch.equal(gx, res["hip"][1]) and torch.equal(gb, res["hip"][3])
    for i, name in enumerate(("y", "dx", "dgamma", "dbeta")):
        eh, et = rel(res["hip"][i], res["64"][i]), rel(res["32"][i], res["64"][i])
        report("layer_norm_train %dx%d %s: hip/f64 %.2e torch/f64 %.2e" % (R, K, name, eh, et))
        assert eh <= FACTOR * et + 1e-6, (case, name, eh, et)


@pytest.mark.parametrize("det", [True, False])
def test_forward_and_backward_are_bitwise_reproducible_in_either_mode(dev, det):
    prev = forge_amd.determinism.get_deterministic_setting()
    forge_amd.set_deterministic(det)
    try:
        for case in CASES:
            r, t = run(dev, case), run(dev, case)["t"]
            for _ in range(2):
                ls = {n: (None if t[n] is None else t[n].detach().clone().requires_grad_(True)) for n in NAMES}
                y = hip_train(ls, case[4])
                wrt = [n for n in NAMES if ls[n] is not None]
                grads = torch.autograd.grad(y, [ls[n] for n in wrt], t["dy"])
                assert torch.equal(y, r["yhip"]), case
                assert all(torch.equal(g, r["gradship"][n]) for n, g in zip(wrt, grads)), case
    finally:
        forge_amd.set_deterministic(prev)


def test_forward_and_backward_capture_into_one_graph(dev):
    from forge_amd.graph import GraphedCall
    t = inputs(dev, CASES[6])
    ls = {n: t[n].detach().clone().requires_grad_(True) for n in NAMES}
    wrt = [ls[n] for n in NAMES if n != "res"]                                         # (the residual's gradient is dy itself: an input, not an output)

    def step():
        y = hip_train(ls, "gelu")
        n2 = ops.layer_norm_train(ls["x"], ls["gamma"], ls["beta"], EPS)
        return (y, n2) + torch.autograd.grad([y, n2], wrt, [t["dy"], t["x"]])

    eager = [v.detach().clone() for v in step()]
    graphed = GraphedCall(step, dev, warmup=2)
    for _ in range(2):
        for v in graphed():
            v.detach().fill_(float("nan"))                                             # a replay has to write every output again
        got = graphed()
        torch.cuda.synchronize()
        assert all(torch.equal(a.detach(), b) for a, b in zip(got, eager))


def test_refusals(dev, switch_on):
    t = lambda *s: torch.randn(*s, device=dev)
    x, w, b, g = t(2, 40, 128), t(64, 128), t(64), t(128)
    ln = (g, g, EPS)
    assert ops.token_layers_applies(x, w, b, ln, "gelu", t(2, 40, 64)) and ops.token_layers_applies(x, ln=ln)
    wide = t(2, 40, 136)
    refused = {"float64": x.double(), "a host tensor": x.cpu(), "K no multiple of 64": t(2, 40, 96), "a channel stride": t(2, 128, 40).transpose(1, 2),
               "a row stride that is no multiple of 4": t(2, 40, 130)[:, :, :128], "a base that is not 16-byte aligned": wide[:, :, 2:130],
               "rows that do not collapse into one stride": t(2, 48, 128)[:, :40]}
    for what, bad in refused.items():
        assert not ops.token_layers_applies(bad, w, b, ln), what
        assert not ops.token_layers_applies(bad, ln=ln), what
        for fn in (ops.token_linear, ops.token_linear_train):
            with pytest.raises(RuntimeError, match=r"multiples of 64.*got act None, x \(2, \d+, \d+\)"):
                fn(bad, w if bad.shape[-1] == 128 else t(64, bad.shape[-1]), b)
        for fn in (ops.layer_norm, ops.layer_norm_train):
            with pytest.raises(RuntimeError, match=r"multiple of 64.*got x \(2, \d+, \d+\)"):
                fn(bad, g, g)
    assert ops.token_layers_applies(wide[:, :, 4:132], w, b, ln)                        # a 16-byte aligned slice of a wider row is in the domain
    assert not ops.token_layers_applies(t(4, 320), t(64, 320), None, (t(320), t(320), EPS))      # a LayerNorm over more than 256 channels
    assert ops.token_layers_applies(t(4, 320), t(64, 320))
    assert not ops.token_layers_applies(x, w, b, ln, "tanh") and not ops.token_layers_applies(x, w, t(32), ln)
    assert not ops.token_layers_applies(x, w, b, ln, None, t(2, 40, 128))               # a residual of another width
    assert not ops.token_layers_applies(x, w, b, dropout_p=0.1, training=True) and ops.token_layers_applies(x, w, b, dropout_p=0.1, training=False)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.token_linear(x, w, b, out=t(2, 40, 128))
    ops.set_token_layers(False)
    assert not ops.token_layers_applies(x, w, b, ln) and not ops.token_layers_applies(x, ln=ln)      # off: the modules keep torch's ops
    assert ops.token_linear(x, w, b, ln=ln).shape == (2, 40, 64)                        # the ops themselves do not depend on the switch
    # the C ABI refuses the same, with its codes
    L, st = _lib.lib(), _lib.current_stream()
    x2, y2 = x.view(80, 128), torch.empty(80, 64, device=dev)
    p = _lib.ptr
    fwd = lambda ldx=128, K=128, N=64, act=0, R=80: L.forge_token_linear_fwd(p(x2), ldx, p(w), p(b), p(g), p(g), EPS, None, 0, p(y2), 64, None, None, R, K, N, act, st)
    assert fwd(K=96) == -2 and b"multiples of 64" in L.forge_last_error()
    assert fwd(ldx=130) == -2 and b"stride" in L.forge_last_error()
    assert fwd(act=2) == -1 and b"act=2" in L.forge_last_error()
    assert fwd(R=0) == -1 and b"rows" in L.forge_last_error()
    assert fwd() == 0
    torch.cuda.synchronize()


# ---- the wiring: CrossAttention + SelfAttention, the 3-D Block, then the whole estimators

@pytest.fixture()
def all_sites(monkeypatch):
    """The 2-D estimator's call sites stay on torch as shipped (ops.TOKEN_SITES_ON_TORCH: they did not win in profiles/r16_token_layers_probe.txt);
    their wiring is exercised with the set emptied."""
    monkeypatch.setattr(ops, "TOKEN_SITES_ON_TORCH", frozenset())


def test_sites_that_did_not_win_stay_on_torch_with_the_switch_on(dev, switch_on):
    from forge_amd.flopmeter import FlopMeter
    from forge_amd.pose_estimator_3d import Block
    assert ops.TOKEN_SITES_ON_TORCH == {"2d.proj", "2d.o_proj", "2d.fc1", "2d.fc2", "2d.norm"}
    cross, selfa, feat, canon, w = blocks(dev)
    blk = Block(dim=64, mlp_ratio=2).to(dev)
    tok = torch.randn(1, 256, 64, device=dev)
    with FlopMeter() as fm:
        block_grads(cross, selfa, feat, canon, w)
    assert fm.launches["forge_token_linear_fwd"] == 0 and fm.launches["forge_token_linear_bwd"] == 0
    with FlopMeter() as fm, torch.no_grad():
        blk.forward_tokens(tok, tok)
    assert fm.launches["forge_token_linear_fwd"] == 5


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
    """(called under the all_sites fixture)"""
    if not _BLOCKS:
        cross, selfa, feat, canon, w = blocks(dev)
        names = ["feat", "canon"] + ["cross." + n for n, _ in cross.named_parameters()] + ["self." + n for n, _ in selfa.named_parameters()]
        from forge_amd.flopmeter import FlopMeter
        prev = ops.set_token_layers(False)
        try:
            block_grads(cross, selfa, feat, canon, w)                                  # warm-up: the BLAS library settles its kernel choice on first use
            with FlopMeter() as fm_off:
                off = block_grads(cross, selfa, feat, canon, w)
            ops.set_token_layers(True)
            with FlopMeter() as fm_on:
                on = block_grads(cross, selfa, feat, canon, w)
            on2 = block_grads(cross, selfa, feat, canon, w)
            with torch.no_grad():
                infer = selfa(cross(x_q=feat, x_k=canon, x_v=canon, residual=feat))
        finally:
            ops.set_token_layers(prev)
        f64 = block_grads(*blocks(dev, torch.float64))
        _BLOCKS.update(names=names, off=off, on=on, on2=on2, infer=infer, f64=f64, launches={"off": fm_off.launches, "on": fm_on.launches}, flops=fm_on.flops)
    return _BLOCKS


def test_blocks_take_the_kernels_only_with_the_switch(dev, all_sites):
    r = block_runs(dev)
    new = ("forge_token_linear_fwd", "forge_token_linear_bwd")
    # per block: q, k, v projections, o_proj, fc1, fc2
    assert [r["launches"]["off"][n] for n in new] == [0, 0] and [r["launches"]["on"][n] for n in new] == [12, 12]
    rows_q, rows_k = 512, 256
    fwd = 2.0 * 256 * 256 * ((rows_q + 2 * rows_k + rows_q) + 4 * rows_q) + 2.0 * 4 * rows_q * 256 * 1024
    assert r["flops"]["forge_token_linear_fwd"] == fwd and r["flops"]["forge_token_linear_bwd"] == 2 * fwd
    assert any(not torch.equal(a, b) for a, b in zip(r["on"][1], r["off"][1]))          # on: other bits, the same function (next test)
    assert torch.equal(r["on"][0], r["on2"][0]) and all(torch.equal(a, b) for a, b in zip(r["on"][1], r["on2"][1]))     # and they repeat
    assert torch.equal(r["on"][0], r["infer"])                                          # the inference forms: the same bits


def test_blocks_output_and_gradients_vs_float64(dev, all_sites):
    """Output, input gradients and every parameter gradient of CrossAttention -> SelfAttention with the switch on against the same modules in
    float64, the switch-off fp32 run as yardstick, rule eh <= 2 et + 1e-6 per tensor (errors relative to the tensor's float64 maximum; the two
    k_proj biases, whose exact gradient is zero - a key bias shifts every logit of a row alike - relative to their weight's gradient, the scale of
    what cancels, as tests/test_gpu_attention_mh.py has it)."""
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


def test_3d_block_at_256_tokens_vs_float64(dev):
    """pose_estimator_3d.Block (dim 64, mlp_ratio 2) on 256 tokens: the tokens-major inference route and the [B,C,N] training route with the switch
    on against the float64 module, the switch-off fp32 run as yardstick (rule as above), and five token launches forward per Block."""
    from forge_amd.flopmeter import FlopMeter
    from forge_amd.pose_estimator_3d import Block
    torch.manual_seed(11)
    blk = Block(dim=64, mlp_ratio=2).to(dev)
    for p in blk.parameters():                                                          # biases and LayerNorm parameters off their initial 0 / 1
        if p.dim() == 1:
            p.data.add_(0.3 * torch.randn_like(p))
    g = torch.Generator(device=dev).manual_seed(12)
    q, k, w = (torch.randn(2, 64, 256, device=dev, generator=g) * s for s in (0.5, 0.5, 1.0))
    blk64 = copy.deepcopy(blk).double()

    def grads(m, q, k, w):
        q, k = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
        out = m(q, k)
        return (out.detach(),) + torch.autograd.grad((out * w).sum(), [q, k] + list(m.parameters()))

    names = ["out", "q", "k"] + [n for n, _ in blk.named_parameters()]
    prev = ops.set_token_layers(False)
    try:
        off, f64 = grads(blk, q, k, w), grads(blk64, q.double(), k.double(), w.double())
        ops.set_token_layers(True)
        with FlopMeter() as fm:
            on = grads(blk, q, k, w)
        with torch.no_grad():
            tok = blk.forward_tokens(q.permute(0, 2, 1).contiguous(), k.permute(0, 2, 1).contiguous())
    finally:
        ops.set_token_layers(prev)
    assert fm.launches["forge_token_linear_fwd"] == 5 and fm.launches["forge_token_linear_bwd"] == 5
    assert rel(tok.permute(0, 2, 1), f64[0]) <= FACTOR * rel(off[0], f64[0]) + 1e-6
    bad = []
    for name, got, t32, want in zip(names, on, off, f64):
        eh, et = rel(got, want), rel(t32, want)
        report("3-D Block d/d %-24s hip/f64 %.2e torch/f64 %.2e ratio %.2f" % (name, eh, et, eh / max(et, 1e-30)))
        if not (got.shape == want.shape and eh <= FACTOR * et + 1e-6):
            bad.append((name, eh, et))
    assert not bad, bad


def _double(mod):
    ref = copy.deepcopy(mod).double()
    for m in ref.modules():
        for k, v in list(vars(m).items()):
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(m, k, v.double())
    return ref


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_whole_estimators_with_all_three_switches_vs_float64(dev, which, all_sites):
    """PoseEstimator2D on [1,2,3,256,256] (every call site on the kernels) and PoseEstimator3D on a 32^3 volume pair with the three opt-in switches on, in eval mode (no autograd
    graph) and in training mode (grad mode; batch statistics in the 3-D estimator - the 2-D one ends in a BatchNorm over ONE 1 x 1 map here, which
    has no batch statistics, so its BatchNorm layers stay in eval mode as in a fine-tune), against tools/stock_pose.py's evaluation of the same
    module in float64 on the host;
    the bound tests/test_gpu_configs.py uses for these modules: 3 x the distance of the stock fp32 evaluation on the GPU + 2e-5."""
    import stock_pose
    from forge_amd.flopmeter import FlopMeter
    torch.manual_seed(5)
    if which == "2d":
        from forge_amd.pose_estimator_2d import PoseEstimator2D
        mod, x, launches = PoseEstimator2D(), torch.rand(1, 2, 3, 256, 256), 36
    else:
        from forge_amd.pose_estimator_3d import PoseEstimator3D
        mod, x, launches = PoseEstimator3D(syn.kubric_config()), torch.randn(1, 2, 128, 32, 32, 32) * 0.5, 7
    sd = syn.seeded_state_dict({"m." + k: v for k, v in mod.state_dict().items()}, 13)
    mod.load_state_dict({k[2:]: v for k, v in sd.items()})
    ref_mod, g, stock_g, xd = _double(mod), copy.deepcopy(mod).to(dev), copy.deepcopy(mod).to(dev), x.to(dev)
    relc = lambda got, want: (got.detach().double().cpu() - want).abs().max().item() / want.abs().max().item()
    prev = ops.set_token_layers(False), ops.set_multihead_attention(False), ops.set_attention_training(False)
    try:
        for training in (False, True):
            for m in (ref_mod, g, stock_g):
                m.train(training)
                if which == "2d":
                    for sub in m.modules():
                        if isinstance(sub, torch.nn.modules.batchnorm._BatchNorm):
                            sub.eval()
            ops.set_token_layers(False), ops.set_multihead_attention(False), ops.set_attention_training(False)
            with torch.set_grad_enabled(training):
                ref = stock_pose.stock_forward(ref_mod)(x.double(), return_features=True).detach()
                stock_ = stock_pose.stock_forward(stock_g)(xd, return_features=True)
                ops.set_token_layers(True), ops.set_multihead_attention(True), ops.set_attention_training(True)
                with FlopMeter() as fm:
                    on = g(xd, return_features=True)
            assert fm.launches["forge_token_linear_fwd"] == launches and fm.launches["forge_token_linear_bwd"] == 0
            eh, es = relc(on, ref), relc(stock_, ref)
            report("PoseEstimator%s %s features: switches on/f64 %.2e, stock/f64 %.2e" % (which.upper(), "training" if training else "eval", eh, es))
            assert on.shape == ref.shape and eh <= 3.0 * es + 2e-5, (which, training, eh, es)
    finally:
        ops.set_token_layers(prev[0]), ops.set_multihead_attention(prev[1]), ops.set_attention_training(prev[2])


def test_joint_step_gradients_bitwise_reproducible_with_all_three_switches(dev):
    """The twin of tests/test_gpu_deterministic.py::test_joint_step_gradients_bitwise_reproducible with the three opt-in switches on: the joint
    configs[4] step run twice gives bitwise-identical gradients for every parameter and the same loss, and it runs the token kernels."""
    from forge_amd.flopmeter import FlopMeter
    from test_gpu_configs import joint_training_step
    prev = ops.set_token_layers(True), ops.set_multihead_attention(True), ops.set_attention_training(True)
    runs = []
    try:
        for _ in range(2):
            with FlopMeter() as fm:
                loss, _, model, _, _ = joint_training_step(dev)
            assert fm.launches["forge_token_linear_fwd"] > 0 and fm.launches["forge_token_linear_bwd"] == fm.launches["forge_token_linear_fwd"]
            runs.append((loss.clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
            del model
    finally:
        ops.set_token_layers(prev[0]), ops.set_multihead_attention(prev[1]), ops.set_attention_training(prev[2])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.isfinite(runs[0][0]).all()
    assert runs[0][1].keys() == runs[1][1].keys() and len(runs[0][1]) > 0
    diff = [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
    assert not diff, diff[:8]
