"""GPU (-m gpu): every fusion schedule of ConvGRU_3D against a float64 reference, over the shape cases of tests/convgru_cases.py.

  S1  fuse_hip (_fuse_eval, fused GRU epilogues), also through ConvGRU_3D.forward with a caller h0 and with none
  S2  fuse_groups_hip (input halves shared between groups)
  S3  fuse_frozen_hip / _FuseFrozen (hand-written data-gradient backward; skip_dx0, const0)
  S4  fuse_autograd_hip (_GRUCellRows, batch-statistics BatchNorm)
  S5  fuse_groups_autograd_hip: the _FuseGroupsTrain node or the per-step _GRUCellPreRows fallback (which one ran is asserted)
  S6  ConvGRU_3D.forward with input != hidden or two layers (ConvGRUCell_3D)

The reference is forge_oracle's fusion evaluated in float64 on the CPU (convgru_cases.ref_fuse), with float64 autograd for the gradients
(one fixed random cotangent per output) and the running statistics after the step (momentum 0.1, unbiased variance; S5: one update per
group, in group order). Each reference is computed once per case and shared by the schedules of the same semantics. Every comparison is
max |got - ref| / max |ref| of the tensor; gradients that are analytically zero (conv biases in front of a train-mode BatchNorm) get an
absolute bound relative to the largest parameter gradient. Bounds are ~4x the largest value measured on the MI355X over the matrix
(FORGE_TEST_REPORT=1 prints every comparison). The fusion_conv BatchNorm shifts are pinned a hair away from their seeded values so that no
LeakyReLU pre-activation lies within rounding distance of zero (convgru_cases.pin_lrelu_signs); each reference verifies that margin.
"""
import os

import pytest
import torch

import convgru_cases as cc
import forge_amd
import forge_oracle as fo
from forge_amd import convops as co, fusion, synthetic as syn
from forge_amd.fusion import ConvGRU_3D

pytestmark = pytest.mark.gpu

# bounds: ~4x the largest value measured on the MI355X over the whole matrix (relative to max |reference| of the tensor)
FWD = 1e-5           # outputs: measured 2.2e-6 (S1 case f, forward with a caller h0)
RUNNING = 1.5e-6     # running statistics: measured 3.0e-7 (S5 case g, fusion_conv.4.running_var)
DX = 5e-6            # input gradients: measured 1.1e-6 (S5 case f)
WGRAD = 2.5e-5       # weight gradients (fp32 atomics, or the deterministic slabs): measured 5.7e-6 (S5 case b, out_gate.bias)
WGRAD_ZERO = 3e-6    # |gradient| / largest parameter gradient where it is analytically zero (conv bias before a train-mode BatchNorm): 6.8e-7
LRELU_MARGIN = 2e-6  # min |v| / max |v| of the fusion_conv LeakyReLU pre-activations of a reference (fp32 rounding of v: ~3e-8 typical, 5e-7 worst)
SEED = 9

_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from forge_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def report(tag, err, bound):
    if os.environ.get("FORGE_TEST_REPORT"):
        print("  convgru %-44s %.2e  (bound %.0e)" % (tag, err, bound))


def rel(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def check(tag, got, ref, bound, floor=None):
    scale = max(ref.abs().max().item(), floor or 0.0)
    err = (got.detach().double().cpu() - ref).abs().max().item() / scale
    report(tag, err, bound)
    assert err < bound, (tag, err, bound)
    return err


def make_inputs(case):
    """(x fp32 [b,t,C,D,H,W], w fp32 state dict with pinned fusion_conv shifts, cotangents): deterministic per case."""
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=case.C, hidden_size=case.C)
    w = syn.seeded_state_dict(gru.state_dict(), SEED)
    gen = torch.Generator().manual_seed(ord(case.name))
    x = torch.randn(case.b, cc.T, case.C, case.D, case.H, case.W, generator=gen) * 0.5
    cc.pin_lrelu_signs(x, w, case.groups)
    gys = {g: torch.randn(case.b, case.C, case.D, case.H, case.W, generator=gen, dtype=torch.float64) for g in case.groups}
    return x, w, gys


def ref(name):
    """The float64 references of a case (computed once): eval outputs per group (+ S3's input gradients), train outputs, gradients and
    running statistics per group, the zero-h0 recurrence."""
    if name in _REF:
        return _REF[name]
    case = cc.CASE[name]
    x, w, gys = make_inputs(case)
    wd = {k: v.double() for k, v in w.items()}
    xd = x.double()
    full = tuple(range(cc.T))
    r = dict(x=x, w=w, gys=gys, eval={}, train={}, margins=[])
    for g in case.groups:
        log = {}
        if g == full and name in S3_CASES:
            xg = xd.clone().requires_grad_(True)
            out = cc.ref_fuse(xg, wd, False, log=log)
            out.backward(gys[g])
            r["s3"] = dict(dx=xg.grad.clone(), dmean=log["m"].grad.clone())
            out = out.detach()
        else:
            with torch.no_grad():
                out = cc.ref_fuse(xd[:, list(g)], wd, False, log=log)
        r["eval"][g] = out
        r["margins"].append(cc.lrelu_margin(log))
        if g == full:
            r["h0"] = log["h0"].detach().float()
    with torch.no_grad():
        r["zero_h0"] = cc.ref_fuse(xd, wd, False, h0=torch.zeros(case.b, case.C, case.D, case.H, case.W, dtype=torch.float64))
    params = {k: v.clone().requires_grad_(True) for k, v in wd.items() if "running" not in k and "num_batches" not in k}
    for g in case.groups:
        log = {}
        xg = xd.clone().requires_grad_(True)
        out = cc.ref_fuse(xg[:, list(g)], dict(wd, **params), True, log=log)
        keys = list(params)
        grads = torch.autograd.grad(out, [xg] + [params[k] for k in keys], gys[g])
        r["train"][g] = dict(out=out.detach(), dx=grads[0], dw=dict(zip(keys, grads[1:])), stats=log["stats"])
        r["margins"].append(cc.lrelu_margin(log))
    assert min(r["margins"]) > LRELU_MARGIN, "case %s: a fusion_conv LeakyReLU pre-activation lies within %.1e of zero: pick another seed" % (
        name, min(r["margins"]))
    _REF[name] = r
    return r


S3_CASES = ("b", "c", "e", "g")
ALL = [c.name for c in cc.CASES]


@pytest.fixture
def case_env(request, monkeypatch):
    """The case of the test's `name` parameter with its operand limit applied; asserts the path / form table first."""
    def enter(name):
        case = cc.CASE[name]
        if case.small_limit:
            monkeypatch.setattr(co, "MAX_OPERAND_BYTES", cc.operand_limit(case))
        assert cc.paths(co, case) == case.expect, "case %s left its path / form" % name
        return case
    return enter


def module(case, w, dev, train):
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=case.C, hidden_size=case.C)
    gru.load_state_dict(w)
    gru = gru.to(dev)
    return gru.train() if train else gru.eval()


# ------------------------------------------------------------------------------------------------------------ S1 / S2: inference
@pytest.mark.parametrize("name", ALL)
def test_s1_fuse_hip(dev, case_env, name):
    """fuse_hip, forward(x, [h0]) with the reference's fusion_conv output as the caller's h0, and forward(x) (zero h0) vs float64."""
    case = case_env(name)
    r = ref(name)
    gru = module(case, r["w"], dev, False)
    x = r["x"].to(dev)
    full = tuple(range(cc.T))
    with torch.no_grad():
        check("S1 %s fuse_hip" % name, gru.fuse_hip(x), r["eval"][full], FWD)
        check("S1 %s forward(h0)" % name, gru(x, [r["h0"].to(dev)]), r["eval"][full], FWD)
        check("S1 %s forward()" % name, gru(x), r["zero_h0"], FWD)


@pytest.mark.parametrize("name", ALL)
def test_s2_fuse_groups_hip(dev, case_env, name):
    case = case_env(name)
    r = ref(name)
    gru = module(case, r["w"], dev, False)
    with torch.no_grad():
        outs = gru.fuse_groups_hip(r["x"].to(dev), [list(g) for g in case.groups])
    for g, o in zip(case.groups, outs):
        check("S2 %s %s" % (name, g), o, r["eval"][g], FWD)


# ------------------------------------------------------------------------------------------------------------ S3: frozen weights
def _frozen(case, r, dev):
    gru = module(case, r["w"], dev, False)
    for p in gru.parameters():
        p.requires_grad_(False)
    return gru


def _frozen_expect(r, skip):
    dx = r["s3"]["dx"].clone()
    if skip:
        dx[:, 0] = r["s3"]["dmean"] / cc.T          # view 0 keeps the fusion_conv(mean) share only
    return dx


@pytest.mark.parametrize("skip", [False, True], ids=["full", "skip_dx0"])
@pytest.mark.parametrize("name", S3_CASES)
def test_s3_fuse_frozen(dev, case_env, name, skip):
    case = case_env(name)
    r = ref(name)
    gru = _frozen(case, r, dev)
    full = tuple(range(cc.T))
    x = r["x"].to(dev).requires_grad_(True)
    out = gru.fuse_frozen_hip(x, skip_dx0=skip)
    out.backward(r["gys"][full].float().to(dev))
    check("S3 %s %s out" % (name, "skip" if skip else "full"), out, r["eval"][full], FWD)
    check("S3 %s %s dx" % (name, "skip" if skip else "full"), x.grad, _frozen_expect(r, skip), DX)


@pytest.mark.parametrize("name", S3_CASES)
def test_s3_const0_reuse(dev, case_env, name):
    """const0: the second call adds the cached input-half products of view 0; both calls meet the float64 bounds."""
    case = case_env(name)
    r = ref(name)
    gru = _frozen(case, r, dev)
    full = tuple(range(cc.T))
    const0 = {}
    for call in (1, 2):
        x = r["x"].to(dev).requires_grad_(True)
        out = gru.fuse_frozen_hip(x, skip_dx0=True, const0=const0)
        out.backward(r["gys"][full].float().to(dev))
        check("S3 %s const0 call %d out" % (name, call), out, r["eval"][full], FWD)
        check("S3 %s const0 call %d dx" % (name, call), x.grad, _frozen_expect(r, True), DX)
    assert bool(const0) == case.expect["frozen_wino"]


# ------------------------------------------------------------------------------------------------------------ S4 / S5: training
def check_param_grads(tag, gru, dw):
    """Every parameter gradient of gru against dw (float64, None: the parameter takes no part). An analytically zero gradient - float64
    at rounding level - is bounded absolutely, relative to the largest parameter gradient."""
    gscale = max(v.abs().max().item() for v in dw.values() if v is not None)
    for k, p in gru.named_parameters():
        if dw[k] is None:
            assert p.grad is None, k
        elif dw[k].abs().max().item() < 1e-9 * gscale:
            check("%s d %s (zero)" % (tag, k), p.grad, dw[k], WGRAD_ZERO, floor=gscale)
        else:
            check("%s d %s" % (tag, k), p.grad, dw[k], WGRAD)


def _check_train(tag, gru, x, outs, groups, r):
    """Outputs, dx, every parameter gradient and the running statistics against the float64 sums over `groups`."""
    for g, o in zip(groups, outs):
        check("%s out %s" % (tag, g), o, r["train"][g]["out"], FWD)
    dx = sum(r["train"][g]["dx"] for g in groups)
    check("%s dx" % tag, x.grad, dx, DX)
    check_param_grads(tag, gru, {k: sum(r["train"][g]["dw"][k] for g in groups) for k in r["train"][groups[0]]["dw"]})
    run = cc.running_after(r["w"], [s for g in groups for s in r["train"][g]["stats"]])
    for k, (rm, rv) in run.items():
        bn = gru.get_submodule(k)
        check("%s %s.running_mean" % (tag, k), bn.running_mean, rm, RUNNING, floor=1.0)
        check("%s %s.running_var" % (tag, k), bn.running_var, rv, RUNNING, floor=1.0)


def _s4(case, r, dev):
    gru = module(case, r["w"], dev, True)
    x = r["x"].to(dev).requires_grad_(True)
    out = gru.fuse_autograd_hip(x)
    out.backward(r["gys"][tuple(range(cc.T))].float().to(dev))
    return gru, x, out


@pytest.mark.parametrize("name", ALL)
def test_s4_fuse_autograd(dev, case_env, name):
    case = case_env(name)
    r = ref(name)
    gru, x, out = _s4(case, r, dev)
    _check_train("S4 %s" % name, gru, x, [out], [tuple(range(cc.T))], r)


def _s5(case, r, dev, monkeypatch):
    calls = []
    orig = fusion._FuseGroupsTrain.apply
    monkeypatch.setattr(fusion._FuseGroupsTrain, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    gru = module(case, r["w"], dev, True)
    x = r["x"].to(dev).requires_grad_(True)
    outs = gru.fuse_groups_autograd_hip(x, [list(g) for g in case.groups])
    sum((o * r["gys"][g].float().to(dev)).sum() for g, o in zip(case.groups, outs)).backward()
    monkeypatch.setattr(fusion._FuseGroupsTrain, "apply", orig)
    return gru, x, outs, bool(calls)


@pytest.mark.parametrize("name", ALL + ["d_direct"])
def test_s5_fuse_groups_autograd(dev, case_env, monkeypatch, name):
    """d_direct: case d under convops.winograd(False) - the fallback on the direct kernels."""
    base = name.split("_")[0]
    if name.endswith("_direct"):
        monkeypatch.setattr(co.STATE, "winograd", False)
    case = cc.CASE[base]
    if name.endswith("_direct"):
        assert not cc.paths(co, case)["node"]
        expect_node = False
    else:
        case_env(base)
        expect_node = case.expect["node"]
    r = ref(base)
    gru, x, outs, node = _s5(case, r, dev, monkeypatch)
    assert node == expect_node, "S5 %s: %s ran" % (name, "the node" if node else "the fallback")
    _check_train("S5 %s" % name, gru, x, outs, list(case.groups), r)


# ------------------------------------------------------------------------------------------------------------ deterministic mode
@pytest.mark.parametrize("sched", ["S4", "S5"])
def test_deterministic_mode_bitwise_and_within_bounds(dev, case_env, monkeypatch, sched):
    case = case_env("e")
    r = ref("e")
    runs = []
    with forge_amd.deterministic(True):
        for _ in range(2):
            if sched == "S4":
                gru, x, out = _s4(case, r, dev)
                outs = [out]
                _check_train("det S4 e", gru, x, outs, [tuple(range(cc.T))], r)
            else:
                gru, x, outs, node = _s5(case, r, dev, monkeypatch)
                assert node
                _check_train("det S5 e", gru, x, outs, list(case.groups), r)
            runs.append([o.detach().clone() for o in outs] + [x.grad.clone()] + [p.grad.clone() for p in gru.parameters()]
                        + [b.clone() for b in gru.buffers()])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), sched


# ------------------------------------------------------------------------------------------------------------ S6: the generic module
@pytest.mark.parametrize("cin,hid,layers", [(64, 128, 1), (128, 32, 1), (64, 64, 2)])
def test_s6_generic_forward_autograd(dev, cin, hid, layers):
    """ConvGRU_3D.forward (ConvGRUCell_3D per layer and view, zero initial state, fusion_norm in train mode) under autograd vs float64."""
    torch.manual_seed(3)
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=layers, input_size=cin, hidden_size=hid)
    w = syn.seeded_state_dict(gru.state_dict(), SEED)
    gru.load_state_dict(w)
    gru = gru.to(dev).train()
    gen = torch.Generator().manual_seed(cin + hid + layers)
    x = torch.randn(2, 3, cin, 4, 16, 16, generator=gen) * 0.5
    gy = torch.randn(2, hid, 4, 16, 16, generator=gen, dtype=torch.float64)
    wd = {k: v.double().requires_grad_("running" not in k and "num_batches" not in k) for k, v in w.items()}
    xd = x.double().requires_grad_(True)
    cur, h = xd, None
    for layer in range(layers):
        hs = []
        h = torch.zeros(2, hid, 4, 16, 16, dtype=torch.float64)
        for t in range(x.shape[1]):
            h = fo.conv_gru_cell(cur[:, t], h, wd, "cells.%d" % layer)
            hs.append(h)
        cur = torch.stack(hs, dim=1)
    log = {}
    refo = cc._bn(h, wd, "fusion_norm", True, log)
    refo.backward(gy)
    xg = x.to(dev).requires_grad_(True)
    out = gru(xg)
    out.backward(gy.float().to(dev))
    tag = "S6 %d->%d x%d" % (cin, hid, layers)
    check(tag + " out", out, refo.detach(), FWD)
    check(tag + " dx", xg.grad, xd.grad, DX)
    check_param_grads(tag, gru, {k: wd[k].grad for k, _ in gru.named_parameters()})
    rm, rv = cc.running_after(w, log["stats"])["fusion_norm"]
    check(tag + " running_mean", gru.fusion_norm.running_mean, rm, RUNNING, floor=1.0)
    check(tag + " running_var", gru.fusion_norm.running_var, rv, RUNNING, floor=1.0)


# ------------------------------------------------------------------------------------------------------------ the bounds catch something
MUTATIONS = {"gates_swapped": dict(swap=True), "slope_0.02": dict(slope=0.02), "mean_over_t-1": dict(mean_div=cc.T - 1)}


@pytest.mark.parametrize("sched", ["S1", "S2", "S3", "S4", "S5"])
def test_bounds_reject_wrong_references(dev, case_env, monkeypatch, sched):
    """The HIP output of each schedule family at case d misses three deliberately wrong float64 references by >= 10x the forward bound.
    (Train mode skips the view mean divided by t - 1: batch statistics normalise the scale of the mean away, so that mistake does not
    change a train-mode result at all.)"""
    case = case_env("d")
    r = ref("d")
    full = tuple(range(cc.T))
    x = r["x"].to(dev)
    train = sched in ("S4", "S5")
    if sched == "S1":
        with torch.no_grad():
            got = module(case, r["w"], dev, False).fuse_hip(x)
    elif sched == "S2":
        with torch.no_grad():
            got = module(case, r["w"], dev, False).fuse_groups_hip(x, [list(g) for g in case.groups])[list(case.groups).index(full)]
    elif sched == "S3":
        got = _frozen(case, r, dev).fuse_frozen_hip(x.requires_grad_(True))
    elif sched == "S4":
        got = module(case, r["w"], dev, True).fuse_autograd_hip(x)
    else:
        got = _s5(case, r, dev, monkeypatch)[2][list(case.groups).index(full)]
    good = r["train" if train else "eval"][full]
    good = good["out"] if train else good
    report("%s d vs the reference" % sched, rel(got, good), FWD)
    assert rel(got, good) < FWD
    wd = {k: v.double() for k, v in r["w"].items()}
    errs = {}
    for k, kw in MUTATIONS.items():
        if train and "mean_div" in kw:
            continue
        with torch.no_grad():
            errs[k] = rel(got, cc.ref_fuse(r["x"].double(), wd, train, **kw))
        report("%s d vs wrong reference %s" % (sched, k), errs[k], 10 * FWD)
    assert all(e >= 10 * FWD for e in errs.values()), (sched, errs)
