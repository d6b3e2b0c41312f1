"""CPU: the restatements of tests/pointwise_cases.py against independent ones (autograd, torch.optim.Adam, F.mse_loss, F.unfold, explicit windows), the
wrong readings of every section against the very bounds the GPU test uses with the float32 yardstick standing in for the kernel, and the host-side
refusals (nothing is launched) - before tests/test_gpu_pointwise_matrix.py spends a GPU on any of it."""
import ctypes

import pytest
import torch

import pointwise_cases as pc
from forge_amd import _lib


@pytest.fixture(scope="module")
def L(built_lib):
    return _lib.lib()


def _close(a, b, tol=1e-12):
    nm = ~torch.isnan(b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and (a[nm] - b[nm]).abs().max().item() <= tol * max(1.0, b[nm].abs().max().item())


def _yard(fn):
    with pc.yardstick_threads():
        return fn()


# ---- GRU halves
@pytest.mark.parametrize("name", [c.name for c in pc.GRU_CASES])
def test_gru_restatement(name):
    """Forward: sigmoid and tanh by their exponentials. State backward: autograd through hn = h (1 - z) + cand z at the saved values. Gates backward:
    the derivative written the other way round. The accumulator rows by an explicit loop over the batches."""
    c = pc.GRU_CASE[name]
    d = pc.gru_data(c)
    o = pc.gru_eval(c, d)
    C = c.C
    g, cp = d["g"].double(), d["c"].double()
    assert _close(1 / (1 + torch.exp(-g[:, :C])), o["z"]) and _close(1 / (1 + torch.exp(-g[:, C:])), o["r"])
    assert _close(torch.expm1(2 * cp) / (torch.exp(2 * cp) + 1), o["cand"])
    assert g.abs().max() == 20 and cp.abs().max() == 20 and (d["z"] == 1).any() and (d["cand"].abs() == 1).any(), "the data does not saturate"
    h, z, cand = (d[k].double().clone().requires_grad_(True) for k in ("h", "z", "cand"))
    (h * (1 - z) + cand * z).backward(d["dhn"].double())
    assert _close(h.grad, o["s_dh"]) and _close(z.grad, o["s_dz"]) and _close(cand.grad * (1 - d["cand"].double() ** 2), o["s_dc"])
    zs, rs, hh = d["z"].double(), d["r"].double(), d["h"].double()
    dg = torch.cat([d["dz_in"].double() * (zs - zs * zs), d["dhr"].double() * hh * (rs - rs * rs)], dim=1)
    assert _close(dg, o["g_dg"])
    if c.acc_mode:
        for key, val, prior in (("s_acc", o["s_dc"], d["prior_c"]), ("g_acc", dg, d["prior_g"])):
            want = torch.full(o[key].shape, pc.NAN, dtype=torch.float64)
            for b in range(c.M // c.vol):
                rows = slice(b * 3 * c.vol, b * 3 * c.vol + c.vol)
                want[rows] = val[b * c.vol:(b + 1) * c.vol] + (prior.double()[rows] if c.acc_mode == 2 else 0)
            assert _close(want, o[key]), (name, key)
            assert torch.isnan(o[key]).sum() == (c.M // c.vol - 1) * 2 * c.vol * val.shape[1], "the rows between the batches"


@pytest.mark.parametrize("name", [c.name for c in pc.GRU_CASES])
def test_gru_wrong_readings(name):
    c = pc.GRU_CASE[name]
    d = pc.gru_data(c)
    ref, yard = pc.gru_eval(c, d), _yard(lambda: pc.gru_eval(c, d, torch.float32))
    assert not pc.compare_all(yard, ref, yard)[1], name
    for mut in c.muts.split():
        assert pc.compare_all(yard, pc.gru_eval(c, d, mut=mut), yard, true=ref)[1], (name, mut, "a wrong reading passes: a case is missing")


def test_gru_coverage():
    cs = pc.GRU_CASES
    assert {c.C for c in cs} == {4, 8, 128} and {c.M for c in cs} == {1, 7, 1000}
    assert any((c.M * c.C // 4) % 256 and c.M * c.C // 4 > 256 for c in cs)
    assert {c.acc_mode for c in cs} == {0, 1, 2} and all(c.M % c.vol == 0 for c in cs)
    assert any(c.acc_mode == m and c.M // c.vol > 1 for c in cs for m in (1, 2)) and all(any(c.acc_mode == m and c.M // c.vol > 1 for c in cs) for m in (1, 2))
    assert any(c.dh_out is None for c in cs) and any(c.dh_out == "alias" and c.ld_dhr > c.C for c in cs) and any(isinstance(c.dh_out, int) and c.dh_out > c.C for c in cs)
    assert any(c.ld_dhn > c.C for c in cs) and any(c.ld_dhr > c.C for c in cs)
    assert {m for c in cs for m in c.muts.split()} == set(pc.GRU_MUTATIONS)


# ---- affine_act_bwd
@pytest.mark.parametrize("name", [c.name for c in pc.AFF_CASES])
def test_affine_restatement_and_wrong_readings(name):
    """The two float32 products against autograd of y = lrelu(pre) scale at the sign the saved output has, in float64: within one rounding each. Zero
    of either sign takes the slope side, the smallest denormal the other."""
    c = pc.AFF_CASE[name]
    d = pc.aff_data(c)
    got = pc.aff_eval(c, d)["dx"][:, :c.C]
    sc = d["scale"].double() if d["scale"] is not None else torch.ones(c.C, dtype=torch.float64)
    want = d["dy"].double() * sc * torch.where(d["y"] > 0, 1.0, pc.f32(c.slope))
    assert (got.double() - want).abs().max().item() <= 2 * pc.U * max(1.0, want.abs().max().item())
    y, flat = d["y"].view(-1), got.reshape(-1)
    g = (d["dy"] * d["scale"] if d["scale"] is not None else d["dy"]).reshape(-1)
    slope = torch.tensor(c.slope, dtype=torch.float32)
    assert y[0] == 0 and y[1] == 0 and torch.signbit(y[1]) and not torch.signbit(y[0]) and y[2] == pc.DENORM > 0
    assert torch.equal(flat[:2], (g * slope)[:2]) and flat[2] == g[2]
    assert {cc.slope for cc in pc.AFF_CASES} == {0.0, 0.01, 1.0} and {cc.C for cc in pc.AFF_CASES} == {1, 3, 8, 16}
    ref = pc.aff_eval(c, d)
    for mut in c.muts.split():
        assert pc.compare_all(ref, pc.aff_eval(c, d, mut=mut))[1], (name, mut)
    assert {m for cc in pc.AFF_CASES for m in cc.muts.split()} == set(pc.AFF_MUTATIONS)


# ---- sums of squared errors
@pytest.mark.parametrize("name", [c.name for c in pc.SSE_CASES])
def test_sse_restatement_and_wrong_readings(name):
    c = pc.SSE_CASE[name]
    d = pc.sse_data(c)
    ref = pc.sse_eval(c, d)
    per = c.B * c.gsize * c.C * c.H * c.W
    assert _close(ref["sums"] / per, pc.sse_mse(c, d))
    # the gradient of the sums weighted by coef / 2, by autograd through the documented slices
    p = d["pred"].double().clone().requires_grad_(True)
    (pc.sse_mse(c, dict(d, pred=p)) * per * d["coef"].double() / 2).sum().backward()
    assert _close(p.grad, pc.sse_view(c, ref["dpred"])) and torch.isnan(ref["dpred"]).sum() == d["base"].numel() - d["pred"].numel()
    yard = _yard(lambda: pc.sse_eval(c, d, torch.float32))
    b = pc.sse_bound(ref["sums"], yard["sums"])
    for mut in c.muts.split():
        wrong = pc.sse_eval(c, d, mut=mut)
        w32 = _yard(lambda: pc.sse_eval(c, d, torch.float32, mut=mut))
        assert ((yard["sums"].double() - wrong["sums"]).abs() / ref["sums"]).max().item() > b, (name, mut, "forward")
        assert pc.compare(yard["dpred"], w32["dpred"])[3], (name, mut, "backward")


def test_sse_coverage():
    cs = pc.SSE_CASES
    assert {(c.Vp, c.Vt, c.gsize) for c in cs} == {(2, 2, 2), (4, 2, 2), (4, 4, 2), (4, 2, 1), (6, 3, 2), (3, 1, 1)}
    assert {c.Vp // c.gsize for c in cs} == {1, 2, 3, 4} and any(c.Vt > c.gsize and c.Vt % c.gsize == 0 for c in cs) and any(c.Vt % c.gsize for c in cs)
    assert {c.B for c in cs} == {1, 2} and {c.C for c in cs} == {1, 3} and {(c.H, c.W) for c in cs} == {(5, 7), (33, 65)}
    assert {c.layout for c in cs} == {"contig", "cl", "slice", "batch_gap"}
    assert min(c.B * c.Vp * c.C * c.H * c.W for c in cs) < 1024 and {m for c in cs for m in c.muts.split()} == set(pc.SSE_MUTATIONS)
    for c in cs:
        p = pc.sse_data(c)["pred"]
        assert (p.stride(0) != c.Vp * p.stride(1)) == (c.layout == "batch_gap")


# ---- Adam
@pytest.mark.parametrize("n", pc.ADAM_N)
def test_adam_restatement_and_wrong_reading(n):
    """adam_eval against torch.optim.Adam in float64 with the same float hyper-parameters, from the same state."""
    d = pc.adam_data(n)
    ref = pc.adam_eval(d)
    p = d["p"].double().clone().requires_grad_(True)
    hy = {k: pc.f32(v) for k, v in pc.ADAM_HYPER.items()}
    opt = torch.optim.Adam([p], lr=hy["lr"], betas=(hy["b1"], hy["b2"]), eps=hy["eps"])
    opt.state[p] = {"step": torch.tensor(pc.ADAM_STEP0), "exp_avg": d["m"].double().clone(), "exp_avg_sq": d["v"].double().clone()}
    for g in d["grads"]:
        p.grad = g.double().clone()
        opt.step()
    assert _close(p.detach(), ref["p"], 1e-12) and _close(opt.state[p]["exp_avg"], ref["m"]) and _close(opt.state[p]["exp_avg_sq"], ref["v"])
    assert float(opt.state[p]["step"]) == pc.ADAM_STEP0 + pc.ADAM_STEPS
    yard = _yard(lambda: pc.adam_eval(d, torch.float32))
    assert not pc.compare_all(yard, ref, yard, floor=False)[1]
    assert all(ey > 0 for _, _, ey in pc.compare_all(yard, ref, yard, floor=False)[0].values()), "a yardstick that rounds exactly leaves no bound"
    wrong = pc.adam_eval(d, mut="stale_step")
    assert pc.compare(yard["p"], wrong["p"], yard["p"], true=ref["p"], floor=False)[3], "a bias correction one step behind passes"


# ---- im2col, max-pool, transposes: bitwise
@pytest.mark.parametrize("name", [c.name for c in pc.COL_CASES])
def test_im2col_restatement_and_wrong_readings(name):
    c = pc.COL_CASE[name]
    d = pc.col_data(c)
    ref = pc.col_eval(c, d)
    assert torch.equal(ref["out"], pc.col_unfold(c, d)) and (ref["out"][:, c.k * c.k * c.C:] == 0).all()
    for mut in c.muts.split():
        assert pc.compare_all(ref, pc.col_eval(c, d, mut=mut))[1], (name, mut)
    cs = pc.COL_CASES
    assert any(c_.Kpad > c_.k * c_.k * c_.C for c_ in cs) and any(c_.H < c_.k and c_.W < c_.k for c_ in cs) and {m for c_ in cs for m in c_.muts.split()} == set(pc.COL_MUTATIONS)
    assert any((c_.C, c_.H, c_.W, c_.k, c_.stride, c_.pad, c_.Kpad) == (3, 9, 11, 7, 2, 3, 160) for c_ in cs)


@pytest.mark.parametrize("name", [c.name for c in pc.POOL_CASES])
def test_maxpool_restatement_and_wrong_readings(name):
    """F.max_pool2d against explicit windows over the -inf padded input; the NaN sits in exactly the windows that contain its pixel, in its channel."""
    c = pc.POOL_CASE[name]
    d = pc.pool_data(c)
    ref = pc.pool_eval(c, d)["out"]
    win, hit = pc.pool_windows(c, d)
    assert pc.pool_equal(ref, win) and int(torch.isnan(ref).sum()) == hit and (ref[~torch.isnan(ref)] < 0).all()
    assert torch.isinf(d["x"]).any() and (d["x"][~torch.isnan(d["x"])] < 0).all()
    for mut in c.muts.split():
        assert not pc.pool_equal(ref, pc.pool_eval(c, d, mut=mut)["out"]), (name, mut)
    cs = pc.POOL_CASES
    assert {(c_.k, c_.stride, c_.pad) for c_ in cs} == {(3, 2, 1), (2, 2, 0)} and {c_.C for c_ in cs} == {4, 64} and all(c_.H % 2 and c_.W % 2 for c_ in cs)
    assert any(pc.pool_windows(c_, pc.pool_data(c_))[1] == 0 for c_ in cs) and any(pc.pool_windows(c_, pc.pool_data(c_))[1] > 1 for c_ in cs)


def test_transpose_restatement_and_wrong_reading():
    for n in pc.TR_N:
        for C, P in pc.TR_SHAPES:
            x = pc.tr_data(n, C, P)
            y = pc.tr_eval(x)
            assert y.shape == (n, P, C) and all(y[i, p, ch] == x[i, ch, p] for i in range(n) for p in (0, P // 2, P - 1) for ch in (0, C - 1))
            assert torch.equal(pc.tr_eval(y), x)
            if n > 1:
                assert not torch.equal(pc.tr_eval(x, mut="no_batch_stride"), y)


# ---- refusals: argument checks run before any launch, the pointers are never dereferenced
def test_refusals(L):
    f = ctypes.c_void_p(0x1000)
    for what, rc, code in pc.gru_refusal_calls(L, f, f):
        assert rc == code, (what, rc, L.forge_last_error())
    for what, rc, code in pc.other_refusal_calls(L, f, f):
        assert rc == code, (what, rc, L.forge_last_error())
