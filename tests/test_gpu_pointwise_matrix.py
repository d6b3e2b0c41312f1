"""GPU (-m gpu): the pointwise training kernels and the data movers - the GRU halves, affine_act_bwd, the grouped sums of squares, adam_small, im2col,
max-pool, the two transposes - against the restatements of tests/pointwise_cases.py, through the C entry points (the sums also through
train.grouped_mse).

Every output lives inside an allocation filled with a NaN of a known bit pattern. Afterwards the floats before and past the buffer and every element
the contract does not name (gap columns of strided rows, accumulator rows between the batches, the other channels of a wider tensor) still hold the
pattern, and the named ones are inside the bound: SHARP x the float32 CPU yardstick with the EPI_ULPS floor for the arithmetic kernels, bitwise for
the data movers and the two-product kernels (pointwise_cases' docstring). Strided inputs carry NaN in their gap columns.
Every line "pointwise_matrix ..." printed under -s is a row of MEASURED in pointwise_cases.py.
"""
import pytest
import torch

import pointwise_cases as pc
from forge_amd import _lib, train
from pointwise_cases import GUARD, finish, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


_REF = {}


def cached(key, fn):
    """References and yardsticks are computed once and left unchanged."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def yard(fn):
    with pc.yardstick_threads():
        return fn()


def out_buf(shape, dev, fill=None):
    """A pattern-filled guarded buffer; fill: a host tensor in buffer layout whose numbers are written, its NaNs leave the pattern."""
    raw, body = guarded(tuple(shape), dev)
    if fill is not None:
        keep = ~torch.isnan(fill)
        body[keep.to(dev)] = fill[keep].float().to(dev)
    return raw, body


def read(raw, body, what, nan_ok=False):
    """The buffer on the host, in buffer layout. The guards hold the pattern, and so does every NaN inside (nan_ok: a result may be a NaN of its own)."""
    torch.cuda.synchronize()
    host = raw.cpu()
    n = body.numel()
    guard = torch.cat([host[:GUARD], host[GUARD + n:]])
    assert (guard == pc.CANARY).all(), (what, "an element outside the buffer was written", int((guard != pc.CANARY).sum()))
    bits = host[GUARD:GUARD + n]
    got = bits.view(torch.float32).view(body.shape).clone()
    if not nan_ok:
        assert (bits[torch.isnan(got).view(-1)] == pc.CANARY).all(), (what, "a NaN that is not the pattern")
    return got


def line(what, figs):
    """One printed row: per buffer the error, its bound and its ratio to the yardstick's error."""
    print("pointwise_matrix %-12s %s" % (what, " | ".join("%s %.2e (bound %.2e, %.2fx)" % (k, e, b, e / ey if ey else 0.0) for k, (e, b, ey) in figs.items())))


# ---- the GRU halves
@pytest.mark.parametrize("name", [c.name for c in pc.GRU_CASES])
def test_gru(dev, name):
    c = pc.GRU_CASE[name]
    d, ref, yd = cached(name, lambda: (lambda d: (d, pc.gru_eval(c, d), yard(lambda: pc.gru_eval(c, d, torch.float32))))(pc.gru_data(c)))
    L, st, p = _lib.lib(), _lib.current_stream(), _lib.ptr
    M, C = c.M, c.C
    up = lambda k: d[k].to(dev)
    g, h, z, r, cand = up("g"), up("h"), up("z"), up("r"), up("cand")
    bufs = {}
    # gates forward
    for k in ("z", "r", "hr"):
        bufs[k] = out_buf((M, C), dev)
    _lib.check(L.forge_gru_gates_fwd(p(g), p(h), p(bufs["z"][1]), p(bufs["r"][1]), p(bufs["hr"][1]), M, C, st), "forge_gru_gates_fwd")
    # state forward: tanh(c) overwrites the pre-activation
    bufs["cand"], bufs["hn"] = out_buf((M, C), dev, fill=d["c"]), out_buf((M, C), dev)
    _lib.check(L.forge_gru_state_fwd(p(bufs["cand"][1]), p(h), p(z), p(bufs["hn"][1]), M, C, st), "forge_gru_state_fwd")
    # state backward
    accp = lambda key, prior: out_buf(ref[key].shape, dev, fill=torch.where(torch.isnan(ref[key]), pc.NAN, prior.double()) if c.acc_mode == 2 else None)
    dhn = pc.strided(d["dhn"], c.ld_dhn).to(dev)
    for k in ("s_dh", "s_dz", "s_dc"):
        bufs[k] = out_buf((M, C), dev)
    if c.acc_mode:
        bufs["s_acc"] = accp("s_acc", d["prior_c"])
    _lib.check(L.forge_gru_state_bwd(p(dhn), c.ld_dhn, p(h), p(z), p(cand), p(bufs["s_dh"][1]), p(bufs["s_dz"][1]), p(bufs["s_dc"][1]), M, C,
                                     p(bufs["s_acc"][1]) if c.acc_mode else None, 3 * c.vol, c.vol, c.acc_mode, st), "forge_gru_state_bwd")
    # gates backward
    dz = up("dz_in")
    bufs["g_dg"] = out_buf((M, 2 * C), dev)
    dh = out_buf((M, C), dev, fill=d["dh_in"])
    if c.dh_out == "alias":
        bufs["g_dh_out"] = out_buf((M, c.ld_dhr), dev, fill=pc.strided(d["dhr"], c.ld_dhr))
        dhr, dh_out, ld_out = bufs["g_dh_out"][1], bufs["g_dh_out"][1], c.ld_dhr
    else:
        dhr = pc.strided(d["dhr"], c.ld_dhr).to(dev)
        if c.dh_out is None:
            bufs["g_dh"], dh_out, ld_out = dh, None, 0
        else:
            bufs["g_dh_out"] = out_buf((M, c.dh_out), dev)
            dh_out, ld_out = bufs["g_dh_out"][1], c.dh_out
    if c.acc_mode:
        bufs["g_acc"] = accp("g_acc", d["prior_g"])
    _lib.check(L.forge_gru_gates_bwd(p(dz), p(dhr), c.ld_dhr, p(h), p(z), p(r), p(bufs["g_dg"][1]), p(dh[1]), p(dh_out), ld_out, M, C,
                                     p(bufs["g_acc"][1]) if c.acc_mode else None, 3 * c.vol, c.vol, c.acc_mode, st), "forge_gru_gates_bwd")
    got = {k: read(raw, body, (name, k)) for k, (raw, body) in bufs.items()}
    if c.dh_out is not None:
        assert torch.equal(read(*dh, (name, "dh")), d["dh_in"]), (name, "dh was written although dh_out was given")
    assert set(got) == set(ref)
    for k in ("z", "r"):
        assert (got[k] >= 0).all() and (got[k] <= 1).all(), (name, k, "a gate outside [0, 1]")
    assert (got["cand"].abs() <= 1).all(), (name, "tanh outside [-1, 1]")
    figs, fails = pc.compare_all(got, ref, yd)
    line(name, figs)
    assert not fails, (name, fails)


# ---- affine_act_bwd: bitwise
@pytest.mark.parametrize("name", [c.name for c in pc.AFF_CASES])
def test_affine_act_bwd(dev, name):
    c = pc.AFF_CASE[name]
    d = cached(name, lambda: pc.aff_data(c))
    ref = pc.aff_eval(c, d)
    L, st, p = _lib.lib(), _lib.current_stream(), _lib.ptr
    y = pc.strided(d["y"], c.ld_y).to(dev)
    scale = None if d["scale"] is None else d["scale"].to(dev)
    if c.inplace:
        assert c.ld_dx == c.ld_dy
        raw, dx = out_buf((c.M, c.ld_dx), dev, fill=pc.strided(d["dy"], c.ld_dy))
        dy = dx
    else:
        raw, dx = out_buf((c.M, c.ld_dx), dev)
        dy = pc.strided(d["dy"], c.ld_dy).to(dev)
    _lib.check(L.forge_affine_act_bwd(p(dy), c.ld_dy, p(y), c.ld_y, p(scale), c.slope, p(dx), c.ld_dx, c.M, c.C, st), "forge_affine_act_bwd")
    figs, fails = pc.compare_all({"dx": read(raw, dx, name)}, ref)
    print("pointwise_matrix %-12s affine_act_bwd bitwise: %d elements differ" % (name, figs["dx"][0]))
    assert not fails, (name, fails)


# ---- the grouped sums of squares
@pytest.mark.parametrize("name", [c.name for c in pc.SSE_CASES])
def test_sse_groups(dev, name):
    c = pc.SSE_CASE[name]
    d, ref, yd = cached(name, lambda: (lambda d: (d, pc.sse_eval(c, d), yard(lambda: pc.sse_eval(c, d, torch.float32))))(pc.sse_data(c)))
    L, st, p = _lib.lib(), _lib.current_stream(), _lib.ptr
    G = c.Vp // c.gsize
    base, target, coef = d["base"].to(dev), d["target"].to(dev), d["coef"].to(dev)
    bnd = pc.sse_bound(ref["sums"], yd["sums"])
    rel = lambda s: ((s.double().cpu() - ref["sums"]).abs() / ref["sums"]).max().item()
    msg = ""
    if c.layout != "batch_gap":
        pred = pc.sse_view(c, base)
        strides = pred.stride()[1:]
        dims = (c.B, c.Vp, c.Vt, c.gsize, c.C, c.H, c.W, st)
        nb = L.forge_sse_groups_blocks()
        assert nb == 1024
        raw, partial = guarded((nb, G), dev)
        _lib.check(L.forge_sse_groups_fwd(p(pred), *strides, p(target), p(partial), *dims), "forge_sse_groups_fwd")
        e_c = rel(finish(raw, partial, (name, "partial")).double().sum(0))             # every one of the 1024 G entries is written
        raw, dbase = guarded(tuple(base.shape), dev)
        _lib.check(L.forge_sse_groups_bwd(p(pred), *strides, p(target), p(coef), p(pc.sse_view(c, dbase)), *dims), "forge_sse_groups_bwd")
        _, fails = pc.compare_all({"dpred": read(raw, dbase, (name, "dpred"))}, {"dpred": yd["dpred"]})
        msg = "C entry: sums rel %.2e, dpred bitwise %s; " % (e_c, "yes" if not fails else "NO")
        assert e_c <= bnd, (name, "sums", e_c, bnd)
        assert not fails, (name, fails)
    # through train.grouped_mse: the means, and the gradient of their coef-weighted sum in pred's layout (zeros where pred does not live)
    leaf = base.clone().requires_grad_(True)
    mse = train.grouped_mse(pc.sse_view(c, leaf), target, c.gsize)
    (mse * coef).sum().backward()
    torch.cuda.synchronize()
    per = c.B * c.gsize * c.C * c.H * c.W
    e_m = rel(mse.detach() * per)
    w = dict(d, coef=d["coef"] * 2 / per)
    gref = pc.sse_eval(c, dict(d, coef=w["coef"].double()))["dpred"]
    gy = yard(lambda: pc.sse_eval(c, w, torch.float32))["dpred"]
    grad = leaf.grad.cpu()
    assert (grad[torch.isnan(gref)] == 0).all(), (name, "a gradient outside pred")
    e, b, ey, fails = pc.compare(torch.where(torch.isnan(gref), pc.NAN, grad.double()).float(), gref, gy, floor=False)
    print("pointwise_matrix %-12s sse_groups %sgrouped_mse: sums rel %.2e (bound %.2e, yardstick %.2e), gradient %.2e (bound %.2e)" % (
        name, msg, e_m, bnd, ((yd["sums"].double() - ref["sums"]).abs() / ref["sums"]).max().item(), e, b))
    assert e_m <= bnd, (name, "grouped_mse", e_m, bnd)
    assert not fails, (name, fails)


# ---- adam_small
@pytest.mark.parametrize("n", pc.ADAM_N)
def test_adam_small(dev, n):
    d, ref, yd = cached("adam%d" % n, lambda: (lambda d: (d, pc.adam_eval(d), yard(lambda: pc.adam_eval(d, torch.float32))))(pc.adam_data(n)))
    L, st, p = _lib.lib(), _lib.current_stream(), _lib.ptr
    bufs = {k: out_buf((n,), dev, fill=d[k]) for k in ("p", "m", "v")}
    raw_s, step = out_buf((1,), dev, fill=torch.tensor([pc.ADAM_STEP0]))
    hy = pc.ADAM_HYPER
    for i, g in enumerate(d["grads"]):
        gd = g.to(dev)
        _lib.check(L.forge_adam_small(p(bufs["p"][1]), p(gd), p(bufs["m"][1]), p(bufs["v"][1]), p(step), n, hy["lr"], hy["b1"], hy["b2"], hy["eps"], st), "forge_adam_small")
        assert read(raw_s, step, "step").item() == pc.ADAM_STEP0 + i + 1, "the step counter advances by exactly 1 per launch"
    figs, fails = pc.compare_all({k: read(raw, body, ("adam", n, k)) for k, (raw, body) in bufs.items()}, ref, yd, floor=False)
    line("adam n=%d" % n, figs)
    assert not fails, (n, fails)


# ---- the data movers: bitwise
@pytest.mark.parametrize("name", [c.name for c in pc.COL_CASES])
def test_im2col(dev, name):
    c = pc.COL_CASE[name]
    d = cached(name, lambda: pc.col_data(c))
    ref = pc.col_eval(c, d)["out"]
    raw, out = guarded(tuple(ref.shape), dev)
    img = d["img"].to(dev)
    _lib.check(_lib.lib().forge_im2col_nchw(_lib.ptr(img), _lib.ptr(out), c.N, c.C, c.H, c.W, c.k, c.k, c.stride, c.pad, c.Kpad, _lib.current_stream()), "forge_im2col_nchw")
    got = finish(raw, out, name)
    print("pointwise_matrix %-12s im2col bitwise: %d elements differ" % (name, int((got.view(torch.int32) != ref.view(torch.int32)).sum())))
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), name


@pytest.mark.parametrize("name", [c.name for c in pc.POOL_CASES])
def test_maxpool(dev, name):
    c = pc.POOL_CASE[name]
    d = cached(name, lambda: pc.pool_data(c))
    ref = pc.pool_eval(c, d)["out"]
    raw, out = guarded(tuple(ref.shape), dev)
    x = d["x"].to(dev)
    _lib.check(_lib.lib().forge_maxpool2d_nhwc(_lib.ptr(x), _lib.ptr(out), c.N, c.H, c.W, c.C, c.k, c.stride, c.pad, _lib.current_stream()), "forge_maxpool2d_nhwc")
    got = read(raw, out, name, nan_ok=True)
    print("pointwise_matrix %-12s maxpool bitwise: %s; NaN windows %d of %d" % (name, pc.pool_equal(got, ref), int(torch.isnan(got).sum()), int(torch.isnan(ref).sum())))
    assert pc.pool_equal(got, ref), (name, "not F.max_pool2d bitwise, the NaN included")


@pytest.mark.parametrize("n", pc.TR_N)
@pytest.mark.parametrize("C,P", pc.TR_SHAPES)
def test_transposes(dev, n, C, P):
    L, st, p = _lib.lib(), _lib.current_stream(), _lib.ptr
    x = cached(("tr", n, C, P), lambda: pc.tr_data(n, C, P))
    y = pc.tr_eval(x)
    raw, cl = guarded((n, P, C), dev)
    xd = x.to(dev)
    _lib.check(L.forge_ncdhw_to_ndhwc(p(xd), p(cl), n, C, P, st), "forge_ncdhw_to_ndhwc")
    got = finish(raw, cl, ("to_ndhwc", n, C, P))
    assert torch.equal(got.view(torch.int32), y.view(torch.int32))
    raw2, back = guarded((n, C, P), dev)
    _lib.check(L.forge_ndhwc_to_ncdhw(p(cl), p(back), n, C, P, st), "forge_ndhwc_to_ncdhw")           # the round trip, from the kernel's own output
    assert torch.equal(finish(raw2, back, ("round trip", n, C, P)).view(torch.int32), x.view(torch.int32))
    raw3, cf = guarded((n, C, P), dev)
    yd = y.to(dev)
    _lib.check(L.forge_ndhwc_to_ncdhw(p(yd), p(cf), n, C, P, st), "forge_ndhwc_to_ncdhw")
    assert torch.equal(finish(raw3, cf, ("to_ncdhw", n, C, P)).view(torch.int32), x.view(torch.int32))
    print("pointwise_matrix tr n=%d C=%d P=%d: to_ndhwc, to_ncdhw and the round trip bitwise" % (n, C, P))


def test_refusals_leave_the_output_alone(dev):
    """Every refusal on real buffers: the error code, and not one float of the output touched. The size-only refusals return before they touch memory."""
    L = _lib.lib()
    nfl = (1 << 20) + 8                       # room for the largest launch a refusal that failed to fire would describe (adam_small's n = 2^20 + 1)
    src = torch.zeros(nfl, dtype=torch.float32, device=dev)
    raw, out = guarded((nfl,), dev)
    with torch.cuda.device(dev):
        for what, rc, code in pc.gru_refusal_calls(L, _lib.ptr(src), _lib.ptr(out)) + pc.other_refusal_calls(L, _lib.ptr(src), _lib.ptr(out)):
            assert rc == code, (what, rc, L.forge_last_error())
        torch.cuda.synchronize()
    assert (raw.cpu() == pc.CANARY).all(), "a refused call wrote to its output"
