"""GPU (-m gpu): the ray-marcher over its dispatch space - channel instantiation x camera gradients x tile height x workgroup placement x grid shape and
pitch x view lists x sample counts x ray intervals x densities - against the float64 restatement of its contract (tests/render_cases.py), through
forge_render_fwd / forge_render_bwd.

Per case:
  forward        with depth, into buffers filled with a NaN of a known bit pattern: every element written and finite, one element before and past each
                 buffer still the pattern; features, opacity and depth inside 2e-5 max(1, |ref|). Without depth (out_depth == NULL): bitwise the same
                 features and opacity.
  backward       without dcam: workspace, dfeat and ddens start as the pattern; G is fully written and exactly zero wherever a sample certainly lies
                 outside its ray's interval; dfeat and ddens inside 5e-5 of their maximum. With dcam: the same for the volume gradients, the per-workgroup
                 partials fully written, and - where the case clears the lattice (render_cases.Case.cam, asserted on the CPU) - each camera-entry group
                 inside SHARP x the float32 CPU yardstick (floor 64 u, cap 2e-3). Cases marked nodepth run once more with g_depth == NULL.
  exact zeros    a view whose frustum misses its volume (outputs, its dcam row, the volume's gradients), a volume no view reads, an all-zero density
                 (outputs and dfeat).
Every line "render_matrix ..." printed under -s is a row of the table in the pull request's description.
"""
import pytest
import torch

import render_cases as rc
from forge_amd import _lib
from rotate_cases import GUARD, finish, guarded, yardstick_threads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


_REF = {}


def reference(c):
    """(data, float64 reference, the float32 yardstick's dcam group errors, the reference without g_depth or None), computed once per case."""
    if c.name not in _REF:
        d = rc.make_data(c)
        r = rc.gradients(c, d)
        with yardstick_threads():
            yard = rc.group_errors(rc.gradients(c, d, torch.float32)["dcam"], r["dcam"]) if c.cam else None
        _REF[c.name] = (d, r, yard, rc.gradients(c, d, depth=False) if c.nodepth else None)
    return _REF[c.name]


def _err(got, ref):
    return (got.double() - ref).abs().max().item()


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_case(dev, name):
    c = rc.CASE[name]
    d, r, yard, r0 = reference(c)
    L = _lib.lib()
    V, C, Hr, Wr, S = len(c.cams), c.C, c.Hr, c.Wr, c.S
    t = {k: v.to(dev) for k, v in d.items()}
    st = _lib.current_stream()
    geo = (V, c.nvol, C, c.D, c.H, c.W, Hr, Wr, S, c.zmin, c.zmax, *c.half)
    ins = (_lib.ptr(t["feat"]), _lib.ptr(t["dens"]), _lib.ptr(t["cam"]), _lib.ptr(t["v2v"]))

    # ---- forward, with and without depth
    outs = {}
    for want_depth in (True, False):
        bufs = [guarded(s, dev) for s in ((V, Hr, Wr, C), (V, Hr, Wr)) + (((V, Hr, Wr),) if want_depth else ())]
        _lib.check(L.forge_render_fwd(*ins, _lib.ptr(bufs[0][1]), _lib.ptr(bufs[1][1]), _lib.ptr(bufs[2][1]) if want_depth else None, *geo, st), "forge_render_fwd")
        outs[want_depth] = [finish(raw, body, (name, "forward", want_depth, i)) for i, (raw, body) in enumerate(bufs)]
    of, oo, od = outs[True]
    assert torch.equal(of, outs[False][0]) and torch.equal(oo, outs[False][1]), (name, "the forward without depth differs")
    e_fwd = [_err(of, r["feat"]), _err(oo, r["opac"]), _err(od, r["depth"])]
    for e, k in zip(e_fwd, ("feat", "opac", "depth")):
        assert e <= rc.fwd_bound(r[k]), (name, "forward", k, e, rc.fwd_bound(r[k]))
    for v, kind in enumerate(c.cams):
        if kind == "miss":
            assert (of[v] == 0).all() and (oo[v] == 0).all() and (od[v] == 0).all(), (name, "a frustum that misses the volume does not render exact zeros")
    if c.dens == "zero":
        assert (of == 0).all() and (oo == 0).all() and (od == 0).all()

    # ---- backward
    outside = rc.certainly_outside(c, d)

    def backward(want_cam, depth=True):
        nbytes = L.forge_render_bwd_ws_bytes(V, C, Hr, Wr, S, want_cam)
        assert nbytes == rc.ws_bytes(c, want_cam)
        raw_ws, ws = guarded((nbytes // 4,), dev)
        raw_f, dfeat = guarded(tuple(d["feat"].shape), dev)
        raw_d, ddens = guarded(tuple(d["dens"].shape), dev)
        raw_c, dcam = guarded((V, 16), dev) if want_cam else (None, None)
        _lib.check(L.forge_render_bwd(*ins, _lib.ptr(t["g_feat"]), _lib.ptr(t["g_opac"]), _lib.ptr(t["g_depth"]) if depth else None, _lib.ptr(dfeat), _lib.ptr(ddens),
                                      _lib.ptr(dcam), *geo, _lib.ptr(ws), nbytes, st), "forge_render_bwd")
        what = (name, "backward", want_cam, depth)
        gf, gd = finish(raw_f, dfeat, what + ("dfeat",)), finish(raw_d, ddens, what + ("ddens",))
        gc = finish(raw_c, dcam, what + ("dcam",)) if want_cam else None
        torch.cuda.synchronize()
        host = raw_ws.cpu()
        written = ws.numel() if not want_cam else (nbytes - V * Hr * Wr * S * 24) // 4               # G and the per-workgroup partials; the per-sample scalars are written only inside a ray's interval
        assert (host[:GUARD] == rc.CANARY).all() and (host[GUARD + ws.numel():] == rc.CANARY).all(), what + ("an element outside the workspace was written",)
        body = host[GUARD:GUARD + ws.numel()].view(torch.float32)
        assert torch.isfinite(body[:written]).all(), what + ("G or a camera partial was not written",)
        Gv = body[:V * S * Hr * Wr * 2].view(V, S, Hr, Wr, 2)
        assert (Gv[outside] == 0).all(), what + ("G is not exactly zero outside a ray's sample interval",)
        return gf, gd, gc

    ref = {True: r, False: r0}
    runs = [(0, True), (1, True)] + ([(0, False)] if c.nodepth else [])
    e_grad, dcam = [], None
    for want_cam, depth in runs:
        gf, gd, gc = backward(want_cam, depth)
        rr = ref[depth]
        ef, ed = _err(gf, rr["dfeat"]), _err(gd, rr["ddens"])
        e_grad.append((ef / max(rr["dfeat"].abs().max().item(), 1e-300), ed / max(rr["ddens"].abs().max().item(), 1e-300)))
        assert ef <= rc.grad_bound(rr["dfeat"]), (name, "dfeat", want_cam, depth, ef, rc.grad_bound(rr["dfeat"]))
        assert ed <= rc.grad_bound(rr["ddens"]), (name, "ddens", want_cam, depth, ed, rc.grad_bound(rr["ddens"]))
        for n in range(c.nvol):
            if n not in c.v2v or all(c.cams[v] == "miss" for v in range(V) if c.v2v[v] == n):
                assert (gf[n] == 0).all() and (gd[n] == 0).all(), (name, "the gradients of a volume that no ray reaches are not exactly zero", n)
        if c.dens == "zero":
            assert (gf == 0).all()
        if want_cam:
            dcam = gc
    for v, kind in enumerate(c.cams):
        if kind == "miss":
            assert (dcam[v] == 0).all(), (name, "dcam of a frustum that misses the volume is not exactly zero")
    line = "render_matrix %-7s fwd %.1e %.1e %.1e (of 2e-5) dfeat %.1e ddens %.1e (of 5e-5)" % (name, *[e / max(1.0, r[k].abs().max().item()) for e, k in zip(e_fwd, ("feat", "opac", "depth"))],
                                                                                             max(e[0] for e in e_grad), max(e[1] for e in e_grad))
    if c.cam:
        eg, bound = rc.group_errors(dcam, r["dcam"]), rc.dcam_bounds(yard)
        ratio = max(x / max(y, rc.DCAM_FLOOR / rc.SHARP) for x, y in zip(eg, yard))
        print(line + " dcam R T f c: yardstick %s got %s; worst ratio to the yardstick %.2f" % (" ".join("%.1e" % y for y in yard), " ".join("%.1e" % x for x in eg), ratio))
        assert all(x <= b for x, b in zip(eg, bound)), (name, "dcam", eg, bound)
    else:
        print(line + " dcam not compared (samples on the lattice)")
