"""GPU (-m gpu): the F(4, 3) depth nest with F(4, 3) along H - forge_wino_input_dn4h / forge_wino_weights_dn4h / forge_wino_gemm_dn4h /
forge_wino_output_dn4h - against its restatement (tests/wino_dn4h_cases.py), through raw ctypes calls into canary-patterned buffers with guard rows, in
the shape of test_gpu_wino_depth_nest4.py.

Shapes (Ht Wt = 64: exactly one 64-row tile per plane):
  1 x D 8 x H 16 x W 32, C 32 | 32 -> 32, gates      the smallest: every H tile row is an edge or its neighbour, both depth groups touch an edge
  1 x D 8 x H 32 x W 16, C 64 -> 128, state          interior H tile rows, one full column tile
  1 x D 12 x H 16 x W 32, C 32 | 32 -> 32, state     an interior depth group
  2 x D 8 x H 16 x W 32, C 32 | 32 -> 160, gates     groups never straddle elements, non-zero batch stride, a partial column tile
V1 is fed as view 1 of a [n][3] stack of forge_wino_input_dn4h outputs whose other views are NaN. Per case:
  transform      forge_wino_input_dn4h: torch.equal with the float32 restatement (depth lines, the same lines over the patch rows, F(2, 3) columns)
  weights        forge_wino_weights_dn4h: torch.equal with the float64 evaluation in the documented order, rounded once
  point products |got - ref| <= gamma_(2 Cin + 2) sum |operand||weight| on the float32 operands the launch got (wino_dn4_cases.k_point)
  chain          input -> gemm -> forge_wino_output_dn4h (the case's GRU tail) against float64: q = max |got - ref| / (u sigma) and q_rms of every output
                 within SHARP = 4x the float32 CPU evaluation of THIS algorithm (wino_dn4h_cases.chain_dn4h in float32)
  ratio          q against the F(4, 3) nest's chain (forge_wino_input_dn4 -> forge_wino_gemm_dn4 -> forge_wino_output) on the same inputs: printed
  repeat         every launch once more on fresh canaries, bitwise
test_bounds_reject_wrong_references: one point, one depth position, one patch row dropped.
test_input_of_a_view_mean: nsum = 2 on 1 x 8 x 8 x 4 x 4, torch.equal with the float32 restatement.
test_refusals: H % 4 != 0, Ht Wt % 64 != 0, D % 4 != 0, D < 8, an operand of 2 GiB or more -> an error code, no launch.
test_fuse_hip_*: ConvGRU_3D.fuse_hip on 2 scenes x 3 views x 8 x 16 x 32 x 32 channels against the oracle GRU in float64, launch counts by entry; switched
off (STATE.wino_h4) the F(4, 3) nest's launches and bits.
"""
import ctypes

import pytest
import torch

import conv_igemm_cases as cc
import convgru_cases as gc
import wino_cases as wc
import wino_dn4_cases as d4
import wino_dn4h_cases as dh
from wino_gpu_util import EINVAL, F32, NAN, OutBuf, P, emitter, padded, twice
from forge_amd import _lib, convops as co, flopmeter, synthetic as syn
from forge_amd.fusion import ConvGRU_3D

pytestmark = pytest.mark.gpu

CASES = [
    wc.mk("dn4h_n1_d8_h16_w32_o32", "", 1, 8, 16, 32, 32, 32, C2=32, epi=2, out3=True),
    wc.mk("dn4h_n1_d8_h32_w16_o128", "", 1, 8, 32, 16, 64, 128, epi=3, out2=True, out3=True),
    wc.mk("dn4h_n1_d12_h16_w32_o32", "", 1, 12, 16, 32, 32, 32, C2=32, epi=3),
    wc.mk("dn4h_n2_d8_h16_w32_o160", "", 2, 8, 16, 32, 32, 160, C2=32, epi=2, out3=True),
]
CASE = {c.name: c for c in CASES}
VIEWS, VIEW = 3, 1
_CHAIN = {}

# The bound of test_fuse_hip_against_the_oracle, relative to max |reference|. Measured on the MI355X on this test's shape (2 scenes x 3 views x 8 x 16 x 32 x 32
# channels): 9.40e-6 with the 24-point form, 2.52e-6 with the F(4, 3) nest on the same inputs (3.7x; the CPU estimate of the chain said 4-5x). The bound is the
# measurement times the 4.5x margin that test_gpu_convgru_matrix.py's FWD = 1e-5 has over its measured 2.2e-6: 4.2e-5.
FWD_H4_MEASURED = 9.4e-6
FWD_H4 = 4.5 * FWD_H4_MEASURED


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


emit = emitter("wino_dn4h_matrix")


def _tail_buffers(c, d, dev):
    """(operands of the tail on the device, the output buffers by name)."""
    M = c.n * c.D * c.H * c.W
    ops = {k: (None if d.get(k) is None else padded(d[k], dev)) for k in ("bias", "scale", "shift", "aux_h", "aux_z")}
    width = c.Cout // 2 if c.epi == 2 else c.Cout
    outs = {k: OutBuf(dev, 1, M, width) for k in wc.out_names(c)}
    return ops, outs


def run_chain(c, dev):
    """Every launch of the case (module docstring); returns what the tests read. Computed once per case."""
    if c.name in _CHAIN:
        return _CHAIN[c.name]
    L, st = _lib.lib(), _lib.current_stream
    d = wc.make_data(c)
    n, D, H, W, C1, C2, Cout = c.n, c.D, c.H, c.W, c.C1, c.C2, c.Cout
    Ht, Wt, Cin = H // 4, W // 2, C1 + C2
    R = n * D * Ht * Wt                                         # tile rows of the 4 x 2 grid
    vol6, R6 = D // 4 * 6 * Ht * Wt, R // 4 * 6                # operand rows per element / in all
    grid = dh.grid_of(c)
    # ---- forge_wino_input_dn4h of both operands: bitwise the float32 restatement
    V = {}
    for key, C in (("x1", C1), ("x2", C2)):
        if C == 0:
            continue
        x = padded(d[key], dev)
        vb = OutBuf(dev, 24, R6, C)
        got = twice(lambda: _lib.check(L.forge_wino_input_dn4h(P(x), C, 0, vb.ptr(), C, 0, n, D, H, W, C, 1, 0, st()), "forge_wino_input_dn4h"), vb, (c.name, key))
        assert torch.equal(got, dh.input_transform_dn4h(d[key], 1, F32)), (c.name, "input_dn4h", key)
        V[key] = got

    def stacked(v, rows, points):                              # V1 as view VIEW of a [n][VIEWS] stack, the other views' rows NaN
        s = torch.full((points, n, VIEWS, rows, C1), NAN)
        s[:, :, VIEW] = v.reshape(points, n, rows, C1)
        return padded(s, dev)
    v1 = stacked(V["x1"], vol6, 24)
    p1 = ctypes.c_void_p(v1.data_ptr() + 4 * VIEW * vol6 * C1)
    v2 = padded(V["x2"], dev) if C2 else None
    Vcat = V["x1"] if not C2 else torch.cat([V["x1"], V["x2"]], dim=-1)
    # ---- forge_wino_weights_dn4h
    wp = padded(d["wp"], dev)
    ub = OutBuf(dev, 24, 6 * Cout, Cin)
    Ud = twice(lambda: _lib.check(L.forge_wino_weights_dn4h(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn4h"), ub, (c.name, "weights_dn4h"))
    Ud = Ud.reshape(24, 6, Cout, Cin)
    assert torch.equal(Ud, dh.weights_dn4h(d["wp"], F32)), (c.name, "U is not the float64 evaluation rounded once")
    _lib.check(L.forge_wino_weights_dn4h(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn4h")
    # ---- forge_wino_gemm_dn4h
    mb = OutBuf(dev, 24, R, Cout)
    args = (p1, C1, C1, VIEWS * vol6, n * VIEWS * vol6 * C1, P(v2), C2, C2, 0, 0, ub.ptr(), mb.ptr(), n, D, Ht, Wt, Cout, 3, st())
    Mm = twice(lambda: _lib.check(L.forge_wino_gemm_dn4h(*args), "forge_wino_gemm_dn4h"), mb, (c.name, "gemm_dn4h"))
    ref, mg = dh.nest_gemm(Vcat, Ud, grid), dh.nest_gemm(Vcat, Ud, grid, mag=True)
    r = ((Mm.double() - ref).abs() / (wc.gamma(d4.k_point(Cin)) * mg).clamp_min(1e-300)).max().item()
    q, qr = wc.q_of(Mm, ref, mg)
    emit("%-26s gemm_dn4h K 6x%-3d R %4d  q %5.2f q_rms %5.3f uncond %.2e" % (c.name, Cin, R, q, qr, r))
    assert r <= 1, (c.name, "point products: unconditional bound exceeded %.3g times" % r)
    # ---- forge_wino_output_dn4h with the case's GRU tail
    ops, outs = _tail_buffers(c, d, dev)
    ldo = Cout // 2 if c.epi == 2 else Cout
    optr = lambda k: outs[k].ptr() if k in outs else None
    _lib.check(L.forge_wino_gemm_dn4h(*args), "forge_wino_gemm_dn4h")

    def inverse():
        _lib.check(L.forge_wino_output_dn4h(mb.ptr(), P(ops["bias"]), P(ops["scale"]), P(ops["shift"]), P(ops["aux_h"]), P(ops["aux_z"]), optr("out"),
                                            optr("out2"), optr("out3"), n, D, H, W, Cout, ldo, c.epi, st()), "forge_wino_output_dn4h")
    got = {}
    for _ in range(2):
        for b in outs.values():
            b.t.fill_(cc.CANARY)
        inverse()
        now = {k: b.fetch((c.name, "output_dn4h", k))[0] for k, b in outs.items()}
        assert all(torch.equal(now[k].view(torch.int32), got.get(k, now[k]).view(torch.int32)) for k in now), (c.name, "two runs of the inverse differ")
        got = now
    # ---- the F(4, 3) nest's chain on the same inputs: forge_wino_input_dn4 -> forge_wino_gemm_dn4 -> forge_wino_output with the same tail
    Ht2 = H // 2
    vol62 = D // 4 * 6 * Ht2 * Wt
    V4, xs = {}, {}
    for key, C in (("x1", C1), ("x2", C2)):
        if C:
            vb, xs[key] = OutBuf(dev, 16, n * vol62, C), padded(d[key], dev)
            _lib.check(L.forge_wino_input_dn4(P(xs[key]), C, 0, vb.ptr(), C, 0, n, D, H, W, C, 1, 0, st()), "forge_wino_input_dn4")
            V4[key] = vb
    U4 = padded(d4.weights_dn4(d["wp"], F32), dev)
    m4 = OutBuf(dev, 16, n * D * Ht2 * Wt, Cout)
    _lib.check(L.forge_wino_gemm_dn4(V4["x1"].ptr(), C1, C1, 0, 0, V4["x2"].ptr() if C2 else None, C2, C2, 0, 0, P(U4), m4.ptr(), n, D, Ht2, Wt, Cout, 3, st()),
               "forge_wino_gemm_dn4")
    for b in outs.values():
        b.t.fill_(cc.CANARY)
    _lib.check(L.forge_wino_output(m4.ptr(), None, 0, 0, P(ops["bias"]), P(ops["scale"]), P(ops["shift"]), 1.0, None, P(ops["aux_h"]), P(ops["aux_z"]),
                                   optr("out"), optr("out2"), optr("out3"), n, D, H, W, Cout, ldo, c.epi, st()), "forge_wino_output")
    got4 = {k: b.fetch((c.name, "output of dn4", k))[0] for k, b in outs.items()}
    _CHAIN[c.name] = dict(d=d, out=got, out4=got4)
    return _CHAIN[c.name]


def yardstick(c, d):
    """(float64 reference outputs, sigma by output, {output: (q, q_rms)} of the float32 CPU evaluation of the 24-point chain in the kernels' order)."""
    ref, sS, sA = dh.chain_dn4h(c, d, want_sigma=True)
    sig = {k: sS[k] + sA[k] for k in ref}
    cpu = dh.chain_dn4h(c, d, F32)[0]
    return ref, sig, {k: wc.q_of(cpu[k], ref[k], sig[k]) for k in ref}


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_dn4h_against_float64(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    for k in ref:
        (q, qr), (q4, qr4) = wc.q_of(ch["out"][k], ref[k], sig[k]), wc.q_of(ch["out4"][k], ref[k], sig[k])
        emit("%-26s chain %-4s q %6.2f q_rms %5.3f | F(4,3) nest q %6.2f q_rms %5.3f | ratio to it %4.2f %4.2f | yard %6.2f %5.3f" % (
            name, k, q, qr, q4, qr4, q / q4, qr / qr4, yard[k][0], yard[k][1]))
        assert q <= wc.SHARP * yard[k][0] and qr <= wc.SHARP * yard[k][1], (name, k, q, qr, yard[k])


@pytest.mark.parametrize("name", ["dn4h_n1_d8_h16_w32_o32", "dn4h_n2_d8_h16_w32_o160"])
def test_bounds_reject_wrong_references(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    for mut in dh.MUTATIONS:
        wrong = dh.chain_dn4h(c, ch["d"], mut=mut)[0]
        ratio = max(max(a / b for a, b in zip(wc.q_of(ch["out"][k], wrong[k], sig[k]), yard[k])) for k in ref)
        emit("%-26s wrong reference %-14s q / yardstick %.3g" % (name, mut, ratio))
        assert ratio > wc.SHARP, (name, mut, ratio)


def test_input_of_a_view_mean(dev):
    """forge_wino_input_dn4h with nsum > 1 (the argument path the input entries share): the mean of two views sum_stride rows apart, then the three stages,
    torch.equal with the float32 restatement. n = 1, D = 8 (two groups), H = 8 (two tile rows), W = 4, C = 4."""
    L, st = _lib.lib(), _lib.current_stream
    n, D, H, W, C, nsum = 1, 8, 8, 4, 4, 2
    x = torch.randn(nsum, n, D, H, W, C, generator=torch.Generator().manual_seed(21))
    xd = padded(x, dev)
    vb = OutBuf(dev, 24, n * (D // 4) * 6 * (H // 4) * (W // 2), C)
    got = twice(lambda: _lib.check(L.forge_wino_input_dn4h(P(xd), C, 0, vb.ptr(), C, 0, n, D, H, W, C, nsum, n * D * H * W, st()), "forge_wino_input_dn4h"),
                vb, "input_dn4h of a view mean")
    assert torch.equal(got, dh.input_transform_dn4h(x, nsum, F32))


def test_refusals(dev):
    """Illegal calls return an error code before any launch; the buffers are large enough for the nearest accepted call."""
    L, st = _lib.lib(), _lib.current_stream
    buf = lambda nfl: torch.zeros(nfl, dtype=F32, device=dev)
    X, V, U, Mm = buf(8 * 16 * 32 * 32), buf(24 * 768 * 64), buf(24 * 6 * 32 * 64), buf(24 * 512 * 32)
    h = buf(8 * 16 * 32 * 32)

    def gemm(D, Ht, Wt, C1=32, C2=0, n=1, Cout=32):
        return L.forge_wino_gemm_dn4h(P(V), C1, C1, 0, 0, P(V) if C2 else None, C2, C2, 0, 0, P(U), P(Mm), n, D, Ht, Wt, Cout, 3, st())

    def inp(D, H, W):
        return L.forge_wino_input_dn4h(P(X), 32, 0, P(V), 32, 0, 1, D, H, W, 32, 1, 0, st())

    def outp(H, W):
        return L.forge_wino_output_dn4h(P(Mm), None, None, None, P(h), P(h), P(X), None, None, 1, 8, H, W, 32, 32, co.EPI_GRU_OUT, st())
    torch.cuda.synchronize()
    assert inp(8, 14, 32) != 0 and b"multiple of 4" in L.forge_last_error()      # H % 4 != 0
    assert outp(14, 32) != 0
    assert inp(6, 16, 32) != 0 and inp(4, 16, 32) != 0                            # D % 4 != 0, D < 8
    assert gemm(8, 4, 8) == EINVAL and b"Ht Wt" in L.forge_last_error()           # Ht Wt = 32
    assert gemm(6, 4, 16) == EINVAL and b"D % 4" in L.forge_last_error()
    assert gemm(4, 4, 16) == EINVAL and b"at least 8" in L.forge_last_error()
    assert gemm(8, 4, 16, C1=16) == EINVAL
    assert gemm(8, 64, 64, n=64, C1=256) == EINVAL                                # an operand of 3 GiB
    assert gemm(8, 8, 8, n=4096, Cout=256) == EINVAL                              # an output plane of 2 GiB
    torch.cuda.synchronize()
    assert int(Mm.abs().sum().item()) == 0 and int(V.abs().sum().item()) == 0 and int(X.abs().sum().item()) == 0       # nothing was launched
    assert gemm(8, 4, 16) == 0 and gemm(8, 4, 16, C1=32, C2=32) == 0 and inp(8, 16, 32) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the fusion
def _fuse(dev, monkeypatch, h4):
    """ConvGRU_3D.fuse_hip on 2 scenes x 3 views x 8 x 16 x 32 x 32 channels. At 32 channels forge_wino_gemm would not take its 64 x 128 tile, so the rule's tile
    condition is lifted for the test (the entries' own preconditions stay), as the other nest tests do."""
    case = gc.Case("dn4h", 32, 2, 8, 16, 32, (tuple(range(3)),), False, None)
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=case.C, hidden_size=case.C)
    w = syn.seeded_state_dict(gru.state_dict(), 9)
    x = torch.randn(case.b, 3, case.C, case.D, case.H, case.W, generator=torch.Generator().manual_seed(14)) * 0.5
    gru.load_state_dict(w)
    gru = gru.to(dev).eval()
    monkeypatch.setattr(co.STATE, "wino_depth_nest", True)
    monkeypatch.setattr(co.STATE, "wino_depth_nest4", True)
    monkeypatch.setattr(co.STATE, "wino_h4", h4)
    monkeypatch.setattr(co, "wino_gemm_tile", lambda R, Cout, Cin: "B")
    with torch.no_grad(), flopmeter.FlopMeter() as m:
        y = gru.fuse_hip(x.to(dev))
        torch.cuda.synchronize()
    return x, w, y, m.launches


def test_fuse_hip_against_the_oracle(dev, monkeypatch):
    x, w, y, launches = _fuse(dev, monkeypatch, True)
    # gates + state of three views on the 24 points; fusion_conv's two launches stay on the F(2, 3) nest
    assert launches["forge_wino_gemm_dn4h"] == 6 and launches["forge_wino_gemm_dn"] == 2, launches
    assert launches["forge_wino_gemm_dn4"] + launches["forge_wino_gemm_half"] + launches["forge_wino_gemm"] == 0, launches
    with torch.no_grad():
        ref = gc.ref_fuse(x.double(), {k: v.double() for k, v in w.items()}, False)
    err = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    _, _, y4, _ = _fuse(dev, monkeypatch, False)
    err4 = (y4.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    emit("fuse_hip 2 x 3 x 8x16x32x32 24-point form: max error / max |ref| %.2e (bound %.2e) | F(4, 3) nest %.2e" % (err, FWD_H4, err4))
    assert err < FWD_H4, err


def test_fuse_hip_switched_off_makes_the_launches_of_before(dev, monkeypatch):
    _, _, y_on, _ = _fuse(dev, monkeypatch, True)
    _, _, y_off, launches = _fuse(dev, monkeypatch, False)
    assert launches["forge_wino_gemm_dn4h"] == 0 and launches["forge_wino_gemm_dn4"] == 6 and launches["forge_wino_gemm_dn"] == 2, launches
    _, _, y_again, _ = _fuse(dev, monkeypatch, False)
    assert torch.equal(y_off, y_again)
    assert not torch.equal(y_on, y_off)                        # another rounding order: the switch does select another path
