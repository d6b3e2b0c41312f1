"""GPU (-m gpu): the F(4, 3) depth nest with F(4, 3) along H and W - forge_wino_input_dn4hw / forge_wino_weights_dn4hw / forge_wino_gemm_dn4hw /
forge_wino_output_dn4hw - against its restatement (tests/wino_dn4hw_cases.py), through raw ctypes calls into canary-patterned buffers with guard rows, in
the shape of test_gpu_wino_dn4h.py.

Shapes (Ht Wt = 64: exactly one 64-row tile per plane, the point GEMM's minimum):
  1 x D 8 x H 32 x W 32, C 32 | 32 -> 32, gates, r stored       both depth groups touch an edge, interior tiles in H and W
  1 x D 12 x H 16 x W 64, C 64 -> 128, state, both extra outputs three groups (an interior one), a full column tile
  2 x D 8 x H 32 x W 32, C 32 | 32 -> 160, gates                groups never straddle elements, non-zero batch stride, a partial column tile
V1 is fed as view 1 of a [n][3] stack of forge_wino_input_dn4hw outputs whose other views are NaN. Per case:
  transform      forge_wino_input_dn4hw: torch.equal with the float32 restatement (the six lines over planes, patch rows, patch columns)
  weights        forge_wino_weights_dn4hw: torch.equal with the float64 evaluation in the documented order, rounded once
  point products |got - ref| <= gamma_(2 Cin + 2) sum |operand||weight| on the float32 operands the launch got (wino_dn4_cases.k_point)
  chain          input -> gemm -> forge_wino_output_dn4hw (the case's GRU tail) against float64: q = max |got - ref| / (u sigma) and q_rms of every output
                 within SHARP = 4x the float32 CPU evaluation of THIS algorithm (wino_dn4hw_cases.chain_dn4hw in float32)
  repeat         every launch once more on fresh canaries, bitwise
test_bounds_reject_wrong_references: a wrong column line, H and W points swapped, a wrong position order.
test_input_of_a_view_mean: nsum = 2 on 1 x 8 x 8 x 8 x 4, torch.equal with the float32 restatement.
test_refusals: W % 4, H % 4, D % 4, D = 4, Cin % 32, Ht Wt = 32, an operand of 3 GiB -> FORGE_EINVAL, no launch.
test_fuse_hip_*: ConvGRU_3D.fuse_hip against the oracle GRU in float64, launch counts by entry; switched off (STATE.wino_w4) the 24-point form's launches
and bits. Two shapes: 2 scenes x 3 views x 8 x 32 x 32 x 64 channels - its state launch has Cout = 64, for which forge_wino_gemm_tile answers the 64-column
tile 'C' and no nest's rule holds, so the rule's tile condition is lifted for it as in the other nest tests (the entries' own preconditions stay) - and
2 scenes x 3 views x 16 x 32 x 32 x 128 channels with NOTHING patched: fusion._fuse_eval's choice on the rules as they run in the product.
"""
import ctypes

import pytest
import torch

import conv_igemm_cases as cc
import convgru_cases as gc
import wino_cases as wc
import wino_dn4_cases as d4
import wino_dn4hw_cases as dw
from wino_gpu_util import EINVAL, F32, NAN, OutBuf, P, emitter, padded, twice
from forge_amd import _lib, convops as co, flopmeter, synthetic as syn
from forge_amd.fusion import ConvGRU_3D

pytestmark = pytest.mark.gpu

CASES = [
    wc.mk("dn4hw_n1_d8_h32_w32_o32", "", 1, 8, 32, 32, 32, 32, C2=32, epi=2, out3=True),
    wc.mk("dn4hw_n1_d12_h16_w64_o128", "", 1, 12, 16, 64, 64, 128, epi=3, out2=True, out3=True),
    wc.mk("dn4hw_n2_d8_h32_w32_o160", "", 2, 8, 32, 32, 32, 160, C2=32, epi=2, out3=True),
]
CASE = {c.name: c for c in CASES}
VIEWS, VIEW = 3, 1
_CHAIN = {}
_YARD = {}

# The bound of test_fuse_hip_against_the_oracle, relative to max |reference|: the project's fuse bound (test_gpu_parity.py: 1e-4 max |ref|).
FWD = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


emit = emitter("wino_dn4hw_matrix")


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
    Ht, Wt, Cin = H // 4, W // 4, C1 + C2
    R = n * D * Ht * Wt                                         # tile rows of the 4 x 4 grid
    vol6, R6 = D // 4 * 6 * Ht * Wt, R // 4 * 6                # operand rows per element / in all
    grid = dw.grid_of(c)
    # ---- forge_wino_input_dn4hw of both operands: bitwise the float32 restatement
    V = {}
    for key, C in (("x1", C1), ("x2", C2)):
        if C == 0:
            continue
        x = padded(d[key], dev)
        vb = OutBuf(dev, 36, R6, C)
        got = twice(lambda: _lib.check(L.forge_wino_input_dn4hw(P(x), C, 0, vb.ptr(), C, 0, n, D, H, W, C, 1, 0, st()), "forge_wino_input_dn4hw"), vb, (c.name, key))
        assert torch.equal(got, dw.input_transform_dn4hw(d[key], 1, F32)), (c.name, "input_dn4hw", key)
        V[key] = got

    def stacked(v, rows, points):                              # V1 as view VIEW of a [n][VIEWS] stack, the other views' rows NaN
        s = torch.full((points, n, VIEWS, rows, C1), NAN)
        s[:, :, VIEW] = v.reshape(points, n, rows, C1)
        return padded(s, dev)
    v1 = stacked(V["x1"], vol6, 36)
    p1 = ctypes.c_void_p(v1.data_ptr() + 4 * VIEW * vol6 * C1)
    v2 = padded(V["x2"], dev) if C2 else None
    Vcat = V["x1"] if not C2 else torch.cat([V["x1"], V["x2"]], dim=-1)
    # ---- forge_wino_weights_dn4hw
    wp = padded(d["wp"], dev)
    ub = OutBuf(dev, 36, 6 * Cout, Cin)
    Ud = twice(lambda: _lib.check(L.forge_wino_weights_dn4hw(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn4hw"), ub, (c.name, "weights_dn4hw"))
    Ud = Ud.reshape(36, 6, Cout, Cin)
    assert torch.equal(Ud, dw.weights_dn4hw(d["wp"], F32)), (c.name, "U is not the float64 evaluation rounded once")
    _lib.check(L.forge_wino_weights_dn4hw(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn4hw")
    # ---- forge_wino_gemm_dn4hw
    mb = OutBuf(dev, 36, R, Cout)
    args = (p1, C1, C1, VIEWS * vol6, n * VIEWS * vol6 * C1, P(v2), C2, C2, 0, 0, ub.ptr(), mb.ptr(), n, D, Ht, Wt, Cout, 3, st())
    Mm = twice(lambda: _lib.check(L.forge_wino_gemm_dn4hw(*args), "forge_wino_gemm_dn4hw"), mb, (c.name, "gemm_dn4hw"))
    ref, mg = dw.nest_gemm(Vcat, Ud, grid), dw.nest_gemm(Vcat, Ud, grid, mag=True)
    r = ((Mm.double() - ref).abs() / (wc.gamma(d4.k_point(Cin)) * mg).clamp_min(1e-300)).max().item()
    q, qr = wc.q_of(Mm, ref, mg)
    emit("%-26s gemm_dn4hw K 6x%-3d R %4d  q %5.2f q_rms %5.3f uncond %.2e" % (c.name, Cin, R, q, qr, r))
    assert r <= 1, (c.name, "point products: unconditional bound exceeded %.3g times" % r)
    # ---- forge_wino_output_dn4hw with the case's GRU tail
    ops, outs = _tail_buffers(c, d, dev)
    ldo = Cout // 2 if c.epi == 2 else Cout
    optr = lambda k: outs[k].ptr() if k in outs else None
    _lib.check(L.forge_wino_gemm_dn4hw(*args), "forge_wino_gemm_dn4hw")

    def inverse():
        _lib.check(L.forge_wino_output_dn4hw(mb.ptr(), P(ops["bias"]), P(ops["scale"]), P(ops["shift"]), P(ops["aux_h"]), P(ops["aux_z"]), optr("out"),
                                             optr("out2"), optr("out3"), n, D, H, W, Cout, ldo, c.epi, st()), "forge_wino_output_dn4hw")
    got = {}
    for _ in range(2):
        for b in outs.values():
            b.t.fill_(cc.CANARY)
        inverse()
        now = {k: b.fetch((c.name, "output_dn4hw", k))[0] for k, b in outs.items()}
        assert all(torch.equal(now[k].view(torch.int32), got.get(k, now[k]).view(torch.int32)) for k in now), (c.name, "two runs of the inverse differ")
        got = now
    _CHAIN[c.name] = dict(d=d, out=got)
    return _CHAIN[c.name]


def yardstick(c, d):
    """(float64 reference outputs, sigma by output, {output: (q, q_rms)} of the float32 CPU evaluation of the 36-point chain in the kernels' order). Computed
    once per case."""
    if c.name not in _YARD:
        ref, sS, sA = dw.chain_dn4hw(c, d, want_sigma=True)
        sig = {k: sS[k] + sA[k] for k in ref}
        cpu = dw.chain_dn4hw(c, d, F32)[0]
        _YARD[c.name] = ref, sig, {k: wc.q_of(cpu[k], ref[k], sig[k]) for k in ref}
    return _YARD[c.name]


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_dn4hw_against_float64(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    for k in ref:
        q, qr = wc.q_of(ch["out"][k], ref[k], sig[k])
        emit("%-26s chain %-4s q %6.2f q_rms %5.3f | yard %6.2f %5.3f" % (name, k, q, qr, yard[k][0], yard[k][1]))
        assert q <= wc.SHARP * yard[k][0] and qr <= wc.SHARP * yard[k][1], (name, k, q, qr, yard[k])


@pytest.mark.parametrize("name", ["dn4hw_n1_d8_h32_w32_o32"])
def test_bounds_reject_wrong_references(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    for mut in dw.MUTATIONS:
        wrong = dw.chain_dn4hw(c, ch["d"], mut=mut)[0]
        ratio = max(max(a / b for a, b in zip(wc.q_of(ch["out"][k], wrong[k], sig[k]), yard[k])) for k in ref)
        emit("%-26s wrong reference %-18s q / yardstick %.3g" % (name, mut, ratio))
        assert ratio > wc.SHARP, (name, mut, ratio)


def test_input_of_a_view_mean(dev):
    """forge_wino_input_dn4hw with nsum > 1 (the argument path the input entries share): the mean of two views sum_stride rows apart, then the three stages,
    torch.equal with the float32 restatement. n = 1, D = 8 (two groups), H = 8, W = 8 (two tile rows and columns), C = 4."""
    L, st = _lib.lib(), _lib.current_stream
    n, D, H, W, C, nsum = 1, 8, 8, 8, 4, 2
    x = torch.randn(nsum, n, D, H, W, C, generator=torch.Generator().manual_seed(21))
    xd = padded(x, dev)
    vb = OutBuf(dev, 36, n * (D // 4) * 6 * (H // 4) * (W // 4), C)
    got = twice(lambda: _lib.check(L.forge_wino_input_dn4hw(P(xd), C, 0, vb.ptr(), C, 0, n, D, H, W, C, nsum, n * D * H * W, st()), "forge_wino_input_dn4hw"),
                vb, "input_dn4hw of a view mean")
    assert torch.equal(got, dw.input_transform_dn4hw(x, nsum, F32))


def test_refusals(dev):
    """Illegal calls return FORGE_EINVAL before any launch; the buffers are large enough for the nearest accepted call."""
    L, st = _lib.lib(), _lib.current_stream
    buf = lambda nfl: torch.zeros(nfl, dtype=F32, device=dev)
    X, V, U, Mm = buf(8 * 32 * 32 * 32), buf(36 * 768 * 64), buf(36 * 6 * 32 * 64), buf(36 * 512 * 32)
    h = buf(8 * 32 * 32 * 32)

    def gemm(D, Ht, Wt, C1=32, C2=0, n=1, Cout=32):
        return L.forge_wino_gemm_dn4hw(P(V), C1, C1, 0, 0, P(V) if C2 else None, C2, C2, 0, 0, P(U), P(Mm), n, D, Ht, Wt, Cout, 3, st())

    def inp(D, H, W):
        return L.forge_wino_input_dn4hw(P(X), 32, 0, P(V), 32, 0, 1, D, H, W, 32, 1, 0, st())

    def outp(H, W):
        return L.forge_wino_output_dn4hw(P(Mm), None, None, None, P(h), P(h), P(X), None, None, 1, 8, H, W, 32, 32, co.EPI_GRU_OUT, st())
    torch.cuda.synchronize()
    assert inp(8, 32, 30) == EINVAL and b"multiple of 4" in L.forge_last_error()  # W % 4 != 0
    assert inp(8, 30, 32) == EINVAL and b"multiple of 4" in L.forge_last_error()  # H % 4 != 0
    assert outp(32, 30) == EINVAL and outp(30, 32) == EINVAL
    assert inp(6, 32, 32) == EINVAL and inp(4, 32, 32) == EINVAL                  # D % 4 != 0, D = 4
    assert gemm(8, 4, 8) == EINVAL and b"Ht Wt" in L.forge_last_error()           # Ht Wt = 32
    assert gemm(6, 8, 8) == EINVAL and b"D % 4" in L.forge_last_error()
    assert gemm(4, 8, 8) == EINVAL and b"at least 8" in L.forge_last_error()
    assert gemm(8, 8, 8, C1=16) == EINVAL and gemm(8, 8, 8, C1=32, C2=16) == EINVAL   # Cin % 32
    assert gemm(8, 64, 64, n=64, C1=256) == EINVAL                                # an operand of 3 GiB
    assert gemm(8, 8, 8, n=4096, Cout=256) == EINVAL                              # an output plane of 2 GiB
    torch.cuda.synchronize()
    assert int(Mm.abs().sum().item()) == 0 and int(V.abs().sum().item()) == 0 and int(X.abs().sum().item()) == 0       # nothing was launched
    assert gemm(8, 8, 8) == 0 and gemm(8, 8, 8, C1=32, C2=32) == 0 and inp(8, 32, 32) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the fusion
# name -> (channels, scenes, D, H, W, lift the rule's tile condition). "c64": the issue's shape; its state launch has Cout = 64, for which forge_wino_gemm_tile
# answers 'C', so the tile condition is lifted (module docstring). "c128": the smallest shape at which convops' rules hold UNPATCHED - Cout >= 128 and
# n D H/4 W/4 = 2048 tile rows of the 4 x 4 grid, the least forge_wino_gemm_tile gives the 64 x 128 tile - so that _fuse_eval's choice runs on the real rule.
FUSE_SHAPES = {"c64": (64, 2, 8, 32, 32, True), "c128": (128, 2, 16, 32, 32, False)}
_FUSE, _REF = {}, {}


def _fuse(dev, monkeypatch, shape, w4):
    """ConvGRU_3D.fuse_hip on FUSE_SHAPES[shape] x 3 views, twice per setting: (x, weights, y, launch counts, y of the second run). Computed once per
    shape and setting."""
    C, b, D, H, W, lift = FUSE_SHAPES[shape]
    monkeypatch.setattr(co.STATE, "wino_depth_nest", True)
    monkeypatch.setattr(co.STATE, "wino_depth_nest4", True)
    monkeypatch.setattr(co.STATE, "wino_h4", True)
    monkeypatch.setattr(co.STATE, "wino_w4", w4)
    if lift:
        monkeypatch.setattr(co, "wino_gemm_tile", lambda R, Cout, Cin: "B")
    if (shape, w4) not in _FUSE:
        case = gc.Case("dn4hw", C, b, D, H, W, (tuple(range(3)),), False, None)
        gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=case.C, hidden_size=case.C)
        w = syn.seeded_state_dict(gru.state_dict(), 9)
        x = torch.randn(case.b, 3, case.C, case.D, case.H, case.W, generator=torch.Generator().manual_seed(14)) * 0.5
        gru.load_state_dict(w)
        gru = gru.to(dev).eval()
        with torch.no_grad(), flopmeter.FlopMeter() as m:
            y = gru.fuse_hip(x.to(dev))
            torch.cuda.synchronize()
        with torch.no_grad():
            y2 = gru.fuse_hip(x.to(dev))
            torch.cuda.synchronize()
        _FUSE[shape, w4] = (x, w, y, m.launches, y2)
    return _FUSE[shape, w4]


def _ref(shape, x, w):
    """The oracle GRU in float64, once per shape."""
    if shape not in _REF:
        with torch.no_grad():
            _REF[shape] = gc.ref_fuse(x.double(), {k: v.double() for k, v in w.items()}, False)
    return _REF[shape]


@pytest.mark.parametrize("shape", list(FUSE_SHAPES))
def test_fuse_hip_against_the_oracle(dev, monkeypatch, shape):
    x, w, y, launches, _ = _fuse(dev, monkeypatch, shape, True)
    # gates + state of three views on the 36 points; fusion_conv's two launches stay on the F(2, 3) nest
    assert launches["forge_wino_gemm_dn4hw"] == 6 and launches["forge_wino_gemm_dn"] == 2, launches
    assert launches["forge_wino_gemm_dn4h"] + launches["forge_wino_gemm_dn4"] + launches["forge_wino_gemm_half"] + launches["forge_wino_gemm"] == 0, launches
    ref = _ref(shape, x, w)
    err = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    _, _, y4, _, _ = _fuse(dev, monkeypatch, shape, False)
    err4 = (y4.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    C, b, D, H, W, _ = FUSE_SHAPES[shape]
    emit("fuse_hip %d x 3 x %dx%dx%dx%d 36-point form: max error / max |ref| %.2e (bound %.2e) | 24-point form %.2e | ratio %.2f" % (
        b, D, H, W, C, err, FWD, err4, err / err4))
    assert err < FWD, err


@pytest.mark.parametrize("shape", list(FUSE_SHAPES))
def test_fuse_hip_switched_off_makes_the_launches_of_before(dev, monkeypatch, shape):
    _, _, y_on, _, _ = _fuse(dev, monkeypatch, shape, True)
    _, _, y_off, launches, y_again = _fuse(dev, monkeypatch, shape, False)
    assert launches["forge_wino_gemm_dn4hw"] == 0 and launches["forge_wino_gemm_dn4h"] == 6 and launches["forge_wino_gemm_dn"] == 2, launches
    assert torch.equal(y_off, y_again)
    assert not torch.equal(y_on, y_off)                        # another rounding order: the switch does select another path
