"""GPU (-m gpu): the depth nest - forge_wino_gemm_dn / forge_wino_weights_dn - against its float64 restatement (tests/wino_dn_cases.py), through raw
ctypes calls into NaN-patterned buffers, in the shape of test_gpu_wino_matrix.py (whose helpers it repeats in the small).

Shapes: H = W = 16 (exactly one 64-row tile per plane), D in {2, 4, 6} (D = 2: both outer planes of the only pair are out of grid), n in {1, 2} (a pair
must not read across batch elements), (C1, C2) in {(32, 32), (64, 0)} with V1 fed as view 1 of a [n][2] stack whose other view is NaN, Cout in {32, 160}
(ragged below one 128-column tile and across two). Per case:
  weights        forge_wino_weights_dn: torch.equal with the float64 product rounded once
  point products |got - ref| <= gamma_(Cin + 3) sigma on the float32 operands the launch got: one rounding of the operand addition, Cin fused
                 multiply-adds, two output additions (the bound style of wino_cases)
  chain          forge_wino_input -> forge_wino_gemm_dn -> forge_wino_output against float64: q = max |got - ref| / (u sigma) and q_rms within SHARP = 4x
                 the float32 CPU yardstick of the existing form (wino_cases.chain in float32), the bound test_gpu_wino_matrix.py grants
  ratio          q of the nest / q of the four-point chain (forge_wino_gemm_half -> forge_wino_output_half) on the same inputs: printed, a row of
                 profiles/r14_wino_dn_matrix.txt under -s
  repeat         every launch once more on fresh canaries, bitwise
test_bounds_reject_wrong_references: swapped a_k / b_k, the sign of k = 2, y_{z+1} written to plane z, a pair reading across batch elements.
test_refusals: odd D, Ht Wt = 16, one depth tap -> FORGE_EINVAL, no launch. test_fuse_hip_*: ConvGRU_3D.fuse_hip with the switch on against the oracle
GRU in float64 under test_gpu_convgru_matrix.py's forward bound; switched off it makes no nest launch and the four-point launches of before.
"""
import ctypes
import itertools

import pytest
import torch

import conv_igemm_cases as cc
import convgru_cases as gc
import wino_cases as wc
import wino_dn_cases as dn
from wino_gpu_util import EINVAL, F32, FWD, NAN, OutBuf, P, emitter, padded, twice
from forge_amd import _lib, convops as co, flopmeter, synthetic as syn
from forge_amd.fusion import ConvGRU_3D

pytestmark = pytest.mark.gpu

CASES = [wc.mk("dn_n%d_d%d_c%d_%d_o%d" % (n, D, C1, C2, Cout), "", n, D, 16, 16, C1, Cout, C2=C2)
         for D, n, (C1, C2), Cout in itertools.product((2, 4, 6), (1, 2), ((32, 32), (64, 0)), (32, 160))]
CASE = {c.name: c for c in CASES}
_CHAIN = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


emit = emitter("wino_dn_matrix")


def run_chain(c, dev):
    """Every launch of the case (module docstring); returns what the tests read. Computed once per case."""
    if c.name in _CHAIN:
        return _CHAIN[c.name]
    L, st = _lib.lib(), _lib.current_stream
    d = wc.make_data(c)
    n, D, H, W, C1, C2, Cout = c.n, c.D, c.H, c.W, c.C1, c.C2, c.Cout
    Ht, Wt, Cin = H // 2, W // 2, c.C1 + c.C2
    vol, R, M = D * Ht * Wt, wc.R_of(c), c.n * c.D * c.H * c.W
    grid = wc.grid_of(c)
    # ---- forge_wino_input of both operands (bitwise the float32 CPU stage, as the existing matrix pins it)
    V = {}
    for key, C in (("x1", C1), ("x2", C2)):
        if C == 0:
            continue
        x = padded(d[key], dev)
        vb = OutBuf(dev, 16, R, C)
        got = twice(lambda: _lib.check(L.forge_wino_input(P(x), C, 0, vb.ptr(), C, 0, n, D, H, W, C, 1, 0, st()), "forge_wino_input"), vb, (c.name, key))
        assert torch.equal(got, wc.input_transform(d[key], 1, F32)), (c.name, "input", key)
        V[key] = got
    # V1 as view 1 of a [n][2] stack, the other view's rows NaN; V2 dense
    stack = torch.full((16, n, 2, vol, C1), NAN)
    stack[:, :, 1] = V["x1"].reshape(16, n, vol, C1)
    v1 = padded(stack, dev)
    p1 = ctypes.c_void_p(v1.data_ptr() + 4 * vol * C1)
    v2 = padded(V["x2"], dev) if C2 else None
    Vcat = V["x1"] if not C2 else torch.cat([V["x1"], V["x2"]], dim=-1)
    # ---- forge_wino_weights_dn
    wp = padded(d["wp"], dev)
    ub = OutBuf(dev, 16, 4 * Cout, Cin)
    Ud = twice(lambda: _lib.check(L.forge_wino_weights_dn(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn"), ub, (c.name, "weights_dn"))
    Ud = Ud.reshape(16, 4, Cout, Cin)
    assert torch.equal(Ud, dn.weights_dn(d["wp"], F32)), (c.name, "U' is not the float64 product rounded once")
    _lib.check(L.forge_wino_weights_dn(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn")
    # ---- forge_wino_gemm_dn
    mb = OutBuf(dev, 16, R, Cout)
    args = (p1, C1, C1, 2 * vol, n * 2 * vol * C1, P(v2), C2, C2, 0, 0, ub.ptr(), mb.ptr(), n, D, Ht, Wt, Cout, 3, st())
    Mm = twice(lambda: _lib.check(L.forge_wino_gemm_dn(*args), "forge_wino_gemm_dn"), mb, (c.name, "gemm_dn"))
    ref, mg = dn.nest_gemm(Vcat, Ud, grid), dn.nest_gemm(Vcat, Ud, grid, mag=True)
    r = ((Mm.double() - ref).abs() / (wc.gamma(Cin + 3) * mg).clamp_min(1e-300)).max().item()
    q, qr = wc.q_of(Mm, ref, mg)
    emit("%-22s gemm_dn K 4x%-3d R %4d  q %5.2f q_rms %5.3f uncond %.2e" % (c.name, Cin, R, q, qr, r))
    assert r <= 1, (c.name, "point products: unconditional bound exceeded %.3g times" % r)
    # ---- forge_wino_output (bias) on the nest's 16 planes, and the four-point chain on the same inputs
    bias = padded(d["bias"], dev)
    ob = OutBuf(dev, 1, M, Cout)
    _lib.check(L.forge_wino_gemm_dn(*args), "forge_wino_gemm_dn")
    out_args = lambda m: (m.ptr(), None, 0, 0, P(bias), None, None, 1.0, None, None, None, ob.ptr(), None, None, n, D, H, W, Cout, Cout, co.EPI_BIAS, st())
    out = twice(lambda: _lib.check(L.forge_wino_output(*out_args(mb)), "forge_wino_output"), ob, (c.name, "output"))[0]
    U3 = padded(wc.weights(d["wp"], 3, dtype=F32), dev)
    m8 = OutBuf(dev, 8, R, Cout)
    _lib.check(L.forge_wino_gemm_half(p1, C1, C1, 2 * vol, n * 2 * vol * C1, P(v2), C2, C2, 0, 0, P(U3), m8.ptr(), n, D, Ht, Wt, Cout, 3, st()),
               "forge_wino_gemm_half")
    m8.fetch((c.name, "gemm_half"))
    ob.t.fill_(cc.CANARY)
    _lib.check(L.forge_wino_output_half(*out_args(m8)), "forge_wino_output_half")
    out4 = ob.fetch((c.name, "output_half"))[0]
    _CHAIN[c.name] = dict(d=d, out=out, out4=out4)
    return _CHAIN[c.name]


def yardstick(c, d):
    """(float64 reference rows, sigma, (q, q_rms) of the existing form's float32 CPU evaluation) - the existing matrix's chain yardstick."""
    ref, sS, sA = wc.chain(c, d, want_sigma=True)
    sig = sS["out"] + sA["out"]
    y, _, _ = wc.chain(c, d, F32)
    return ref["out"], sig, wc.q_of(y["out"], ref["out"], sig)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_nest_against_float64(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    q, qr = wc.q_of(ch["out"], ref, sig)
    q4, qr4 = wc.q_of(ch["out4"], ref, sig)
    emit("%-22s chain   q %5.2f q_rms %5.3f | four-point q %5.2f q_rms %5.3f | ratio %4.2f %4.2f | yard %5.2f %5.3f" % (
        name, q, qr, q4, qr4, q / q4, qr / qr4, yard[0], yard[1]))
    assert q <= wc.SHARP * yard[0] and qr <= wc.SHARP * yard[1], (name, "chain", q, qr, yard)


@pytest.mark.parametrize("name", ["dn_n2_d4_c32_32_o160", "dn_n2_d2_c64_0_o32"])
def test_bounds_reject_wrong_references(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    for mut in dn.MUTATIONS:
        wrong = dn.chain_dn(c, ch["d"], mut=mut)
        ratio = max(a / b for a, b in zip(wc.q_of(ch["out"], wrong, sig), yard))
        emit("%-22s wrong reference %-12s q / yardstick %.3g" % (name, mut, ratio))
        assert ratio > wc.SHARP, (name, mut, ratio)


def test_refusals(dev):
    """Illegal calls return FORGE_EINVAL before any launch; the buffers are large enough for the nearest accepted call."""
    L, st = _lib.lib(), _lib.current_stream
    buf = lambda nfl: torch.zeros(nfl, dtype=F32, device=dev)
    V, U, Mm = buf(16 * 512 * 32), buf(16 * 4 * 32 * 32), buf(16 * 512 * 32)
    call = lambda D, Ht, Wt, kd, C=32: L.forge_wino_gemm_dn(P(V), C, C, 0, 0, None, 0, 0, 0, 0, P(U), P(Mm), 1, D, Ht, Wt, 32, kd, st())
    torch.cuda.synchronize()
    assert call(3, 8, 8, 3) == EINVAL and b"even D" in L.forge_last_error()
    assert call(2, 4, 4, 3) == EINVAL
    assert call(2, 8, 8, 1) == EINVAL
    assert call(2, 8, 8, 3, C=16) == EINVAL
    torch.cuda.synchronize()
    assert int(Mm.abs().sum().item()) == 0                     # nothing was launched
    assert call(2, 8, 8, 3) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the fusion
def _fusion_case():
    return gc.Case("dn", 32, 2, 4, 16, 16, (tuple(range(3)),), False, None)


def _fuse(dev, monkeypatch, on):
    """ConvGRU_3D.fuse_hip on 2 scenes x 3 views x 4 x 16 x 16 x 32. At 32 channels forge_wino_gemm would not take its 64 x 128 tile, so the rule's tile
    condition is lifted for the test (the entry's own preconditions stay): the launches then run the nest kernel on this small shape."""
    case = _fusion_case()
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=case.C, hidden_size=case.C)
    w = syn.seeded_state_dict(gru.state_dict(), 9)
    x = torch.randn(case.b, 3, case.C, case.D, case.H, case.W, generator=torch.Generator().manual_seed(14)) * 0.5
    gru.load_state_dict(w)
    gru = gru.to(dev).eval()
    monkeypatch.setattr(co.STATE, "wino_depth_nest", on)
    monkeypatch.setattr(co, "wino_gemm_tile", lambda R, Cout, Cin: "B")
    with torch.no_grad(), flopmeter.FlopMeter() as m:
        y = gru.fuse_hip(x.to(dev))
        torch.cuda.synchronize()
    return x, w, y, m.launches


def test_fuse_hip_with_the_nest_against_the_oracle(dev, monkeypatch):
    x, w, y, launches = _fuse(dev, monkeypatch, True)
    assert launches["forge_wino_gemm_dn"] == 8, launches       # fusion_conv twice, gates + state of three views
    with torch.no_grad():
        ref = gc.ref_fuse(x.double(), {k: v.double() for k, v in w.items()}, False)
    err = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    emit("fuse_hip 2 x 3 x 4x16x16x32 nest on: max error / max |ref| %.2e (bound %.0e)" % (err, FWD))
    assert err < FWD, err


def test_fuse_hip_switched_off_makes_the_launches_of_before(dev, monkeypatch):
    _, _, y_off, launches = _fuse(dev, monkeypatch, False)
    assert launches["forge_wino_gemm_dn"] == 0 and launches["forge_wino_gemm_half"] + launches["forge_wino_gemm"] == 8, launches
    _, _, y_again, _ = _fuse(dev, monkeypatch, False)
    assert torch.equal(y_off, y_again)
    _, _, y_on, _ = _fuse(dev, monkeypatch, True)
    assert not torch.equal(y_on, y_off)                        # another rounding order: the switch does select another path
