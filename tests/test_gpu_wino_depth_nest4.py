"""GPU (-m gpu): the F(4, 3) depth nest - forge_wino_input_dn4 / forge_wino_weights_dn4 / forge_wino_gemm_dn4 - against its restatement
(tests/wino_dn4_cases.py), through raw ctypes calls into canary-patterned buffers with guard rows, in the shape of test_gpu_wino_depth_nest.py.

Shapes: H = W = 16 (exactly one 64-row tile per plane), n = 2 (a group must not read across batch elements), D = 8 (two groups per element: the lower
grid edge, an interior group boundary, the upper edge) and one case at D = 4 through the C entry (every group touches both edges; the Python rule leaves
that depth to F(2, 3)), (C1, C2) in {(32, 32), (64, 0)}, Cout in {32, 160} (ragged below one 128-column tile and across two). V1 is fed as view 1 of a
[n][2] stack of forge_wino_input_dn4 outputs whose other view is NaN. Per case:
  transform      forge_wino_input_dn4: torch.equal with the float32 restatement (depth stage in the documented order, then B^T q B)
  weights        forge_wino_weights_dn4: torch.equal with the float64 evaluation in the documented order, rounded once
  point products |got - ref| <= gamma_(2 Cin + 2) sum |operand||weight| on the float32 operands the launch got (wino_dn4_cases.k_point: a term's own Cin
                 fused multiply-adds, two combinations, and the Cin steps of the position accumulated onto it)
  chain          forge_wino_input_dn4 -> forge_wino_gemm_dn4 -> forge_wino_output against float64: q = max |got - ref| / (u sigma) and q_rms within
                 SHARP = 4x the float32 CPU evaluation of THIS algorithm (wino_dn4_cases.chain_dn4 in float32)
  ratio          q against the F(2, 3) nest and the four-point chain on the same inputs: printed, a row of profiles/r18_wino_dn4_matrix.txt under -s
  repeat         every launch once more on fresh canaries, bitwise
test_bounds_reject_wrong_references: a swapped +- pair, a wrong sign in row 3 of A^T, rotated output planes, planes taken across the batch boundary.
test_input_dn4_of_a_view_mean: forge_wino_input_dn4 with nsum = 2 on 1 x 8 x 4 x 4 x 4, torch.equal with the float32 restatement.
test_refusals: D % 4 != 0, Ht Wt = 16, one depth tap, C1 / C2 not multiples of 32, an output plane beyond 32-bit offsets -> FORGE_EINVAL, no launch.
test_fuse_hip_*: ConvGRU_3D.fuse_hip on 2 scenes x 3 views x 8 x 16 x 16 x 32 against the oracle GRU in float64 under test_gpu_convgru_matrix.py's forward
bound, launch counts by entry; either switch off gives the launches and bits of before.
"""
import ctypes
import itertools

import pytest
import torch

import conv_igemm_cases as cc
import convgru_cases as gc
import wino_cases as wc
import wino_dn4_cases as d4
import wino_dn_cases as dn
from wino_gpu_util import EINVAL, F32, FWD, NAN, OutBuf, P, emitter, padded, twice
from forge_amd import _lib, convops as co, flopmeter, synthetic as syn
from forge_amd.fusion import ConvGRU_3D

pytestmark = pytest.mark.gpu

CASES = [wc.mk("dn4_n2_d8_c%d_%d_o%d" % (C1, C2, Cout), "", 2, 8, 16, 16, C1, Cout, C2=C2) for (C1, C2), Cout in itertools.product(((32, 32), (64, 0)), (32, 160))]
CASES.append(wc.mk("dn4_n2_d4_c32_32_o32", "", 2, 4, 16, 16, 32, 32, C2=32))
CASE = {c.name: c for c in CASES}
_CHAIN = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


emit = emitter("wino_dn4_matrix")


def run_chain(c, dev):
    """Every launch of the case (module docstring); returns what the tests read. Computed once per case."""
    if c.name in _CHAIN:
        return _CHAIN[c.name]
    L, st = _lib.lib(), _lib.current_stream
    d = wc.make_data(c)
    n, D, H, W, C1, C2, Cout = c.n, c.D, c.H, c.W, c.C1, c.C2, c.Cout
    Ht, Wt, Cin = H // 2, W // 2, c.C1 + c.C2
    vol, R, M = D * Ht * Wt, wc.R_of(c), c.n * c.D * c.H * c.W
    vol6, R6 = vol // 4 * 6, R // 4 * 6
    grid = wc.grid_of(c)
    # ---- forge_wino_input_dn4 of both operands: bitwise the float32 restatement; forge_wino_input for the existing forms' chains
    V6, V = {}, {}
    for key, C in (("x1", C1), ("x2", C2)):
        if C == 0:
            continue
        x = padded(d[key], dev)
        vb = OutBuf(dev, 16, R6, C)
        got = twice(lambda: _lib.check(L.forge_wino_input_dn4(P(x), C, 0, vb.ptr(), C, 0, n, D, H, W, C, 1, 0, st()), "forge_wino_input_dn4"), vb, (c.name, key))
        assert torch.equal(got, d4.input_transform_dn4(d[key], 1, F32)), (c.name, "input_dn4", key)
        V6[key] = got
        V[key] = wc.input_transform(d[key], 1, F32)
    # V1 as view 1 of a [n][2] stack, the other view's rows NaN; V2 dense
    def stacked(v, rows):
        s = torch.full((16, n, 2, rows, C1), NAN)
        s[:, :, 1] = v.reshape(16, n, rows, C1)
        return padded(s, dev)
    v1 = stacked(V6["x1"], vol6)
    p1 = ctypes.c_void_p(v1.data_ptr() + 4 * vol6 * C1)
    v2 = padded(V6["x2"], dev) if C2 else None
    Vcat6 = V6["x1"] if not C2 else torch.cat([V6["x1"], V6["x2"]], dim=-1)
    # ---- forge_wino_weights_dn4
    wp = padded(d["wp"], dev)
    ub = OutBuf(dev, 16, 6 * Cout, Cin)
    Ud = twice(lambda: _lib.check(L.forge_wino_weights_dn4(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn4"), ub, (c.name, "weights_dn4"))
    Ud = Ud.reshape(16, 6, Cout, Cin)
    assert torch.equal(Ud, d4.weights_dn4(d["wp"], F32)), (c.name, "U'' is not the float64 evaluation rounded once")
    _lib.check(L.forge_wino_weights_dn4(P(wp), ub.ptr(), Cout, Cin, st()), "forge_wino_weights_dn4")
    # ---- forge_wino_gemm_dn4
    mb = OutBuf(dev, 16, R, Cout)
    args = (p1, C1, C1, 2 * vol6, n * 2 * vol6 * C1, P(v2), C2, C2, 0, 0, ub.ptr(), mb.ptr(), n, D, Ht, Wt, Cout, 3, st())
    Mm = twice(lambda: _lib.check(L.forge_wino_gemm_dn4(*args), "forge_wino_gemm_dn4"), mb, (c.name, "gemm_dn4"))
    ref, mg = d4.nest_gemm4(Vcat6, Ud, grid), d4.nest_gemm4(Vcat6, Ud, grid, mag=True)
    r = ((Mm.double() - ref).abs() / (wc.gamma(d4.k_point(Cin)) * mg).clamp_min(1e-300)).max().item()
    q, qr = wc.q_of(Mm, ref, mg)
    emit("%-22s gemm_dn4 K 6x%-3d R %4d  q %5.2f q_rms %5.3f uncond %.2e" % (c.name, Cin, R, q, qr, r))
    assert r <= 1, (c.name, "point products: unconditional bound exceeded %.3g times" % r)
    # ---- forge_wino_output (bias) on the nest's 16 planes; the F(2, 3) nest and the four-point chain on the same inputs
    bias = padded(d["bias"], dev)
    ob = OutBuf(dev, 1, M, Cout)
    _lib.check(L.forge_wino_gemm_dn4(*args), "forge_wino_gemm_dn4")
    out_args = lambda m: (m.ptr(), None, 0, 0, P(bias), None, None, 1.0, None, None, None, ob.ptr(), None, None, n, D, H, W, Cout, Cout, co.EPI_BIAS, st())
    out = twice(lambda: _lib.check(L.forge_wino_output(*out_args(mb)), "forge_wino_output"), ob, (c.name, "output"))[0]
    w1 = stacked(V["x1"], vol)
    q1 = ctypes.c_void_p(w1.data_ptr() + 4 * vol * C1)
    w2 = padded(V["x2"], dev) if C2 else None
    old = (q1, C1, C1, 2 * vol, n * 2 * vol * C1, P(w2), C2, C2, 0, 0)
    U2 = padded(dn.weights_dn(d["wp"], F32), dev)
    _lib.check(L.forge_wino_gemm_dn(*old, P(U2), mb.ptr(), n, D, Ht, Wt, Cout, 3, st()), "forge_wino_gemm_dn")
    ob.t.fill_(cc.CANARY)
    _lib.check(L.forge_wino_output(*out_args(mb)), "forge_wino_output")
    out2 = ob.fetch((c.name, "output of F(2, 3)"))[0]
    U3 = padded(wc.weights(d["wp"], 3, dtype=F32), dev)
    m8 = OutBuf(dev, 8, R, Cout)
    _lib.check(L.forge_wino_gemm_half(*old, P(U3), m8.ptr(), n, D, Ht, Wt, Cout, 3, st()), "forge_wino_gemm_half")
    m8.fetch((c.name, "gemm_half"))
    ob.t.fill_(cc.CANARY)
    _lib.check(L.forge_wino_output_half(*out_args(m8)), "forge_wino_output_half")
    out4 = ob.fetch((c.name, "output_half"))[0]
    _CHAIN[c.name] = dict(d=d, out=out, out2=out2, out4=out4)
    return _CHAIN[c.name]


def yardstick(c, d):
    """(float64 reference rows, sigma, (q, q_rms) of the float32 CPU evaluation of the F(4, 3) nest in the kernel's order)."""
    ref, sS, sA = wc.chain(c, d, want_sigma=True)
    sig = sS["out"] + sA["out"]
    return ref["out"], sig, wc.q_of(d4.chain_dn4(c, d, F32), ref["out"], sig)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_nest4_against_float64(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    (q, qr), (q2, qr2), (q4, qr4) = (wc.q_of(ch[k], ref, sig) for k in ("out", "out2", "out4"))
    emit("%-22s chain   q %5.2f q_rms %5.3f | F(2,3) nest q %5.2f q_rms %5.3f | four-point q %5.2f q_rms %5.3f | ratio to F(2,3) %4.2f %4.2f | yard %5.2f %5.3f" % (
        name, q, qr, q2, qr2, q4, qr4, q / q2, qr / qr2, yard[0], yard[1]))
    assert q <= wc.SHARP * yard[0] and qr <= wc.SHARP * yard[1], (name, "chain", q, qr, yard)


@pytest.mark.parametrize("name", ["dn4_n2_d8_c32_32_o160", "dn4_n2_d4_c32_32_o32"])
def test_bounds_reject_wrong_references(dev, name):
    c = CASE[name]
    ch = run_chain(c, dev)
    ref, sig, yard = yardstick(c, ch["d"])
    for mut in d4.MUTATIONS:
        wrong = d4.chain_dn4(c, ch["d"], mut=mut)
        ratio = max(a / b for a, b in zip(wc.q_of(ch["out"], wrong, sig), yard))
        emit("%-22s wrong reference %-12s q / yardstick %.3g" % (name, mut, ratio))
        assert ratio > wc.SHARP, (name, mut, ratio)


def test_input_dn4_of_a_view_mean(dev):
    """forge_wino_input_dn4 with nsum > 1 - the argument path the three input entries share, otherwise only pinned for the plain transform: the mean of
    two views sum_stride rows apart, then both stages, torch.equal with the float32 restatement. The smallest shape with an interior and both depth
    edges: n = 1, D = 8 (two groups), H = W = 4, C = 4."""
    L, st = _lib.lib(), _lib.current_stream
    n, D, H, W, C, nsum = 1, 8, 4, 4, 4, 2
    x = torch.randn(nsum, n, D, H, W, C, generator=torch.Generator().manual_seed(20))
    xd = padded(x, dev)
    vb = OutBuf(dev, 16, n * (D // 4) * 6 * (H // 2) * (W // 2), C)
    got = twice(lambda: _lib.check(L.forge_wino_input_dn4(P(xd), C, 0, vb.ptr(), C, 0, n, D, H, W, C, nsum, n * D * H * W, st()), "forge_wino_input_dn4"),
                vb, "input_dn4 of a view mean")
    assert torch.equal(got, d4.input_transform_dn4(x, nsum, F32))


def test_refusals(dev):
    """Illegal calls return FORGE_EINVAL before any launch; the buffers are large enough for the nearest accepted call."""
    L, st = _lib.lib(), _lib.current_stream
    buf = lambda nfl: torch.zeros(nfl, dtype=F32, device=dev)
    V, U, Mm = buf(16 * 768 * 64), buf(16 * 6 * 32 * 64), buf(16 * 512 * 32)
    def call(D, Ht, Wt, kd, C1=32, C2=0, n=1, Cout=32):
        return L.forge_wino_gemm_dn4(P(V), C1, C1, 0, 0, P(V) if C2 else None, C2, C2, 0, 0, P(U), P(Mm), n, D, Ht, Wt, Cout, kd, st())
    torch.cuda.synchronize()
    assert call(6, 8, 8, 3) == EINVAL and b"D % 4" in L.forge_last_error()
    assert call(2, 8, 8, 3) == EINVAL
    assert call(4, 4, 4, 3) == EINVAL
    assert call(4, 8, 8, 1) == EINVAL
    assert call(4, 8, 8, 3, C1=16) == EINVAL
    assert call(4, 8, 8, 3, C1=32, C2=16) == EINVAL
    assert call(8, 8, 8, 3, n=4096, Cout=256) == EINVAL          # an output plane of 2 GiB
    assert call(8, 64, 64, 3, n=64, C1=256) == EINVAL            # an operand of 3 GiB
    torch.cuda.synchronize()
    assert int(Mm.abs().sum().item()) == 0                     # nothing was launched
    assert call(4, 8, 8, 3) == 0 and call(8, 8, 8, 3, C1=32, C2=32) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the fusion
def _fuse(dev, monkeypatch, nest, nest4):
    """ConvGRU_3D.fuse_hip on 2 scenes x 3 views x 8 x 16 x 16 x 32. At 32 channels forge_wino_gemm would not take its 64 x 128 tile, so the rule's tile
    condition is lifted for the test (the entries' own preconditions stay), as test_gpu_wino_depth_nest.py does."""
    case = gc.Case("dn4", 32, 2, 8, 16, 16, (tuple(range(3)),), False, None)
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=case.C, hidden_size=case.C)
    w = syn.seeded_state_dict(gru.state_dict(), 9)
    x = torch.randn(case.b, 3, case.C, case.D, case.H, case.W, generator=torch.Generator().manual_seed(14)) * 0.5
    gru.load_state_dict(w)
    gru = gru.to(dev).eval()
    monkeypatch.setattr(co.STATE, "wino_depth_nest", nest)
    monkeypatch.setattr(co.STATE, "wino_depth_nest4", nest4)
    monkeypatch.setattr(co, "wino_gemm_tile", lambda R, Cout, Cin: "B")
    with torch.no_grad(), flopmeter.FlopMeter() as m:
        y = gru.fuse_hip(x.to(dev))
        torch.cuda.synchronize()
    return x, w, y, m.launches


def test_fuse_hip_with_the_nest4_against_the_oracle(dev, monkeypatch):
    x, w, y, launches = _fuse(dev, monkeypatch, True, True)
    # gates + state of three views on F(4, 3); fusion_conv's two launches stay on F(2, 3)
    assert launches["forge_wino_gemm_dn4"] == 6 and launches["forge_wino_gemm_dn"] == 2, launches
    assert launches["forge_wino_gemm_half"] + launches["forge_wino_gemm"] == 0, launches
    with torch.no_grad():
        ref = gc.ref_fuse(x.double(), {k: v.double() for k, v in w.items()}, False)
    err = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    emit("fuse_hip 2 x 3 x 8x16x16x32 nest4 on: max error / max |ref| %.2e (bound %.0e)" % (err, FWD))
    assert err < FWD, err


def test_fuse_hip_switched_off_makes_the_launches_of_before(dev, monkeypatch):
    _, _, y_on, _ = _fuse(dev, monkeypatch, True, True)
    _, _, y_f23, launches = _fuse(dev, monkeypatch, True, False)
    assert launches["forge_wino_gemm_dn4"] == 0 and launches["forge_wino_gemm_dn"] == 8, launches
    _, _, y_again, _ = _fuse(dev, monkeypatch, True, False)
    assert torch.equal(y_f23, y_again)
    assert not torch.equal(y_on, y_f23)                        # another rounding order: the switch does select another path
    _, _, y_off, launches = _fuse(dev, monkeypatch, False, True)
    assert launches["forge_wino_gemm_dn4"] == 0 and launches["forge_wino_gemm_dn"] == 0, launches
    assert launches["forge_wino_gemm_half"] + launches["forge_wino_gemm"] == 8, launches
    _, _, y_off2, _ = _fuse(dev, monkeypatch, False, False)
    assert torch.equal(y_off, y_off2)
