"""CPU: the F(4, 3) depth nest restated in torch (tests/wino_dn4_cases.py) is the convolution. The three matrices are an exact F(4, 3) on a 1-D
example; in float64 the depth stage, U'', the six products and the four rows in the kernel's order equal F.conv3d to rounding; U'' in float32 is the
float64 evaluation rounded once and agrees with the matrix product; each wrong reference of wino_dn4_cases.MUTATIONS is far from the convolution (so the
GPU test's rejections mean something); the rule takes D = 8 / 32 / 64 and leaves D = 4 and both switches; the FLOP meter counts 6 positions per 4 planes."""
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import wino_cases as wc
import wino_dn4_cases as d4

F64 = torch.float64


def _case(n, D, C1, C2, Cout, H=8, W=8):
    return wc.mk("dn4_cpu_%d_%d_%d_%d_%d" % (n, D, C1, C2, Cout), "", n, D, H, W, C1, Cout, C2=C2)


def _conv3d(c, d):
    x = d["x1"].double() if d["x2"] is None else torch.cat([d["x1"].double(), d["x2"].double()], dim=-1)
    w = d["wp"].double().reshape(3, 3, 3, c.Cout, c.C1 + c.C2).permute(3, 4, 0, 1, 2)
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, d["bias"].double(), padding=1)
    return y.permute(0, 2, 3, 4, 1).reshape(-1, c.Cout)


CASES = [_case(1, 4, 32, 0, 8), _case(2, 8, 16, 16, 24), _case(2, 12, 64, 0, 40, 4, 4), _case(1, 8, 64, 64, 64, 4, 4)]


def test_matrices_are_an_exact_f43():
    """A^T [(G g) . (B^T d)] = the four outputs of the 3-tap correlation of six inputs, in exact rational arithmetic."""
    fr = lambda M, den: [[Fraction(int(round(v * den)), den) for v in row] for row in M.tolist()]
    BT, G, AT = fr(d4.BT6, 1), fr(d4.GD, 24), fr(d4.AT6, 1)
    assert G[1] == [Fraction(-1, 6)] * 3 and G[3] == [Fraction(1, 24), Fraction(1, 12), Fraction(1, 6)]
    dvec, g = [Fraction(v) for v in (3, -1, 4, 1, -5, 9)], [Fraction(v) for v in (2, 7, -3)]
    U = [sum(G[k][t] * g[t] for t in range(3)) for k in range(6)]
    V = [sum(BT[k][e] * dvec[e] for e in range(6)) for k in range(6)]
    y = [sum(AT[i][k] * U[k] * V[k] for k in range(6)) for i in range(4)]
    assert y == [sum(g[t] * dvec[i + t] for t in range(3)) for i in range(4)]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_float64_nest_is_conv3d(c):
    d = wc.make_data(c)
    ref = _conv3d(c, d)
    got = d4.chain_dn4(c, d, F64)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_depth_stage_is_bt6_and_keeps_to_the_batch_element():
    x = torch.randn(2, 8, 2, 2, 3, dtype=F64, generator=torch.Generator().manual_seed(3))
    q = d4.depth_stage(x)
    xp = F.pad(x, (0, 0, 0, 0, 0, 0, 1, 1))
    for g in range(2):
        ref = torch.einsum("ke,nehwc->nkhwc", d4.BT6, xp[:, 4 * g:4 * g + 6])
        assert (q[:, g] - ref).abs().max().item() <= 1e-13
    assert (d4.depth_stage(x, cross=True) - q).abs().max().item() > 0.1


@pytest.mark.parametrize("c", CASES[:3], ids=lambda c: c.name)
def test_weights_are_the_float64_product_rounded_once(c):
    wp = wc.make_data(c)["wp"]
    full = torch.einsum("kt,ia,jb,taboc->ijkoc", d4.GD, wc.G, wc.G, wp.double().reshape(3, 3, 3, c.Cout, c.C1 + c.C2)).reshape(16, 6, c.Cout, c.C1 + c.C2)
    U64, U32 = d4.weights_dn4(wp), d4.weights_dn4(wp, torch.float32)
    assert (U64 - full).abs().max().item() <= 1e-15
    assert torch.equal(U32, U64.float())
    # position 5 is the last depth tap of the 2-D weights, untouched; position 0 a quarter of the first
    U = wc.weights(wp, 3, dtype=torch.float32)
    assert torch.equal(U32[:, 5], U[:, 2]) and torch.equal(U32[:, 0], 0.25 * U[:, 0])


@pytest.mark.parametrize("mut", d4.MUTATIONS)
def test_wrong_references_are_not_the_convolution(mut):
    c = CASES[1]                                       # n = 2, D = 8: an interior group edge and the batch boundary
    d = wc.make_data(c)
    ref = _conv3d(c, d)
    err = (d4.chain_dn4(c, d, F64, mut=mut) - ref).abs().max().item()
    assert err > 1e-2 * ref.abs().max().item(), (mut, err)


def test_float32_nest_error_against_the_existing_forms():
    """The float32 restatement in the kernel's order against float64, in units of u sum |x||w|: printed beside the existing form's; the depth stage of
    F(4, 3) amplifies more than F(2, 3)'s (interpolation points 0, +-1, +-2), so the bound here is the ratio of the transforms' own magnitude maps."""
    c = CASES[3]
    d = wc.make_data(c)
    ref = _conv3d(c, d)
    sig = wc.direct_sums(c, d, True) + d["bias"].abs().double()
    q_new = wc.q_of(d4.chain_dn4(c, d, torch.float32), ref, sig)
    outs, _, _ = wc.chain(c, d, torch.float32)
    q_old = wc.q_of(outs["out"], ref, sig)
    print("dn4 float32 chain q %.2f q_rms %.3f | existing form q %.2f q_rms %.3f" % (q_new + q_old))
    # amplification of the 1-D stage: sum_k |A^T||G||B^T| row sums - F(4, 3): max_i sum_k |AT6[i][k]| sum_t |GD[k][t]| sum_e |BT6[k][e]| against F(2, 3)'s
    amp4 = (d4.AT6.abs() @ (d4.GD.abs().sum(1) * d4.BT6.abs().sum(1))).max().item()
    amp2 = (wc.AT.abs() @ (wc.G.abs().sum(1) * wc.BT.abs().sum(1))).max().item()
    assert q_new[1] <= (amp4 / amp2) * q_old[1], (q_new, q_old, amp4 / amp2)


def test_rule(monkeypatch):
    from forge_amd import convops as co
    monkeypatch.setattr(co, "wino_gemm_tile", lambda R, Cout, Cin: "B")
    monkeypatch.setattr(co.STATE, "wino_depth_nest", True)
    monkeypatch.setattr(co.STATE, "wino_depth_nest4", True)
    monkeypatch.setattr(co.STATE, "plan_override", None)
    app = lambda D: co.wino_depth_nest4_applies(2 * D * 64, D, 8, 8, 256, 256)
    assert not app(4) and co.wino_depth_nest_applies(2 * 4 * 64, 4, 8, 8, 256, 256)      # D = 4 stays on F(2, 3)
    assert app(8) and app(32) and app(64)
    assert not app(6) and not app(10)
    assert not co.wino_depth_nest4_applies(8 * 16, 8, 4, 4, 256, 256)                   # Ht Wt = 16
    assert not co.wino_depth_nest4_applies(8 * 64, 8, 8, 8, 256, 48)                    # Cin not a multiple of 32
    monkeypatch.setattr(co.STATE, "wino_depth_nest4", False)
    assert not app(8) and co.wino_depth_nest_applies(2 * 8 * 64, 8, 8, 8, 256, 256)
    monkeypatch.setattr(co.STATE, "wino_depth_nest4", True)
    monkeypatch.setattr(co.STATE, "wino_depth_nest", False)
    assert not app(8)
    assert co.wino_fits(1, 32, 32, 32, 128, views=4, nest4=True) and not co.wino_fits(100, 32, 32, 32, 128, views=4, nest4=True)
    assert co.wino_fits(100, 32, 32, 32, 128, views=4)


def test_flop_meter_counts_six_positions_per_four_planes():
    from forge_amd import flopmeter as fm
    args = [None, 128, 128, 0, 0, None, 128, 128, 0, 0, None, None, 2, 32, 16, 16, 256, 3]
    assert fm._wino_gemm_dn4(args + [None]) * 2 == fm._wino_gemm(args + [0, None])        # 1.5 of 3 loops per plane
    assert fm._wino_gemm_dn4(args + [None]) * 4 == fm._wino_gemm_dn(args + [None]) * 3
    assert fm._wino_gemm_dn4(args + [None]) == 2.0 * 16 * (2 * 32 * 256 // 4) * 256 * 6 * 256
    assert "forge_wino_gemm_dn4" in fm._ENTRIES
