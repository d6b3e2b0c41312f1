"""CPU, no build: the F(4, 3) depth nest with F(4, 3) along H and W restated in torch (tests/wino_dn4hw_cases.py) is the convolution. In float64 the
whole chain - depth lines, the same six lines over the patch rows and over the patch columns, U = G4 (x) G4 (x) G4, the 36 point products in the depth
nest's schedule, A^T of F(4, 3) over the H points and over the W points - equals F.conv3d; the weights are the float64 Kronecker product rounded once;
each wrong reference of wino_dn4hw_cases.MUTATIONS is far from the convolution (so the GPU test's rejections mean something); the float32 evaluation in
the documented order is measured against float64 beside the 24-point form's (a row of profiles/r30_wino_dn4hw_matrix.txt under -s); the form record, its
rule and the FLOP meter's count.
"""
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import wino_cases as wc
import wino_dn4_cases as d4
import wino_dn4h_cases as dh
import wino_dn4hw_cases as dw

F64 = torch.float64
TAG = "wino_dn4hw_matrix"


def _case(n, D, H, W, C1, C2, Cout):
    return wc.mk("dn4hw_cpu_%d_%d_%d_%d_%d_%d_%d" % (n, D, H, W, C1, C2, Cout), "", n, D, H, W, C1, Cout, C2=C2)


def _conv3d(c, d, bias=True):
    x = d["x1"].double() if d["x2"] is None else torch.cat([d["x1"].double(), d["x2"].double()], dim=-1)
    w = d["wp"].double().reshape(3, 3, 3, c.Cout, c.C1 + c.C2).permute(3, 4, 0, 1, 2)
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, d["bias"].double() if bias else None, padding=1)
    return y.permute(0, 2, 3, 4, 1).reshape(-1, c.Cout)


# H = W = 4: one tile, all of its edges padding; H = 8, W = 12: edge tiles and an interior tile column; two batch elements; an interior depth group at D = 12
CASES = [_case(1, 8, 4, 4, 32, 0, 8), _case(2, 8, 8, 12, 16, 16, 24), _case(1, 12, 12, 4, 32, 0, 16), _case(1, 8, 8, 8, 64, 64, 64)]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_float64_chain_is_conv3d(c):
    d = wc.make_data(c)
    ref = _conv3d(c, d, bias=False)
    got = dw.conv_rows(c, d, F64)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-11 * max(1.0, ref.abs().max().item())
    outs, _, _ = dw.chain_dn4hw(c, d, F64)
    assert (outs["out"] - _conv3d(c, d)).abs().max().item() <= 1e-11 * max(1.0, ref.abs().max().item())


def test_operand_is_bt6_on_depth_rows_and_columns():
    x = torch.randn(1, 8, 8, 12, 3, dtype=F64, generator=torch.Generator().manual_seed(5))
    V = dw.input_transform_dn4hw(x)
    assert V.shape == (36, 1 * 2 * 6 * 2 * 3, 3)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    for g, th, tw in ((0, 0, 0), (1, 1, 2), (1, 0, 1)):
        patch = xp[0, 4 * g:4 * g + 6, 4 * th:4 * th + 6, 4 * tw:4 * tw + 6]                        # [e][i][j][c]
        ref = torch.einsum("ke,ai,bj,eijc->kabc", d4.BT6, d4.BT6, d4.BT6, patch)
        got = V.reshape(6, 6, 1, 2, 6, 2, 3, 3)[:, :, 0, g, :, th, tw].permute(2, 0, 1, 3)         # [k][i'][j'][c]
        assert (got - ref).abs().max().item() <= 1e-12


@pytest.mark.parametrize("c", CASES[:3], ids=lambda c: c.name)
def test_weights_are_the_float64_product_rounded_once(c):
    wp = wc.make_data(c)["wp"]
    Cin = c.C1 + c.C2
    full = torch.einsum("kt,ia,jb,taboc->ijkoc", d4.GD, d4.GD, d4.GD, wp.double().reshape(3, 3, 3, c.Cout, Cin)).reshape(36, 6, c.Cout, Cin)
    U64, U32 = dw.weights_dn4hw(wp), dw.weights_dn4hw(wp, torch.float32)
    assert U64.shape == (36, 6, c.Cout, Cin)
    assert (U64 - full).abs().max().item() <= 1e-15
    assert torch.equal(U32, U64.float())
    # W points 0 and 5 of an H point are a quarter of the first and the whole last W tap of the 24-point form's G4 (x) G4 rows
    w3 = wp.double().reshape(3, 3, 3, c.Cout, Cin)
    last_col = torch.einsum("kt,ia,taoc->ikoc", d4.GD, d4.GD, w3[:, :, 2])
    assert (U64[5::6] - last_col).abs().max().item() <= 1e-15


@pytest.mark.parametrize("mut", dw.MUTATIONS)
def test_wrong_references_are_not_the_convolution(mut):
    c = CASES[1]
    d = wc.make_data(c)
    ref = _conv3d(c, d, bias=False)
    err = (dw.conv_rows(c, d, F64, mut=mut) - ref).abs().max().item()
    assert err > 1e-2 * ref.abs().max().item(), (mut, err)


def test_float32_chain_error_against_the_24_point_form():
    """The float32 evaluation in the kernels' order against float64, in units of u sum |x||w|, beside the 24-point form's on the same inputs (printed: a row of
    the matrix file). The W stage of F(4, 3) amplifies more than F(2, 3)'s: the bound is the ratio of the 1-D stages' own magnitude maps, as
    test_wino_dn4h_cpu.py's for the H stage."""
    c = CASES[3]
    d = wc.make_data(c)
    ref = _conv3d(c, d)
    sig = wc.direct_sums(c, d, True) + d["bias"].abs().double()
    q_new = wc.q_of(dw.chain_dn4hw(c, d, torch.float32)[0]["out"], ref, sig)
    q_old = wc.q_of(dh.chain_dn4h(c, d, torch.float32)[0]["out"], ref, sig)
    print(TAG + " cpu float32 chain 1x8x8x8 64|64->64: dn4hw q %.2f q_rms %.3f | dn4h q %.2f q_rms %.3f | ratio %.2f %.2f" % (
        q_new + q_old + (q_new[0] / q_old[0], q_new[1] / q_old[1])))
    amp4 = (d4.AT6.abs() @ (d4.GD.abs().sum(1) * d4.BT6.abs().sum(1))).max().item()
    amp2 = (wc.AT.abs() @ (wc.G.abs().sum(1) * wc.BT.abs().sum(1))).max().item()
    assert q_new[1] <= (amp4 / amp2) * q_old[1], (q_new, q_old, amp4 / amp2)


def test_form_record_and_rule(monkeypatch):
    from forge_amd import _lib, convops as co
    f = co.WINO_DN4HW
    assert isinstance(f, co.WinoForm) and f.name not in co.WINO_FORMS and f not in co.WINO_FORMS.values()
    assert (f.P, f.points, f.th, f.tw, f.rows, f.kloops, f.metered, f.tile) == (36, 36, 4, 4, Fraction(3, 2), Fraction(3, 2), False, False)
    assert all(g.tw == 2 for g in (*co.WINO_FORMS.values(), co.WINO_DN4H))
    assert {f.gemm, f.weights, f.input, "forge_wino_output_dn4hw"} <= set(_lib.SIGNATURES)
    # shapes = the restatement's: n = 1, D = 8, H = 16, W = 8
    g = torch.Generator().manual_seed(20)
    assert f.ushape(3, 40, 32) == tuple(dw.weights_dn4hw(torch.randn(27, 40, 32, generator=g)).shape)
    V = dw.input_transform_dn4hw(torch.randn(1, 8, 16, 8, 32, generator=g))
    assert V.shape == (f.points, 1 * 8 * (16 // f.th) * (8 // f.tw) * f.rows, 32)
    monkeypatch.setattr(co, "wino_gemm_tile", lambda R, Cout, Cin: "B")
    for k in ("wino_depth_nest", "wino_depth_nest4", "wino_h4", "wino_w4"):
        monkeypatch.setattr(co.STATE, k, True)
    monkeypatch.setattr(co.STATE, "plan_override", None)
    app = lambda D, Ht=8, Wt=8, Cin=256: f.applies(2 * D * Ht * Wt, D, Ht, Wt, 256, Cin)
    assert app(8) and app(32) and app(12) and app(8, Cin=128)
    assert not app(4) and not app(6) and not app(10)                                   # D >= 8, D % 4 == 0
    assert not app(8, 4, 8) and not app(8, 8, 4)                                       # Ht Wt = 32: the grids of the 32-channel nest tests (16 x 32, 32 x 16)
    assert not app(8, Cin=64) and not app(8, Cin=96) and not app(8, Cin=48)            # fewer than 64 channels per operand: fewer than four K-steps per loop
    for k in ("wino_w4", "wino_h4", "wino_depth_nest4", "wino_depth_nest"):
        monkeypatch.setattr(co.STATE, k, False)
        assert not app(8)
        monkeypatch.setattr(co.STATE, k, True)
    # switching the form off leaves the 24-point form's rule as it was
    monkeypatch.setattr(co.STATE, "wino_w4", False)
    assert co.WINO_DN4H.applies(2 * 8 * 4 * 16, 8, 4, 16, 256, 256)
    # the operands: 36 points x 3/8 of the F(4, 3) nest's rows; H and W must be multiples of 4
    assert co.wino_fits(1, 32, 32, 32, 128, views=5, form=f) and not co.wino_fits(1, 32, 32, 30, 128, form=f) and not co.wino_fits(1, 32, 30, 32, 128, form=f)
    assert co.wino_fits(1, 32, 32, 30, 128, form=co.WINO_DN4H)
    n_max = co.MAX_OPERAND_BYTES // (32 * 8 * 8 * Fraction(3, 2) * 128 * 4)
    assert co.wino_fits(int(n_max), 32, 32, 32, 128, form=f) and not co.wino_fits(int(n_max) + 1, 32, 32, 32, 128, form=f)


def test_flop_meter_counts_36_points_of_six_positions_per_four_planes():
    from forge_amd import flopmeter as fm
    n, D, H, W, C1, C2, Cout = 2, 32, 32, 32, 128, 128, 256
    args = lambda tw: [None, C1, C1, 0, 0, None, C2, C2, 0, 0, None, None, n, D, H // 4, W // tw, Cout, 3, None]
    got = fm._ENTRIES["forge_wino_gemm_dn4hw"](args(4))
    assert got == 2.0 * (n * (D // 4) * (H // 4) * (W // 4)) * Cout * 36 * 6 * (C1 + C2)          # 36 x 6 x Cin per four planes and tile
    assert got * 4 == fm._ENTRIES["forge_wino_gemm_dn4h"](args(2)) * 3                             # 3/4 of the 24-point form's work


def test_output_checks_the_36_point_form_before_any_launch(monkeypatch):
    """convops.wino_output takes 36-point products only with the GRU tails, without a second addend or a residual, over n D H/4 W/4 rows."""
    from forge_amd import _lib, convops as co
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was called"))
    meta = lambda *s: torch.empty(*s, device="meta")
    n, D, H, W, Cout = 1, 8, 16, 32, 64
    R = n * D * (H // 4) * (W // 4)
    out = meta(n * D * H * W, Cout)
    call = lambda Mm, epi, **kw: co.wino_output(Mm, None, None, None, 1.0, kw.pop("residual", None), out, out, out, None, None, n, D, H, W, Cout, Cout, epi, **kw)
    for Mm, epi, kw in ((meta(36, R, Cout), co.EPI_BIAS, {}), (meta(36, 2 * R, Cout), co.EPI_GRU_OUT, {}), (meta(36, R, Cout), co.EPI_GRU_OUT, dict(Mm2=meta(36, R, Cout))),
                        (meta(36, R, Cout), co.EPI_GRU_OUT, dict(residual=out)), (meta(36, Cout, R).transpose(1, 2), co.EPI_GRU_OUT, {})):
        with pytest.raises(ValueError):
            call(Mm, epi, **kw)
