"""CPU: the depth nest restated in torch (tests/wino_dn_cases.py) is the convolution. In float64 the input combination, U', the four products and
y_z / y_{z+1} in the kernel's order equal F.conv3d at 1e-12; U' in float32 is the float64 product rounded once; each wrong reference of
wino_dn_cases.MUTATIONS is far from the convolution (so the GPU test's rejections mean something); the FLOP meter counts 2/3 of forge_wino_gemm's work."""
import pytest
import torch
import torch.nn.functional as F

import wino_cases as wc
import wino_dn_cases as dn

F64 = torch.float64


def _case(n, D, C1, C2, Cout, H=8, W=8):
    return wc.mk("dn_cpu_%d_%d_%d_%d_%d" % (n, D, C1, C2, Cout), "", n, D, H, W, C1, Cout, C2=C2)


def _conv3d(c, d):
    x = d["x1"].double() if d["x2"] is None else torch.cat([d["x1"].double(), d["x2"].double()], dim=-1)
    w = d["wp"].double().reshape(3, 3, 3, c.Cout, c.C1 + c.C2).permute(3, 4, 0, 1, 2)
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, d["bias"].double(), padding=1)
    return y.permute(0, 2, 3, 4, 1).reshape(-1, c.Cout)


CASES = [_case(1, 2, 32, 0, 8), _case(2, 4, 16, 16, 24), _case(2, 6, 64, 0, 64), _case(1, 8, 128, 128, 128, 4, 4)]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_float64_nest_is_conv3d(c):
    d = wc.make_data(c)
    ref = _conv3d(c, d)
    got = dn.chain_dn(c, d, F64)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("c", CASES[:3], ids=lambda c: c.name)
def test_weights_are_the_float64_product_rounded_once(c):
    wp = wc.make_data(c)["wp"]
    g = wc.G
    full = torch.einsum("kt,ia,jb,taboc->ijkoc", g, g, g, wp.double().reshape(3, 3, 3, c.Cout, c.C1 + c.C2)).reshape(16, 4, c.Cout, c.C1 + c.C2)
    assert torch.equal(dn.weights_dn(wp, torch.float32), full.float())
    # position k = 0 / 3 of U' are the outer depth taps of the 2-D weights, untouched
    U = wc.weights(wp, 3, dtype=torch.float32)
    Ud = dn.weights_dn(wp, torch.float32)
    assert torch.equal(Ud[:, 0], U[:, 0]) and torch.equal(Ud[:, 3], U[:, 2])


@pytest.mark.parametrize("mut", dn.MUTATIONS)
def test_wrong_references_are_not_the_convolution(mut):
    c = CASES[1]                                       # n = 2, D = 4: pairs next to a batch boundary
    d = wc.make_data(c)
    ref = _conv3d(c, d)
    err = (dn.chain_dn(c, d, F64, mut=mut) - ref).abs().max().item()
    assert err > 1e-2 * ref.abs().max().item(), (mut, err)


def test_float32_nest_error_is_of_the_existing_forms_size():
    """The float32 restatement in the kernel's order against float64, in units of u sum |x||w|: within the 4x the tests grant the Winograd chain over the
    existing form's own float32 evaluation."""
    c = CASES[2]
    d = wc.make_data(c)
    ref = _conv3d(c, d)
    sig = wc.direct_sums(c, d, True) + d["bias"].abs().double()
    q_new = wc.q_of(dn.chain_dn(c, d, torch.float32), ref, sig)
    outs, _, _ = wc.chain(c, d, torch.float32)
    q_old = wc.q_of(outs["out"], ref, sig)
    assert q_new[0] <= wc.SHARP * q_old[0] and q_new[1] <= wc.SHARP * q_old[1], (q_new, q_old)


def test_flop_meter_counts_four_positions_per_plane_pair():
    from forge_amd import flopmeter as fm
    args = [None, 128, 128, 0, 0, None, 128, 128, 0, 0, None, None, 2, 32, 16, 16, 256, 3]
    assert fm._wino_gemm_dn(args + [None]) * 3 == fm._wino_gemm(args + [0, None]) * 2
    assert fm._wino_gemm_dn(args + [None]) == 2.0 * 16 * (2 * 32 * 256 // 2) * 256 * 4 * 256
