"""The CPU half of the Winograd matrix (tests/wino_cases.py), no GPU:

  * the stage functions, composed, equal F.conv3d / F.conv2d and their autograd (input and weight gradient) in float64 within 1e-12 of the output scale on
    every case's geometry (the 3 x 8 x 8 corner of the cases that are real launches of the step);
  * the coverage rows of the issue are reached and hold what their names say; each case's tile letter and 8-plane / 16-plane form equal the library's own
    host-side rules;
  * every wrong reference of MUTATIONS misses the true one by more than 10x the sharp bound the GPU half applies, with the float32 yardstick standing in
    for the kernel; the yardstick itself stays inside the unconditional bounds on every case.
"""
import pytest
import torch
import torch.nn.functional as F

import wino_cases as wc

REL = 1e-12
NAMES = [c.name for c in wc.CASES]
_MEMO = {}


def small(name):
    """(case, data) cut to the corner where the case is big; data memoised per module run."""
    if name not in _MEMO:
        c = wc.CASE[name]
        _MEMO[name] = wc.corner(c, wc.make_data(c))
    return _MEMO[name]


def torch_conv(c, d):
    """The case's pre-activation rows (no bias) by F.conv3d / F.conv2d in float64, with autograd leaves (x, w)."""
    x1 = d["x1"].double()
    if c.nsum > 1:
        x1 = x1.mean(0)
    x = (x1 if d["x2"] is None else torch.cat([x1, d["x2"].double()], -1)).requires_grad_(True)
    wp = d["wp"].double().requires_grad_(True)
    Co, Ci = wp.shape[1:]
    if c.kd == 3:
        w = wp.reshape(3, 3, 3, Co, Ci).permute(3, 4, 0, 1, 2)
        conv = lambda a, b: F.conv3d(a.permute(0, 4, 1, 2, 3), b, padding=1).permute(0, 2, 3, 4, 1)
    else:                                                       # 2-D: every (n, D) plane is an image of its own
        w = wp.reshape(3, 3, Co, Ci).permute(2, 3, 0, 1)
        conv = lambda a, b: F.conv2d(a.reshape(-1, *a.shape[2:]).permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1)
    return x, wp, w, conv


@pytest.mark.parametrize("name", NAMES)
def test_composed_stages_are_the_convolution_and_its_gradients(name):
    c, d = small(name)
    x, wp, w, conv = torch_conv(c, d)
    M = c.n * c.D * c.H * c.W
    plain = c._replace(epi=0, residual=False, mm2=None)
    bare = dict(d, bias=None, residual=None, mm2=None)
    for half in (False, True):
        got = wc.chain(plain, bare, half=half)[0]["out"]
        if c.dgrad:                                             # the launch is the data gradient of a convolution Cout -> C1 for the upstream gradient x1
            xin = torch.zeros(c.n, c.D, c.H, c.W, c.Cout, dtype=torch.float64, requires_grad=True)
            conv(xin, w).backward(x.detach().reshape(c.n, c.D, c.H, c.W, -1) if c.kd == 3 else x.detach().reshape(c.n * c.D, c.H, c.W, -1))
            ref = xin.grad.reshape(M, c.Cout)
        else:
            ref = conv(x, w).detach().reshape(M, c.Cout)
        assert (got - ref).abs().max().item() < REL * ref.abs().max().item(), (name, half)
        assert (wc.direct_sums(c, d, False) - ref).abs().max().item() < REL * ref.abs().max().item(), name
    if c.wgrad is not None:
        y = conv(x, w)
        y.backward(d["dy"].double().reshape(y.shape))
        ref = d["prior"].double() + wp.grad
        got = wc.wgrad_chain(c, d)
        assert (got - ref).abs().max().item() < REL * ref.abs().max().item(), name
        # the data gradient: the forward chain on dy with the transposed weights
        cd = c._replace(C1=c.Cout, C2=0, Cout=c.C1 + c.C2, dgrad=True, epi=0, residual=False, mm2=None, nsum=1)
        dd = dict(bare, x1=d["dy"].reshape(c.n, c.D, c.H, c.W, c.Cout), x2=None)
        dx = wc.chain(cd, dd)[0]["out"]
        assert (dx - x.grad.reshape(M, -1)).abs().max().item() < REL * x.grad.abs().max().item(), name


def test_matrices_are_shared():
    import test_winograd_math as wm
    assert wm.BT is wc.BT and wm.G is wc.G and wm.AT is wc.AT


def test_magnitude_sums_dominate():
    """mag=True is the same map with absolute coefficients: it bounds the value element by element, stage by stage."""
    c, d = small("wide_a")
    V, Va = wc.input_transform(d["x1"]), wc.input_transform(d["x1"], mag=True)
    assert (V.abs() <= Va * (1 + 1e-15)).all()
    dM, dMa = wc.dy_transform(d["x1"]), wc.dy_transform(d["x1"], mag=True)
    assert (dM.abs() <= dMa * (1 + 1e-15)).all()
    Uw, Ua = wc.weights(d["wp"], 3), wc.weights(d["wp"], 3, mag=True)
    assert (Uw.abs() <= Ua * (1 + 1e-15)).all()
    V2 = torch.cat([V, wc.input_transform(d["x2"])], -1)
    Mm, Ma = wc.point_gemm(V2, Uw, wc.grid_of(c)), wc.point_gemm(V2, Uw, wc.grid_of(c), mag=True)
    assert (Mm.abs() <= Ma * (1 + 1e-12)).all()
    y, ya = wc.inverse_transform(Mm, None, wc.grid_of(c)), wc.inverse_transform(Mm, None, wc.grid_of(c), mag=True)
    assert (y.abs() <= ya * (1 + 1e-12)).all()
    dU = torch.randn(16, 3, 8, 4, dtype=torch.float64)
    z = torch.zeros(27, 8, 4, dtype=torch.float64)
    assert (wc.dw_transform(dU, z).abs() <= wc.dw_transform(dU, z, mag=True) * (1 + 1e-12)).all()


def test_coverage_rows():
    reached = set().union(*(c.rows for c in wc.CASES))
    assert reached == set(wc.ROWS), (set(wc.ROWS) - reached, reached - set(wc.ROWS))
    R = wc.R_of
    for tag, pred in (
            ("step_gates", lambda c: (c.C1, c.C2, c.Cout, R(c), c.epi) == (128, 128, 256, 8192, 2)),
            ("step_state", lambda c: (c.C1, c.C2, c.Cout, R(c), c.epi) == (128, 128, 128, 8192, 3)),
            ("step_conv1", lambda c: (c.C1, c.C2, c.Cout, R(c)) == (64, 0, 128, 8192)),
            ("step_conv1_dgrad", lambda c: (c.C1, c.Cout, R(c), c.dgrad, wc.rule_tile(c)) == (128, 64, 8192, True, "C")),
            ("trunk320", lambda c: R(c) == 320 and c.kd == 1 and c.D == 1 and wc.rule_tile(c) == "D"),
            ("trunk80", lambda c: R(c) == 80 and c.kd == 1 and c.D == 1 and wc.rule_tile(c) == "D"),
            ("many2d_n", lambda c: c.kd == 1 and c.D == 1 and c.n > 8), ("many2d_d", lambda c: c.kd == 1 and c.n == 1 and c.D > 8),
            ("forced_tiles", lambda c: set(c.tiles) == set(wc.ALL_TILES) and c.Cout >= 96), ("ragged_r", lambda c: R(c) % 64 and R(c) % 128),
            ("cout96", lambda c: c.Cout == 96), ("cout160", lambda c: c.Cout == 160), ("cout200", lambda c: c.Cout == 200),
            ("odd_wt", lambda c: (c.W // 2) % 2 == 1), ("straddle", lambda c: (c.H // 2) * (c.W // 2) < 64 and c.D > 1 and c.n > 1 and c.kd == 3),
            ("d1", lambda c: c.D == 1), ("d2", lambda c: c.D == 2), ("d3", lambda c: c.D == 3), ("n_gt1", lambda c: c.n > 1),
            ("hw2", lambda c: c.H == 2 and c.W == 2), ("ld", lambda c: c.ld1 > c.C1 and c.off1), ("bs", lambda c: c.views1 or c.nsum > 1),
            ("ldv_ptv", lambda c: c.vcat and c.C2), ("ld12", lambda c: c.vcat and c.C2), ("pt12", lambda c: c.vcat or c.gviews), ("gemm_bs", lambda c: c.gviews and c.gviews[0] > 1 and c.gviews[1] > 0),
            ("mm2", lambda c: c.mm2), ("mm2_views", lambda c: c.mm2 and c.mm2[0] > 1 and c.mm2[1] > 0), ("ldo", lambda c: c.ldo > c.Cout),
            ("epi0", lambda c: c.epi == 0), ("epi1", lambda c: c.epi == 1), ("epi2", lambda c: c.epi == 2), ("epi3", lambda c: c.epi == 3),
            ("no_bias", lambda c: not c.bias), ("residual0", lambda c: c.epi == 0 and c.residual), ("residual1", lambda c: c.epi == 1 and c.residual),
            ("residual2", lambda c: c.epi == 2 and c.residual), ("residual3", lambda c: c.epi == 3 and c.residual), ("out2", lambda c: c.epi == 3 and c.out2),
            ("out3_2", lambda c: c.epi == 2 and c.out3), ("out3_3", lambda c: c.epi == 3 and c.out3),
            ("plain2", lambda c: c.epi == 2 and not (c.residual or c.out3 or c.mm2)), ("plain3", lambda c: c.epi == 3 and not (c.residual or c.out2 or c.out3 or c.mm2)),
            ("nsum", lambda c: c.nsum > 1), ("input_dy_ld", lambda c: c.dy_ld and c.dy_ld > c.Cout),
            ("wgrad32", lambda c: c.wgrad is not None and c.C2 == 0 and c.C1 <= 32), ("wgrad64", lambda c: c.wgrad is not None and c.C2 == 0 and 32 < c.C1 <= 64),
            ("wgrad128", lambda c: c.wgrad is not None and c.C2 == 0 and c.C1 >= 128), ("wgrad_two", lambda c: c.wgrad is not None and c.C2 and c.C1 % 128 == 0),
            ("wgrad_bs_pt", lambda c: c.wgrad and c.wgrad[0] > 1 and c.wgrad[1] > 0), ("wgrad_kd1", lambda c: c.wgrad is not None and c.kd == 1),
            ("wgrad_kd3", lambda c: c.wgrad is not None and c.kd == 3), ("dw_prior", lambda c: c.wgrad is not None),
            ("weights_kd1", lambda c: c.kd == 1), ("weights_kd3", lambda c: c.kd == 3), ("weights_t", lambda c: c.dgrad or c.wgrad is not None),
            ("half_form", lambda c: wc.rule_tile(c) == "B"), ("rule_tile", lambda c: not c.tiles)):
        tagged = [c for c in wc.CASES if tag in c.rows]
        assert tagged and all(pred(c) for c in tagged), tag
    assert len([c for c in wc.CASES if c.tiles]) >= 2
    assert {wc.rule_tile(c) == "B" for c in wc.CASES if c.gviews} == {False, True}          # the stacked V1 reaches both GEMM entry points
    for e in range(4):
        assert {bool(c.bias) for c in wc.CASES if c.epi == e} == {False, True}, e
    assert {wc.rule_tile(c) for c in wc.CASES} == {"B", "C", "D"}
    for e in range(4):                                          # every epilogue with and without a second addend somewhere
        assert {bool(c.mm2) for c in wc.CASES if c.epi == e} == {False, True}, e
        assert {bool(c.residual) for c in wc.CASES if c.epi == e} == {False, True}, e
    assert any(k % 2 and co % 4 for co, k, _ in wc.WEIGHT_SHAPES) and {kd for _, _, kd in wc.WEIGHT_SHAPES} == {1, 3}
    assert set(m for _, ms in wc.MUTATION_CASES for m in ms) == set(wc.MUTATIONS)


def test_table_is_well_formed():
    """The contract's own requirements (H, W even; channel multiples; 16-byte aligned slices and strides), so that the GPU half launches nothing illegal."""
    for c in wc.CASES:
        assert c.H % 2 == 0 and c.W % 2 == 0 and c.C1 % 32 == 0 and c.C2 % 32 == 0 and c.Cout % 8 == 0 and c.Cout > 16 and c.kd in (1, 3), c.name
        assert c.ld1 % 4 == 0 and c.off1 % 4 == 0 and c.ld1 >= c.off1 + c.C1 and c.ld2 % 4 == 0 and c.off2 % 4 == 0 and c.ld2 >= c.off2 + c.C2, c.name
        assert c.vcat % 4 == 0 and c.ldo % 4 == 0 and (c.ldo == c.Cout // 2 if c.epi == 2 else c.ldo >= c.Cout), c.name
        assert not (c.dgrad and (c.C2 or c.wgrad is not None or c.nsum > 1)), c.name
        assert c.wgrad is None or c.C2 == 0 or c.C1 % 128 == 0, c.name
        assert not (c.gviews and c.vcat), c.name
        assert not c.big or not (c.tiles or c.mm2 or c.views1 or c.gviews or c.vcat or c.nsum > 1 or c.wgrad is not None), c.name
        assert not c.dy_ld or c.dy_ld % 4 == 0, c.name


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_the_library_rules(built_lib, name):
    """The tile letter the table expects is forge_wino_gemm_tile's; the 8-plane form is chosen exactly there; the Winograd path and its weight gradient
    apply where the case says the product takes them (host-only calls)."""
    from forge_amd import convops as co
    c = wc.CASE[name]
    R, Cin = wc.R_of(c), c.C1 + c.C2
    assert co.wino_gemm_tile(R, c.Cout, Cin) == wc.rule_tile(c), name
    assert co.wino_half_applies(R, c.Cout, Cin) == (wc.rule_tile(c) == "B"), name
    for t in wc.ALL_TILES:
        with co.force_plan(tile=t):
            assert co.wino_gemm_tile(R, c.Cout, Cin) == t and not co.wino_half_applies(R, c.Cout, Cin), (name, t)
    if "step_" in " ".join(c.rows):
        assert co.wino_applies(co.TAPS_3x3x3, 1, c.n, c.D, c.H, c.W, c.C1, c.C2, c.Cout), name
    if "wgrad128" in c.rows or "wgrad_two" in c.rows:
        assert co.wino_wgrad_applies(c.n, c.D, c.H, c.W, c.C1, c.C2, c.Cout), name
    if "trunk320" in c.rows:
        assert co.wino_applies(co.TAPS_3x3, 1, c.n, 1, c.H, c.W, c.C1, 0, c.Cout), name


def yard_q(c, d, half=False):
    """Reference, sigma and the float32 yardstick's (q, q_rms) per output of the forward chain."""
    ref, sS, sA = wc.chain(c, d, half=half, want_sigma=True)
    y = wc.chain(c, d, torch.float32, half=half)[0]
    return ref, {k: sS[k] + sA[k] for k in ref}, y, {k: wc.q_of(y[k], ref[k], sS[k] + sA[k]) for k in ref}


@pytest.mark.parametrize("name", NAMES)
def test_float32_yardstick_stays_inside_the_unconditional_bounds(name):
    """Stage by stage, the float32 evaluation in the documented order fed its own float32 inputs meets gamma_k sigma (+ the tail's budget): the inputs
    are well chosen (no cancellation that would leave a bound empty, no overflow) before a GPU is spent."""
    c, d = small(name)
    f32 = torch.float32
    grid = wc.grid_of(c)
    V = wc.input_transform(d["x1"], c.nsum, f32)
    if c.nsum > 1:
        ref, mg = wc.input_transform(d["x1"], c.nsum), wc.input_transform(d["x1"], c.nsum, mag=True)
        assert ((V.double() - ref).abs() <= wc.gamma(c.nsum + 3) * mg).all(), name
    if d["x2"] is not None:
        V = torch.cat([V, wc.input_transform(d["x2"], 1, f32)], -1)
    Uw = wc.weights(d["wp"], c.kd, c.dgrad, f32)
    Mm = wc.point_gemm(V, Uw, grid, f32, "chain")
    ref, mg = wc.point_gemm(V, Uw, grid), wc.point_gemm(V, Uw, grid, mag=True)
    assert ((Mm.double() - ref).abs() <= wc.gamma(wc.k_gemm(c)) * mg).all(), name
    m2 = wc.mm2_view(c, d)
    for form in (Mm, wc.row_combine(Mm)):
        f2 = None if m2 is None else (m2 if form.shape[0] == 16 else wc.row_combine(m2))
        y32 = wc.tail(wc.inverse_transform(form, f2, grid, f32), None, c, d, f32)[0]
        S = wc.inverse_transform(form, f2, grid, mag=True)
        r64, sS, sA = wc.tail(wc.inverse_transform(form, f2, grid), S, c, d)
        for k in r64:
            assert ((y32[k].double() - r64[k]).abs() <= wc.gamma(wc.k_out(c)) * sS[k] + wc.EPI_ULPS * 2 * wc.U * sA[k]).all(), (name, k)
    if c.wgrad is not None:
        dM = wc.dy_transform(d["dy"].reshape(c.n, c.D, c.H, c.W, c.Cout), f32)
        dU = wc.wgrad_points(dM, V, grid, c.kd, f32, "chain")
        assert ((dU.double() - wc.wgrad_points(dM, V, grid, c.kd)).abs() <= wc.gamma(wc.R_of(c) + 2) * wc.wgrad_points(dM, V, grid, c.kd, mag=True)).all(), name
        dw = wc.dw_transform(dU, d["prior"], f32)
        assert ((dw.double() - wc.dw_transform(dU, d["prior"])).abs() <= wc.gamma(wc.K_DW) * wc.dw_transform(dU, d["prior"], mag=True)).all(), name


@pytest.mark.parametrize("name,muts", wc.MUTATION_CASES)
def test_wrong_references_miss_by_ten_times_the_sharp_bound(name, muts):
    c, d = small(name)
    ref, sig, y, qy = yard_q(c, d)
    assert all(qy[k][0] > 0 for k in qy)
    if c.wgrad is not None:
        wref, wsig = wc.wgrad_chain(c, d), wc.wgrad_chain(c, d, mag=True)
        wq = wc.q_of(wc.wgrad_chain(c, d, torch.float32), wref, wsig)
    for mut in muts:
        if mut == "dw_g_swap" or (mut == "pt_transposed" and name == "bw32"):
            wrong = wc.wgrad_chain(c, d, mut=mut)
            miss = ((wrong - wref).abs() / (wc.SHARP * wq[0] * wc.U * wsig)).max().item()
        else:
            wrong = wc.chain(c, d, mut=mut)[0]
            miss = max(((wrong[k] - ref[k]).abs() / (wc.SHARP * qy[k][0] * wc.U * sig[k])).max().item() for k in ref)
        assert miss > 10, (name, mut, miss)
