"""The CPU half of the forge_conv_igemm launch-space matrix (tests/conv_igemm_cases.py):

  * the float64 restatement of the contract equals independent torch code (F.conv3d, strided F.conv2d / F.conv3d, F.conv_transpose3d(k4, s2, p1)
    and F.conv_transpose2d(k6, s2, p2) through convops.convT_phases_merged, the 2D->3D lift as a view, forge_oracle.conv_gru_cell for the GRU
    epilogues 2 + 3 chained) to 1e-12 relative, so the reference is pinned before anything is measured against it;
  * every case reaches the plan it is in the table for (convops.conv_plan under force_plan: a silent fallback to ksplit = 1 fails here, naming
    the case), and the table covers every row it was asked to cover;
  * the sharp bound (4x the float32 yardstick's own q / q_rms) holds for the yardstick trivially and rejects every wrong reference of
    MUTATION_CASES, so that a GPU session is not spent finding out that a mutation was too mild.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_igemm_cases as cc
import forge_oracle as fo

REL = 1e-12


def rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def rows_of(y):
    """NC(D)HW -> channels-last rows [n (D) H W][C]."""
    return y.movedim(1, -1).reshape(-1, y.shape[1])


def cl(x):
    """NCDHW / NCHW -> [n][D][H][W][C] (D = 1 for a 2-D tensor)."""
    if x.dim() == 4:
        x = x[:, :, None]
    return x.permute(0, 2, 3, 4, 1).contiguous()


def data_of(x1, wp, x2=None, **kw):
    d = dict(x1=x1, x2=x2, wp=wp, bias=None, scale=None, shift=None, residual=None, aux_h=None, aux_z=None)
    d.update(kw)
    return d


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def test_restatement_is_conv3d_of_the_channel_concat():
    rn = gen(1)
    x1, x2, w, b = rn(2, 32, 3, 4, 5), rn(2, 64, 3, 4, 5), rn(7, 96, 3, 3, 3), rn(7)
    case = cc.mk("t", "", 2, 3, 4, 5, 32, 7, cc.T27, C2=64)
    wp = w.reshape(7, 96, 27).permute(2, 0, 1).contiguous()
    got = cc.evaluate(case, data_of(cl(x1), wp, cl(x2), bias=b))
    ref = rows_of(F.conv3d(torch.cat([x1, x2], 1), w, b, padding=1))
    assert got["named"].all() and rel(got["out"], ref) < REL
    S = rows_of(F.conv3d(torch.cat([x1, x2], 1).abs(), w.abs(), b.abs(), padding=1))
    assert rel(got["sig_S"]["out"], S) < REL and got["sig_A"]["out"].abs().max().item() == 0


@pytest.mark.parametrize("nd", [2, 3])
def test_restatement_is_the_strided_convolution(nd):
    rn = gen(2)
    if nd == 3:
        x, w = rn(2, 32, 6, 8, 10), rn(5, 32, 3, 3, 3)
        case = cc.mk("t", "", 2, 3, 4, 5, 32, 5, cc.T27, istride=2)
        ref, wp = F.conv3d(x, w, None, stride=2, padding=1), w.reshape(5, 32, 27).permute(2, 0, 1).contiguous()
    else:
        x, w = rn(2, 32, 10, 12), rn(5, 32, 3, 3)
        case = cc.mk("t", "", 2, 1, 5, 6, 32, 5, cc.T9, istride=2)
        ref, wp = F.conv2d(x, w, None, stride=2, padding=1), w.reshape(5, 32, 9).permute(2, 0, 1).contiguous()
    got = cc.evaluate(case, data_of(cl(x), wp))
    assert rel(got["out"], rows_of(ref)) < REL


@pytest.mark.parametrize("nd", [2, 3])
def test_restatement_is_the_transposed_convolution(built_lib, nd):
    """Merged phases (ConvTranspose3d k4 s2 p1: 8 phases, ConvTranspose2d k6 s2 p2: 4) with convops' own phase decomposition of the weight; the eight
    single-phase launches name disjoint rows that together are the merged output; the table's tap lists are convops'."""
    from forge_amd import convops as co
    rn = gen(3)
    if nd == 3:
        x, w, b = rn(2, 32, 3, 4, 5), rn(32, 6, 4, 4, 4), rn(6)
        ref = F.conv_transpose3d(x, w, b, stride=2, padding=1)
        taps, wp = co.convT_phases_merged(w, 1, 3)
        assert [tuple(t) for t in taps] == cc.MERGED8
        case = cc.mk("t", "", 2, 3, 4, 5, 32, 6, taps, ostride=2, phase="merged")
    else:
        x, w, b = rn(2, 32, 5, 7), rn(32, 6, 6, 6), rn(6)
        ref = F.conv_transpose2d(x, w, b, stride=2, padding=2)
        taps, wp = co.convT_phases_merged(w, 2, 2)
        assert [tuple(t) for t in taps] == cc.MERGED4
        case = cc.mk("t", "", 2, 1, 5, 7, 32, 6, taps, ostride=2, phase="merged")
    assert cc.nphase(case) == (8 if nd == 3 else 4)
    got = cc.evaluate(case, data_of(cl(x), wp, bias=b))
    assert got["named"].all() and rel(got["out"], rows_of(ref)) < REL
    if nd == 3:
        seen = torch.zeros_like(got["named"])
        for p, (ph, tp, _) in enumerate(cc.PH3):
            single = cc.evaluate(case._replace(taps=tp, phase=ph), data_of(cl(x), wp[p * 8:(p + 1) * 8], bias=b))
            nm = single["named"]
            assert not (seen & nm).any() and torch.equal(single["out"][nm], got["out"][nm]) and torch.isnan(single["out"][~nm]).all()
            seen |= nm
        assert seen.all()


def test_restatement_of_lift_is_the_view_of_the_2d_output():
    """models/encoder.py:49: y.view(-1, Cl, lift, H, W) of the NCHW activation; the caller orders the weight rows (z, c), c fastest."""
    rn = gen(4)
    lift, Cl, H, W = 4, 24, 5, 6
    Cout = lift * Cl
    x, w, b, sc, sh, r = rn(2, 32, H, W), rn(Cout, 32, 3, 3), rn(Cout), rn(Cout), rn(Cout), rn(2, Cout, H, W)
    vol = F.leaky_relu(F.conv2d(x, w, b, padding=1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) + r, 0.01).view(-1, Cl, lift, H, W)
    perm = torch.tensor([c * lift + z for z in range(lift) for c in range(Cl)])          # GEMM column z Cl + c <- torch channel c lift + z
    case = cc.mk("t", "", 2, 1, H, W, 32, Cout, cc.T9, epi=1, slope=0.01, residual=True, lift=lift)
    wp = w.reshape(Cout, 32, 9).permute(2, 0, 1)[:, perm].contiguous()
    got = cc.evaluate(case, data_of(cl(x), wp, bias=b[perm], scale=sc[perm], shift=sh[perm], residual=rows_of(r)[:, perm].contiguous()))
    ref = vol.permute(0, 2, 3, 4, 1).reshape(-1, Cl)                                       # [n][z][h][w][c]
    assert got["named"].all() and rel(got["out"], ref) < REL


def test_restatement_of_the_gru_epilogues_is_the_oracle_cell():
    rn = gen(5)
    Cx, Ch, D, H, W = 32, 32, 3, 4, 5
    x, h = rn(2, Cx, D, H, W), rn(2, Ch, D, H, W)
    w = {"c.conv_gate.weight": rn(2 * Ch, Cx + Ch, 3, 3, 3) * 0.05, "c.conv_gate.bias": rn(2 * Ch),
         "c.out_gate.weight": rn(Ch, Cx + Ch, 3, 3, 3) * 0.05, "c.out_gate.bias": rn(Ch)}
    ref = fo.conv_gru_cell(x, h, w, "c")
    pack = lambda t: t.reshape(t.shape[0], t.shape[1], 27).permute(2, 0, 1).contiguous()
    gates = cc.mk("g", "", 2, D, H, W, Cx, 2 * Ch, cc.T27, C2=Ch, epi=2, out3=True)
    g = cc.evaluate(gates, data_of(cl(x), pack(w["c.conv_gate.weight"]), cl(h), bias=w["c.conv_gate.bias"], aux_h=rows_of(h)))
    assert rel(g["out3"] * rows_of(h), g["out2"]) < REL
    state = cc.mk("s", "", 2, D, H, W, Cx, Ch, cc.T27, C2=Ch, epi=3, out3=True)
    hr = g["out2"].reshape(2, D, H, W, Ch)
    s = cc.evaluate(state, data_of(cl(x), pack(w["c.out_gate.weight"]), hr, bias=w["c.out_gate.bias"], aux_h=rows_of(h), aux_z=g["out"]))
    assert rel(s["out"], rows_of(ref)) < REL
    # the input-half form of the contract: conv([x, h], W) = residual conv(x, W_x) + conv(h, W_h)
    Wg = w["c.conv_gate.weight"]
    half = cc.mk("h", "", 2, D, H, W, Ch, 2 * Ch, cc.T27, epi=2, residual=True)
    gh = cc.evaluate(half, data_of(cl(h), pack(Wg[:, Cx:].contiguous()), bias=w["c.conv_gate.bias"], aux_h=rows_of(h),
                                   residual=rows_of(F.conv3d(x, Wg[:, :Cx], None, padding=1))))
    assert rel(gh["out"], g["out"]) < REL and rel(gh["out2"], g["out2"]) < REL


def test_epilogue_ulps():
    """EPI_ULPS grants expf / tanhf / the sigmoid 4 ulps each. The ROCm installation carries no ulp table for its device library, so the figure is
    checked against what torch's CPU float32 functions measure against float64 on the epilogues' range (they must stay inside it)."""
    v = torch.linspace(-12, 12, 200001, dtype=torch.float32)
    for f in (torch.exp, torch.tanh, torch.sigmoid):
        got, ref = f(v).double(), f(v.double())
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-300))) - 23)
        assert ((got - ref).abs() / ulp).max().item() <= 4.0, f.__name__


def test_table_is_well_formed():
    """The contract's 16-byte alignment (slice starts, row strides; ldo for split-K), legal lift / GRU / stats combinations, the narrow kernel each
    narrow row is in the table for."""
    for c in cc.CASES:
        assert c.off1 % 4 == 0 and c.off2 % 4 == 0 and c.ld1 % 4 == 0 and c.ld2 % 4 == 0, c.name
        assert c.ld1 >= c.off1 + c.C1 and c.ld2 >= c.off2 + c.C2 and c.ldo >= c.Cout, c.name
        assert c.C1 % cc.kstep(c) == 0 and c.C2 % cc.kstep(c) == 0 and len(c.taps) <= 64, c.name
        assert not c.lift or (c.epi == 1 and c.D == 1 and c.Cout > 64 and c.Cout % c.lift == 0), c.name
        assert c.epi < 2 or c.Cout > 16, c.name
        assert not c.stats or (c.epi == 0 and all(k == 1 for _, k in c.plans) and c.limit is None), c.name
        if c.phase == "merged":
            assert len(c.taps) % cc.nphase(c) == 0, c.name
        form = cc.narrow_form(c)
        for tag, want in (("narrow_lines1", 1), ("narrow_lines2", 2), ("narrow_generic_shuffled", 0), ("narrow_generic_w_le_r", 0), ("narrow_strided", 0)):
            if tag in c.rows:
                assert c.Cout <= 16 and form == want, (c.name, tag, form)
    assert sorted(c.taps for c in cc.CASES if c.name == "n_gen_shuf")[0] != cc.T27 and sorted(cc.T27_SHUFFLED) == sorted(cc.T27)
    assert cc.CASE["n_gen_w2"].W <= 2                                              # W <= R keeps the x-line form off
    M = lambda c: c.n * c.D * c.H * c.W
    assert any(M(c) % 32 and M(c) % 64 and M(c) % 128 and M(c) % 256 for c in cc.CASES if "ragged_m" in c.rows)
    big = cc.CASE["grid2048"]
    assert (M(big) // 64) * (big.Cout // 64) >= 2048 and ("D", 1) in big.plans


def test_coverage_rows():
    """Every row of the coverage table is reached by a case, the values each row names are really there, and every tile / split-K factor appears."""
    reached = set().union(*(c.rows for c in cc.CASES))
    assert reached == set(cc.ROWS), (set(cc.ROWS) - reached, reached - set(cc.ROWS))
    wide = [c for c in cc.CASES if c.Cout > 16]
    for c in wide:
        assert {t for t, k in c.plans if k == 1} == set(cc.ALL_TILES), c.name
    assert {k for c in wide for _, k in c.plans} == {1, 2, 3, 4, 6, 8}
    assert {c.Cout for c in wide} >= {17, 20, 33, 40, 96, 130, 257} and {c.Cout for c in cc.CASES if c.Cout <= 16} >= {1, 3, 8, 16}
    assert {c.W for c in cc.CASES if c.Cout <= 16 and cc.narrow_form(c)} >= {2, 3, 5, 70}
    assert {tuple(c.phase) for c in cc.CASES if "map_phase" in c.rows} == {(a, b, d) for a in (0, 1) for b in (0, 1) for d in (0, 1)}
    assert all(any(k > 1 for _, k in c.plans) for c in cc.CASES if any(r.startswith("splitk") for r in c.rows))
    for res in (False, True):
        assert {c.slope for c in cc.CASES if c.epi == 1 and c.residual == res} >= {1.0, 0.0, 0.01}, res
    assert {c.lift for c in cc.CASES} >= {0, 2, 32}
    assert {len(c.taps) * (c.C1 + c.C2) // 32 for c in wide} >= {1, 2, 3} and any(cc.K_of(c) == 27 * 256 for c in wide)
    k3 = cc.CASE["k3"]
    assert ("D", len(k3.taps) * (k3.C1 // 32)) in k3.plans                          # one K-step per slice
    for tag, pred in (("splitk_residual", lambda c: c.residual), ("splitk_strided", lambda c: c.istride == 2), ("splitk_lift", lambda c: c.lift),
                      ("splitk_phase", lambda c: c.ostride == 2 and c.phase != "merged"), ("splitk_epi0", lambda c: c.epi == 0),
                      ("splitk_epi1", lambda c: c.epi == 1), ("ld1", lambda c: c.ld1 > c.C1 and c.off1), ("ld2", lambda c: c.ld2 > c.C2 and c.off2),
                      ("ldo", lambda c: c.ldo > c.Cout), ("bs1", lambda c: c.views1), ("bs2", lambda c: c.views2),
                      ("chunk_bs1", lambda c: c.limit and c.views1), ("chunk_lift", lambda c: c.limit and c.lift), ("chunk_gru", lambda c: c.limit and c.epi == 2),
                      ("epi2_residual", lambda c: c.epi == 2 and c.residual), ("epi2_out3", lambda c: c.epi == 2 and c.out3),
                      ("epi2_plain", lambda c: c.epi == 2 and not c.residual), ("epi3_plain", lambda c: c.epi == 3 and not (c.out2 or c.residual)),
                      ("epi3_out2", lambda c: c.epi == 3 and c.out2), ("epi3_out3", lambda c: c.epi == 3 and c.out3),
                      ("epi3_residual", lambda c: c.epi == 3 and c.residual), ("epi1_residual", lambda c: c.epi == 1 and c.residual),
                      ("epi1_plain", lambda c: c.epi == 1 and not c.residual), ("lift_residual", lambda c: c.lift and c.residual),
                      ("narrow_epi1_residual", lambda c: c.Cout <= 16 and c.epi == 1 and c.residual), ("stats", lambda c: c.stats),
                      ("map_merged4_narrow", lambda c: c.Cout <= 16 and cc.nphase(c) == 4), ("map_merged4", lambda c: c.Cout > 16 and cc.nphase(c) == 4),
                      ("map_merged8", lambda c: cc.nphase(c) == 8), ("map_s2_2d", lambda c: c.istride == 2 and c.D == 1),
                      ("map_s2_3d", lambda c: c.istride == 2 and c.D > 1)):
        tagged = [c for c in cc.CASES if tag in c.rows]
        assert tagged and all(pred(c) for c in tagged), tag


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_reaches_its_plan(built_lib, monkeypatch, name):
    """convops.conv_plan under force_plan answers the forced (tile, ksplit) for every plan of the case and every batch chunk the launcher makes;
    'N' exactly for Cout <= 16; where the contract forbids split-K (odd Cout, merged phases, GRU epilogues) a forced split is refused."""
    from forge_amd import convops as co
    c = cc.CASE[name]
    Cin, nph = c.C1 + c.C2, cc.nphase(c)
    for k in cc.chunks(c):
        M = k * c.D * c.H * c.W
        free = co.conv_plan(M, c.Cout, Cin, len(c.taps), c.epi, c.ldo, nph)
        assert (free[0] == "N") == (c.Cout <= 16), (name, free)
        for tile, ks in c.plans:
            if tile == "N":
                assert free == ("N", 1), name
                continue
            with co.force_plan(tile, ks):
                assert co.conv_plan(M, c.Cout, Cin, len(c.taps), c.epi, c.ldo, nph) == (tile, ks), (name, tile, ks)
        if c.Cout > 16 and not cc.can_split(c):
            with co.force_plan("D", 2):
                assert co.conv_plan(M, c.Cout, Cin, len(c.taps), c.epi, c.ldo, nph) == ("D", 1), name
        if c.Cout > 16:
            for tile in cc.ALL_TILES:
                assert co.stats_blocks(M, tile) == cc.stats_blocks(M, tile)
    if c.limit is not None:                                         # the launcher's own chunking rule arrives at chunks(c)
        monkeypatch.setattr(co, "MAX_OPERAND_BYTES", cc.operand_limit(c))
        rows = c.in_grid[0] * c.in_grid[1] * c.in_grid[2]
        span = lambda kk, views, ld: ((kk - 1) * rows * (views[0] if views else 1) + rows) * ld * 4
        nc = c.n
        while nc > 1 and (span(nc, c.views1, c.ld1) > co.MAX_OPERAND_BYTES or (c.C2 and span(nc, c.views2, c.ld2) > co.MAX_OPERAND_BYTES)):
            nc = (nc + 1) // 2
        assert [min(nc, c.n - s) for s in range(0, c.n, nc)] == cc.chunks(c) and len(cc.chunks(c)) > 1, name


def test_stats_blocks_past_m():
    """The statistics case leaves whole 32-row blocks past M on every tile (the trailing-tile path of the by-product)."""
    c = cc.CASE["stats"]
    M = c.n * c.D * c.H * c.W
    for tile in cc.ALL_TILES:
        assert cc.stats_blocks(M, tile) * 32 - M >= 32, tile
    ref, _ = cc.stats_from_outputs(torch.ones(M, 3), M, "A")
    assert ref.shape == (12, 2, 3) and ref[8, 0, 0].item() == M - 256 and (ref[9:] == 0).all()


def passes(case, ref, got, qy):
    """The sharp bound: every output's q and q_rms within SHARP x the yardstick's."""
    return all(cc.q_stats(case, ref, got[k], k)[0] <= cc.SHARP * qy[k][0] and cc.q_stats(case, ref, got[k], k)[1] <= cc.SHARP * qy[k][1]
               for k in cc.out_desc(case))


@pytest.mark.parametrize("name,muts", cc.MUTATION_CASES)
def test_sharp_bound_rejects_wrong_references(name, muts):
    """The float32 yardstick passes the sharp bound against the true reference (trivially: 1 <= 4) and the unconditional bound element by element;
    measured against each deliberately wrong reference it fails the sharp bound by a wide margin - q at least 100x the yardstick's."""
    case = cc.CASE[name]
    d = cc.make_data(case)
    ref, y = cc.evaluate(case, d), cc.evaluate(case, d, torch.float32)
    qy = {k: cc.q_stats(case, ref, y[k], k) for k in cc.out_desc(case)}
    assert passes(case, ref, y, qy)
    for k in cc.out_desc(case):
        nm = ref["named"]
        assert ((y[k][nm].double() - ref[k][nm]).abs() <= cc.unconditional_bound(case, ref, k)[nm]).all(), (name, k)
    for mut in muts:
        wrong = cc.evaluate(case, d, mut=mut)
        wrong.update(sig_S=ref["sig_S"], sig_A=ref["sig_A"])
        assert not passes(case, wrong, y, qy), (name, mut)
        assert max(cc.q_stats(case, wrong, y[k], k)[0] / qy[k][0] for k in cc.out_desc(case)) > 100, (name, mut)


def test_yardstick_grains_agree_with_the_reference():
    """The finer-grained float32 yardsticks (per K-step and split-K slice; one fmaf per k) evaluate the same contract: q of the same order."""
    case = cc.CASE["k27x256"]
    d = cc.make_data(case)
    ref = cc.evaluate(case, d)
    for kw in (dict(grain="tap"), dict(grain="kstep"), dict(grain="kstep", ksplit=8), dict(grain="chain"), dict(grain="chain", ksplit=4)):
        q, qrms, _ = cc.q_stats(case, ref, cc.evaluate(case, d, torch.float32, **kw)["out"], "out")
        assert q < 8 and qrms < 2, (kw, q, qrms)
