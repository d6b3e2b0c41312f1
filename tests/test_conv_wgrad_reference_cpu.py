"""CPU: the float64 restatement of forge_conv_wgrad's contract (tests/conv_wgrad_cases.py) against independent torch code, the case table against
the library's own dispatch (forge_conv_wgrad_plan: host-only, nothing is launched), and the wrong references against the bounds - before
tests/test_gpu_conv_wgrad_matrix.py spends a GPU on any of it."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_wgrad_cases as wc
from forge_amd import _lib

SMALL = [c.name for c in wc.CASES if not wc.is_big(c)]


@pytest.fixture(scope="module")
def L(built_lib):
    """The ctypes handle of the library (built on demand by conftest's built_lib)."""
    return _lib.lib()


def pad_slice_reference(c, d):
    """The contract by zero-padding the input and taking strided slices - no index arithmetic shared with wc.gather."""
    dy = d["dy"].double().reshape(-1, c.Cout)
    x = d["x1"].double() if not c.C2 else torch.cat([d["x1"].double(), d["x2"].double()], dim=-1)
    P = 1 + max(abs(v) for t in c.taps for v in t)
    xp = F.pad(x, (0, 0, P, P, P, P, P, P))
    out = torch.empty(len(c.taps), c.Cout, x.shape[-1], dtype=torch.float64)
    for t, (dz, dy_, dx) in enumerate(c.taps):
        s = c.istride
        xs = xp[:, P + dz:P + dz + (c.D - 1) * s + 1:s, P + dy_:P + dy_ + (c.H - 1) * s + 1:s, P + dx:P + dx + (c.W - 1) * s + 1:s]
        assert xs.shape[1:4] == (c.D, c.H, c.W)
        out[t] = dy.t() @ xs.reshape(-1, x.shape[-1])
    return out


@pytest.mark.parametrize("name", SMALL)
def test_evaluate_vs_padded_slices(name):
    c = wc.CASE[name]
    d = wc.make_data(c)
    ref, S = wc.reference(c, d)
    want = pad_slice_reference(c, d)
    assert ref.shape == (len(c.taps), c.Cout, c.C1 + c.C2)
    assert ((ref - want).abs() <= 1e-13 * S + 1e-300).all(), (name, (ref - want).abs().max().item())
    assert (S >= ref.abs() * (1 - 1e-12)).all()


def _autograd_case(kind, nd, k, pad, stride):
    """dw of a torch convolution's weight by autograd, and the same through evaluate(): (want [T][Cout][Cin], got)."""
    g = torch.Generator().manual_seed(k * 10 + stride)
    n, Ci, Co = 2, 8, 12
    sp = (3, 5, 4) if nd == 3 else (1, 5, 6)
    taps = [(kz - pad if nd == 3 else 0, ky - pad, kx - pad) for kz in range(k if nd == 3 else 1) for ky in range(k) for kx in range(k)]
    conv = {("conv", 3): F.conv3d, ("conv", 2): F.conv2d, ("tconv", 3): F.conv_transpose3d, ("tconv", 2): F.conv_transpose2d}[(kind, nd)]
    fine = tuple(s * stride if (nd == 3 or i) else 1 for i, s in enumerate(sp))
    coarse_ch, fine_ch = (Co, Ci) if kind == "conv" else (Ci, Co)           # conv: rows = outputs (coarse), gathered = inputs (fine)
    coarse = torch.randn(n, *sp, coarse_ch, generator=g, dtype=torch.float64)
    fin = torch.randn(n, *fine, fine_ch, generator=g, dtype=torch.float64)
    nchw = lambda t: t.permute(0, 4, 1, 2, 3) if nd == 3 else t[:, 0].permute(0, 3, 1, 2)
    ks = (k,) * nd
    if kind == "conv":          # out = conv(fin); loss = <out, coarse>; d loss / d w [Co][Ci][k..]
        w = torch.zeros(Co, Ci, *ks, dtype=torch.float64, requires_grad=True)
        out = conv(nchw(fin), w, stride=stride, padding=pad)
        assert out.shape[2:] == (sp if nd == 3 else sp[1:])
        (out * nchw(coarse)).sum().backward()
        want = w.grad.reshape(Co, Ci, -1).permute(2, 0, 1)
    else:                        # out = tconv(coarse); loss = <out, fin>; d loss / d w [Ci][Co][k..]; the "dy" rows of the launch are the tconv's INPUT
        w = torch.zeros(Ci, Co, *ks, dtype=torch.float64, requires_grad=True)
        out = conv(nchw(coarse), w, stride=stride, padding=pad)
        assert out.shape[2:] == (fine if nd == 3 else fine[1:])
        (out * nchw(fin)).sum().backward()
        want = w.grad.reshape(Ci, Co, -1).permute(2, 0, 1)
    c = wc.mk("autograd", "", n, sp[0], sp[1], sp[2], fine_ch, coarse_ch, taps, (0, 0, 0, 0), istride=stride, in_grid=fine)
    got = wc.evaluate(c, {"dy": coarse, "x1": fin, "x2": None})
    return want, got


@pytest.mark.parametrize("kind,nd,k,pad,stride", [("conv", 3, 3, 1, 1), ("conv", 2, 3, 1, 1), ("conv", 2, 5, 2, 1), ("conv", 3, 3, 1, 2), ("conv", 2, 6, 2, 2),
                                                  ("conv", 3, 4, 1, 2), ("tconv", 3, 4, 1, 2), ("tconv", 2, 6, 2, 2)])
def test_evaluate_vs_torch_autograd(kind, nd, k, pad, stride):
    """Stride-1 and stride-2 'same' convolutions and the transposed-convolution tap sets (tap = kernel index - padding on the stride-times finer grid)."""
    want, got = _autograd_case(kind, nd, k, pad, stride)
    assert want.abs().max() > 1 and (want - got).abs().max() <= 1e-12 * want.abs().max()


def test_tap_sets_are_the_geometries_they_stand_for():
    assert wc.T64 == [(kz - 1, ky - 1, kx - 1) for kz in range(4) for ky in range(4) for kx in range(4)] and len(set(wc.T64)) == 64
    assert wc.T36 == [(0, ky - 2, kx - 2) for ky in range(6) for kx in range(6)]
    lines = lambda taps: len({t[:2] for t in taps})
    assert (len(wc.T28_9L), lines(wc.T28_9L)) == (28, 9) and (len(wc.T28_10L), lines(wc.T28_10L)) == (28, 10)
    assert (len(wc.T29_9L), lines(wc.T29_9L)) == (29, 9) and (len(wc.T36), lines(wc.T36)) == (36, 6) and (len(wc.T35_7L), lines(wc.T35_7L)) == (35, 7)
    assert max(abs(t[2]) for t in wc.DX3) == 3 and max(abs(t[2]) for t in wc.DX4) == 4
    assert sorted(wc.T9_SHUFFLED) == sorted(wc.T9) and wc.T9_SHUFFLED != wc.T9


@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_case_reaches_its_kernel(L, name):
    """Both paths of every case land on the kernel family and template parameters the table names (the dispatch itself answers)."""
    c = wc.CASE[name]
    for det in (0, 1):
        rc, p = wc.query_plan(c, det)
        assert rc == 0, (name, det, L.forge_last_error())
        assert (p["family"], p["p1"], p["p2"], p["nwv"]) == c.plan, (name, det, wc.plan_text(p))
        assert p["grid"] >= 1 and p["nchunk"] >= 1
    if det:
        C1, C2 = wc.plan_shape(c)
        ta = (ctypes.c_int * (3 * len(c.taps)))(*[v for t in c.taps for v in t])
        nbytes = L.forge_conv_wgrad_det_ws_bytes(C1, C2, c.n, c.D, c.H, c.W, c.istride, *c.in_grid, c.Cout, ta, len(c.taps))
        assert nbytes == p["nchunk"] * len(c.taps) * c.Cout * (C1 + C2) * 4, (name, nbytes, p)      # one slab per chunk / persistent workgroup


def test_coverage_rows(L):
    """Every row of the coverage table is reached by a case that holds what the row's name says."""
    reached = {r for c in wc.CASES for r in c.rows}
    assert reached == set(wc.ROWS), (sorted(set(wc.ROWS) - reached), sorted(reached - set(wc.ROWS)))
    lines = lambda c: len({t[:2] for t in c.taps})
    maxdx = lambda c: max(abs(t[2]) for t in c.taps)
    vol = lambda c: c.in_grid[0] * c.in_grid[1] * c.in_grid[2]

    def outside(c):           # a tap no voxel of the row grid reaches inside the input grid
        S = wc.evaluate(c, wc.make_data(c), mag=True)
        return bool((S.reshape(len(c.taps), -1).max(1).values == 0).any())
    fam = lambda *pl: (lambda c: c.plan == pl)
    holds = {
        "fam_tiles128": fam(1, 128, 1, 4), "fam_tiles64": fam(1, 64, 1, 4), "fam_tiles32": fam(1, 32, 1, 4), "fam_tiles32_tg4": fam(1, 32, 4, 4),
        "fam_tiles64_tg2": fam(1, 64, 2, 4), "fam_small": fam(2, 32, 4, 4), "fam_lines": fam(3, 32, 1, 4), "fam_lines16_c16": fam(4, 16, 1, 4),
        "fam_lines16_c32": fam(4, 32, 1, 8), "fam_lines16_s2": fam(4, 16, 2, 4),
        "ldy": lambda c: c.ldy > c.Cout, "ld1": lambda c: c.ld1 > c.C1, "ld2": lambda c: c.C2 and c.ld2 > c.C2,
        "bs1": lambda c: c.views1 and c.views1[0] > 1 and c.n > 1, "bs2": lambda c: c.views2 and c.views2[0] > 1 and c.n > 1,
        "cout132": lambda c: c.Cout == 132, "cout260": lambda c: c.Cout == 260,
        "cin36": lambda c: (c.C1, c.C2) == (36, 0), "cin68": lambda c: (c.C1, c.C2) == (68, 0), "cin132": lambda c: (c.C1, c.C2) == (132, 0),
        "two_128_36": lambda c: (c.C1, c.C2) == (128, 36), "two_128_132": lambda c: (c.C1, c.C2) == (128, 132), "two_256_64": lambda c: (c.C1, c.C2) == (256, 64),
        "m_lt_16": lambda c: wc.M_of(c) < 16, "m_not_16": lambda c: wc.M_of(c) % 16,
        "chunk_in_row": lambda c: c.plan[0] in (1, 2) and wc.query_plan(c, 0)[1]["nchunk"] >= 2 and wc.query_plan(c, 0)[1]["mchunk"] % c.W,
        "w1": lambda c: c.W == 1, "w2": lambda c: c.W == 2, "w3": lambda c: c.W == 3, "w5": lambda c: c.W == 5,
        "lines9": lambda c: lines(c) == 9 and c.plan[0] in (3, 4), "lines10": lambda c: lines(c) == 10 and len(c.taps) <= 28 and maxdx(c) <= 3,
        "dx3": lambda c: maxdx(c) == 3 and c.plan[0] in (3, 4), "dx4": lambda c: maxdx(c) == 4 and lines(c) <= 9 and len(c.taps) <= 28,
        "taps28": lambda c: len(c.taps) == 28, "taps29": lambda c: len(c.taps) == 29 and lines(c) <= 9 and maxdx(c) <= 3,
        "s2_lines6": lambda c: c.istride == 2 and lines(c) == 6 and len(c.taps) == 36, "s2_lines7": lambda c: c.istride == 2 and lines(c) == 7 and len(c.taps) <= 36,
        "cout16": lambda c: c.Cout == 16 and c.plan[0] == 4, "cout20": lambda c: c.Cout == 20 and c.plan[0] == 3,
        "cin16": lambda c: c.C1 == 16 and c.plan[:2] == (4, 16), "cin20": lambda c: c.C1 == 20 and c.plan[:2] == (4, 32),
        "w_even": lambda c: c.W % 2 == 0 and c.plan[0] == 2, "w_odd": lambda c: c.W % 2 == 1 and c.plan == (1, 32, 1, 4),
        "m131072": lambda c: wc.M_of(c) == 131072 and c.plan[2] > 1, "m_below_131072": lambda c: 131072 - 512 <= wc.M_of(c) < 131072 and c.plan == (1, 32, 1, 4),
        "walk_lines": lambda c: c.plan[0] == 3 and wc.query_plan(c, 0)[1]["grid"] == 512 < c.n * c.D * c.H * ((c.W + 31) // 32),
        "walk_lines16_c16": lambda c: c.plan == (4, 16, 1, 4) and wc.query_plan(c, 0)[1]["grid"] == 1024 < c.n * c.D * c.H * ((c.W + 31) // 32),
        "walk_lines16_c32": lambda c: c.plan == (4, 32, 1, 8) and wc.query_plan(c, 0)[1]["grid"] == 512 < c.n * c.D * c.H * ((c.W + 31) // 32),
        "walk_lines16_s2": lambda c: c.plan == (4, 16, 2, 4) and wc.query_plan(c, 0)[1]["grid"] == 768 < c.n * c.D * c.H * ((c.W + 31) // 32),
        "small_s2": lambda c: c.plan[0] == 2 and c.istride == 2,
        "small_in_grid": lambda c: c.plan[0] == 2 and c.istride == 1 and c.in_grid != (c.D, c.H, c.W),
        "outside_tiles": lambda c: c.plan[0] == 1 and outside(c), "outside_small": lambda c: c.plan[0] == 2 and outside(c),
        "outside_lines": lambda c: c.plan[0] == 3 and outside(c), "outside_lines16": lambda c: c.plan[0] == 4 and outside(c),
        "line_order": lambda c: c.plan[0] in (3, 4) and [t[:2] for t in c.taps] != sorted([t[:2] for t in c.taps], key=[t[:2] for t in c.taps].index),
        "s2_64taps": lambda c: c.istride == 2 and c.taps == wc.T64 and c.plan == (1, 32, 4, 4) and wc.M_of(c) == 131072,
        "launcher_concat": lambda c: c.launcher == "concat" and c.C2 and c.C1 % 128,
        "launcher_chunk_bs1": lambda c: c.launcher == "chunk" and c.n == 3 and c.views1[0] > 1,
    }
    assert set(holds) == set(wc.ROWS)
    for c in wc.CASES:
        for r in c.rows:
            assert holds[r](c), (c.name, r)
    # the boundary pairs land on different sides of the dispatch
    for a, b in wc.BOUNDARIES:
        ca, cb = wc.CASE[wc.BOUNDARY_CASES[a]], wc.CASE[wc.BOUNDARY_CASES[b]]
        assert a in ca.rows and b in cb.rows
        pa, pb = wc.query_plan(ca, 0)[1], wc.query_plan(cb, 0)[1]
        assert (pa["family"], pa["p1"], pa["p2"], pa["nwv"]) != (pb["family"], pb["p1"], pb["p2"], pb["nwv"]), (a, b, wc.plan_text(pa), wc.plan_text(pb))


def test_plan_is_the_dispatch_not_a_copy(L):
    """The chunking the plan reports is the one the workspace query sizes, the deterministic cap lowers the chunk count, and refusals pass through."""
    c = wc.CASE["g_tg4"]
    rc0, p0 = wc.query_plan(c, 0)
    rc1, p1 = wc.query_plan(c, 1)
    assert rc0 == 0 and rc1 == 0 and p0["grid"] == 3 * p0["nchunk"] and p0["mchunk"] % 16 == 0 and p0["mchunk"] * p0["nchunk"] >= wc.M_of(c)
    assert p1["nchunk"] <= p0["nchunk"]
    out = (ctypes.c_longlong * 8)()
    ta = (ctypes.c_int * 3)(0, 0, 0)
    assert L.forge_conv_wgrad_plan(32, 0, 1, 1, 4, 4, 1, 1, 4, 4, 32, ta, 1, 2, out) == -1            # det not 0 / 1
    assert L.forge_conv_wgrad_plan(32, 0, 1, 1, 4, 4, 1, 1, 4, 4, 32, ta, 1, 0, None) == -1           # no plan array
    assert L.forge_conv_wgrad_plan(30, 0, 1, 1, 4, 4, 1, 1, 4, 4, 32, ta, 1, 0, out) == -2            # C1 % 4
    assert L.forge_conv_wgrad_plan(64, 32, 1, 1, 4, 4, 1, 1, 4, 4, 32, ta, 1, 0, out) == -2           # two inputs, C1 % 128


@pytest.mark.parametrize("bad", [128, -129, 200, 1 << 20])
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_tap_components_outside_a_signed_byte_are_refused(L, bad, pos):
    """A tap component the kernels' signed-byte table cannot hold is FORGE_EINVAL - it used to wrap (128 -> -128) into a wrong gradient."""
    tap = [0, 0, 0]
    tap[pos] = bad
    ta = (ctypes.c_int * 6)(0, 1, -1, *tap)
    out = (ctypes.c_longlong * 8)()
    for det in (0, 1):
        assert L.forge_conv_wgrad_plan(32, 0, 1, 4, 4, 4, 1, 4, 4, 4, 64, ta, 2, det, out) == -1
        assert b"outside [-128, 127]" in L.forge_last_error()
    assert L.forge_conv_wgrad_det_ws_bytes(32, 0, 1, 4, 4, 4, 1, 4, 4, 4, 64, ta, 2) == -1
    ok = (ctypes.c_int * 6)(127, -128, 127, -128, 127, -128)
    assert L.forge_conv_wgrad_plan(32, 0, 1, 4, 4, 4, 1, 4, 4, 4, 64, ok, 2, 0, out) == 0
    assert L.forge_conv_wgrad_det_ws_bytes(32, 0, 1, 4, 4, 4, 1, 4, 4, 4, 64, ok, 2) > 0


def _yard(c, d, ref, S, grain, mchunk):
    y = wc.evaluate(c, d, torch.float32, grain=grain, mchunk=mchunk)
    return wc.q_stats(c, ref, S, y)


@pytest.mark.parametrize("name,muts", [(n, m) for n, m in wc.MUTATION_CASES if not wc.is_big(wc.CASE[n])])
def test_bounds_reject_wrong_references(L, name, muts):
    """Each wrong reference, in float64 against the true one, is beyond BOTH bounds on at least one element of every case named for it; the float32
    yardstick itself is inside them."""
    c = wc.CASE[name]
    d = wc.make_data(c)
    ref, S = wc.reference(c, d)
    mchunk = wc.query_plan(c, 0)[1]["mchunk"]
    yq, yr, yu, _ = _yard(c, d, ref, S, 2, mchunk)          # the grain the GPU matrix settled on
    assert 0 < yu <= 1 and yq > 0, (name, yq, yu)
    for mut in muts:
        wrong = wc.evaluate(c, d, mut=mut, mchunk=mchunk)
        err = (wrong - ref).abs()
        beyond = (err > wc.gamma(c) * S) & (err > wc.SHARP * yq * wc.U * S)
        assert beyond.any(), (name, mut, (err / (wc.U * S).clamp_min(1e-300)).max().item(), yq)


def test_every_mutation_is_named_somewhere():
    named = {m for _, ms in wc.MUTATION_CASES for m in ms}
    assert named == set(wc.MUTATIONS), set(wc.MUTATIONS) ^ named
    assert {m for n, ms in wc.MUTATION_CASES if not wc.is_big(wc.CASE[n]) for m in ms} == set(wc.MUTATIONS)       # each is validated here, without a GPU


def test_yardstick_grains_agree_with_the_reference():
    """The float32 yardsticks at every grain (chunk, K-step, MFMA pair, fmaf chain) stay inside the unconditional bound."""
    c = wc.CASE["t_two36"]
    d = wc.make_data(c)
    ref, S = wc.reference(c, d)
    corner = (2, 8, 8)
    for grain in (wc.M_of(c), 16, 2, 1):
        y = wc.evaluate(c, d, torch.float32, grain=grain, mchunk=112, corner=corner)
        q, qr, ub, _ = wc.q_stats(c, ref[:2, :8, :8], S[:2, :8, :8], y)
        assert 0 < q and ub <= 1, (grain, q, ub)
