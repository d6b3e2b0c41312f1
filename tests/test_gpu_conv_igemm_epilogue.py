"""GPU (-m gpu): the two epilogues of the wide implicit-GEMM kernel store the same bits.

A launch with identity output rows takes the direct-store epilogue (buffer stores with one 32-bit offset per lane, the residual read ahead of the
stores); STATE.conv_fast_epilogue = False (FORGE_CONV_FAST_EPILOGUE=0) sends every launch through the row-table epilogue.

  test_direct_equals_general   bitwise equality (whole buffers, guard rows and neighbouring channels included) over rows x columns x taps x epilogue
                               variants x output / residual layouts x every tile the plan override can force. The (rows, columns, tile) product is
                               walked in full with every layout; Cin and the epilogue variant cycle along it (7 variants against 5 layouts and 5 tiles:
                               every pair meets several times).
  test_general_only_launches   launches that must stay on the row-table epilogue give the same bits with the switch on and off.
  test_float64_reference       both epilogues against float64 on the 3x3 case, at the matrix's own bounds (conv_igemm_cases). The reference is not a
                               torch.nn.functional.conv2d call but conv_igemm_cases.evaluate, the float64 restatement of the contract (gather + matmul per
                               tap, written from include/forge_hip.h, pinned to independent torch code by tests/test_conv_igemm_reference_cpu.py): it is
                               the reference those bounds (error scales sigma_S / sigma_A, the chain-grain yardstick) are defined against, and it covers
                               the affine epilogue with its residual, which conv2d alone does not. Launch, reference and measure are imported from
                               tests/test_gpu_conv_igemm_matrix.py so that the canaries and the bounds are that file's, not a copy.

A residual with a row stride other than the output's (ldr != ldo) cannot be asked for through forge_conv_igemm: its contract reads the residual at
[rows][ldo] (ldr = Cout only with a lift or a GRU epilogue, which keep the row-table epilogue). That layout is covered by the selection rule alone
(tests/test_conv_igemm_epilogue_cpu.py).
"""
import itertools

import pytest
import torch

import conv_igemm_cases as cc
from forge_amd import _lib, convops as co
from test_gpu_conv_igemm_matrix import Launch, measure, reference

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 70, 200)                  # below, at and just past one and two 64 / 128-row tiles
COUTS = (32, 40, 64, 130, 256)               # ragged last column tile, below and above one 128 tile
CINS = (32, 64)
# (epilogue, slope, bias)
VARIANTS = ((0, 1.0, True), (0, 1.0, False), (1, 0.0, True), (1, 0.01, True), (1, 1.0, True), (1, 0.0, False), (1, 0.01, False))
LAYOUTS = ("plain", "residual", "residual_slice", "in_place", "slice")
PAD = 8                                      # channels of the wider tensor on either side of a channel slice


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


class switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = co.STATE.conv_fast_epilogue
        co.STATE.conv_fast_epilogue = self.on

    def __exit__(self, *exc):
        co.STATE.conv_fast_epilogue = self.prev
        return False


_DATA = {}


def operands(dev, grid, taps, Cin, Cout):
    key = (grid, len(taps), Cin, Cout)
    if key not in _DATA:
        g = torch.Generator().manual_seed(1000 * Cout + 10 * Cin + len(taps) + grid[3])
        n, D, H, W = grid
        M = n * D * H * W
        rn = lambda *s: torch.randn(*s, generator=g)
        _DATA[key] = tuple(t.to(dev) for t in (rn(M, Cin), rn(len(taps), Cout, Cin) / (len(taps) * Cin) ** 0.5, rn(Cout), torch.rand(Cout, generator=g) + 0.5,
                                               rn(Cout), rn(M, Cout)))
    return _DATA[key]


def canary_buffer(dev, M, ld):
    """Three guard rows, M rows of ld floats, three guard rows: all canaries. Returns (flat int32 buffer, float32 view of the M rows)."""
    G = 3 * ld
    buf = torch.full((2 * G + M * ld,), cc.CANARY, dtype=torch.int32, device=dev)
    return buf, buf.view(torch.float32)[G:G + M * ld].view(M, ld)


def launch(dev, grid, taps, Cin, Cout, tile, variant, layout, fast):
    """One conv_igemm under force_plan(tile, 1) with the switch at `fast`. Returns (the output's whole buffer as int32 on the CPU, mask of the elements
    the launch names). In place: the output rows hold the residual before the launch when fast; the general run reads it from a copy."""
    epi, slope, with_bias = variant
    n, D, H, W = grid
    M = n * D * H * W
    x, w, bias, scale, shift, res = operands(dev, grid, taps, Cin, Cout)
    sliced = layout in ("residual_slice", "slice") or (layout == "in_place" and Cout % 3 == 1)
    ld, off = (Cout + 2 * PAD, PAD) if sliced else (Cout, 0)
    buf, rows = canary_buffer(dev, M, ld)
    out = rows[:, off:off + Cout]
    residual = None
    if epi == 1 and layout in ("residual", "residual_slice"):
        _, rrows = canary_buffer(dev, M, ld)
        residual = rrows[:, off:off + Cout]
        residual.copy_(res)
    elif epi == 1 and layout == "in_place":
        if fast:
            out.copy_(res)
            residual = out
        else:
            _, rrows = canary_buffer(dev, M, ld)
            residual = rrows[:, off:off + Cout]
            residual.copy_(res)
    assert co.conv_epilogue_is_direct(M, Cout, ld, ld, residual is not None, epilogue=epi), "the launch under test would not take the direct-store epilogue"
    with switch(fast), co.force_plan(tile, 1):
        co.conv_igemm(x, Cin, Cin, None, 0, 0, w, bias if with_bias else None, scale if epi else None, shift if epi else None, slope, residual, None, None,
                      out, None, grid, (D, H, W), Cout, ld, taps, epilogue=epi)
    mask = torch.zeros(M, ld, dtype=torch.bool)
    mask[:, off:off + Cout] = True
    full = torch.zeros(buf.numel(), dtype=torch.bool)
    full[3 * ld:3 * ld + M * ld] = mask.reshape(-1)
    return buf.cpu(), full


def _shapes():
    for M, Cout in itertools.product(ROWS, COUTS):
        yield (1, 1, 1, M), cc.T1, Cout
    for Cout in (40, 130):
        yield (2, 1, 6, 7), cc.T9, Cout            # the nine taps of a 2-D 3x3 on a 6 x 7 grid, n = 2: M = 84


def test_direct_equals_general(dev):
    k, seen = 0, set()
    for (grid, taps, Cout), tile in itertools.product(_shapes(), cc.ALL_TILES):
        for layout in LAYOUTS:
            Cin, variant = CINS[k % 2], VARIANTS[k % len(VARIANTS)]
            k += 1
            seen.add((variant, layout))
            seen.add((variant, tile))
            what = (grid, len(taps), Cin, Cout, tile, variant, layout)
            got, named = launch(dev, grid, taps, Cin, Cout, tile, variant, layout, True)
            want, _ = launch(dev, grid, taps, Cin, Cout, tile, variant, layout, False)
            assert (want[~named] == cc.CANARY).all(), (what, "the general epilogue wrote an element the launch does not name")
            assert (got[~named] == cc.CANARY).all(), (what, "the direct-store epilogue wrote an element the launch does not name",
                                                      int((got[~named] != cc.CANARY).sum()))
            assert torch.isfinite(got.view(torch.float32)[named]).all(), (what, "a named element is not finite")
            assert torch.equal(got, want), (what, "the two epilogues differ", int((got != want).sum()))
    assert len(seen) == len(VARIANTS) * (len(LAYOUTS) + len(cc.ALL_TILES)), "the cycle does not pair every variant with every layout and tile"


# (case of the matrix, plan, the reason it keeps the row-table epilogue)
GENERAL_ONLY = [("phase010", ("D", 1), "ostride = 2 with a phase"), ("merged8", ("B", 1), "merged phases"), ("lift2", ("D", 1), "lift > 0"),
                ("k27x256", ("D", 2), "forced ksplit = 2"), ("stats", ("D", 1), "want_stats")]


@pytest.mark.parametrize("name,plan,why", GENERAL_ONLY)
def test_general_only_launches(dev, name, plan, why):
    case = cc.CASE[name]
    M = case.n * case.D * case.H * case.W
    same = tuple(case.out_grid) == (case.D, case.H, case.W)
    assert not co.conv_epilogue_is_direct(M, case.Cout, case.ldo, case.Cout if case.lift else case.ldo, case.residual, case.ostride, same, cc.nphase(case),
                                          case.lift, plan[1], case.stats, case.epi), why
    L = Launch(case, dev)
    runs = []
    for on in (True, False):
        stats = None
        if case.stats:
            stats = torch.zeros(cc.stats_blocks(M, plan[0]) * 2 * case.Cout, dtype=torch.float64, device=dev)
        with switch(on):
            got = L.launch(plan[0], plan[1], stats=stats)
        runs.append((got, None if stats is None else stats.cpu()))
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k].view(torch.int32), runs[1][0][k].view(torch.int32)), (name, k, why)
    if case.stats:
        assert torch.equal(runs[0][1], runs[1][1]), (name, "statistics", why)


CASE_3X3 = cc.mk("epilogue3x3", "epi1_residual", 2, 1, 6, 7, 32, 40, cc.T9, epi=1, slope=0.01, residual=True)


@pytest.mark.parametrize("fast", [True, False])
def test_float64_reference(dev, fast):
    """So that both epilogues are not wrong together: the 3x3 case against float64, at the bounds of test_gpu_conv_igemm_matrix (the unconditional
    bound and SHARP x the chain-grain yardstick, both from conv_igemm_cases), canaries included."""
    case = CASE_3X3
    _, ref = reference(case)
    L = Launch(case, dev)
    fails = []
    for tile in cc.ALL_TILES:
        assert co.conv_epilogue_is_direct(84, case.Cout, case.ldo, case.ldo, True, epilogue=1)
        with switch(fast):
            got = L.launch(tile, 1)
        fails += measure(case, ref, got, tile, 1)[1]
    assert not fails, fails
