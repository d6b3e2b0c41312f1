"""CPU: the float64 restatement of the direct convolutions' contract (tests/direct_cases.py) against independent index arithmetic; the case table
against the dispatch it is meant to reach; the wrong readings against the very bounds the GPU test uses, with the float32 yardstick standing in for
the kernel; and the host-side refusals (nothing is launched) - before tests/test_gpu_conv_direct_matrix.py spends a GPU on any of it."""
import ctypes

import pytest

import direct_cases as dc
from forge_amd import _lib

NAMES = [c.name for c in dc.CASES]


@pytest.fixture(scope="module")
def L(built_lib):
    return _lib.lib()


def _close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("name", NAMES)
def test_evaluate_vs_index_arithmetic(name):
    """Shifted slices + autograd against coordinates, bound tests and flat row indices: 1e-12. The data gradient is also the forward of the
    transposed weights over the negated taps."""
    c = dc.CASE[name]
    r = dc.reference(c)
    ex = dc.explicit(c, r["d"])
    assert _close(ex["dw"], r["dw"]), name
    if "fwd" in c.ops:
        assert _close(ex["fwd"], r["fwd"]) and _close(ex["dx"], r["dx"]), name
        d = r["d"]
        adj = dc.linear(d["dout"].double(), d["w"].double().transpose(1, 2), [tuple(-v for v in t) for t in c.taps]).reshape(dc.M_of(c), c.Cin)
        assert _close(adj, r["dx"]), name
    # a tap that cannot reach the grid: no product, an exactly zero slice
    for t, tap in enumerate(c.taps):
        if any(abs(v) >= s for v, s in zip(tap, (c.D, c.H, c.W))):
            assert (r["S_dw"][t] == 0).all() and (r["dw"][t] == 0).all(), (name, tap)


HOLDS = {
    "m_lt_256": lambda c: dc.M_of(c) < 256,
    "m_two_blocks": lambda c: 256 < dc.M_of(c) < 512 and len({c.D, c.H, c.W}) == 3,
    "slope1": lambda c: c.slope == 1.0 and "fwd" in c.ops, "slope0": lambda c: c.slope == 0.0, "slope001": lambda c: c.slope == 0.01,
    "bias": lambda c: c.bias and "fwd" in c.ops, "nobias": lambda c: not c.bias,
    "ld_in": lambda c: c.ldi > c.Cin and c.ldi % 4 == 0, "ld_in16_c8": lambda c: (c.Cin, c.ldi) == (8, 16), "ld_out": lambda c: c.ldo > c.Cout,
    "lds_full": lambda c: len(c.taps) * c.Cin * c.Cout == 64 * 4 * 16 and "fwd" in c.ops,
    "above_grid_cap": lambda c: (dc.M_of(c) + 255) // 256 > dc.GRID_CAP and (c.n, c.D, c.H, c.W, c.Cin, c.Cout, c.tapname) == (2, 66, 64, 64, 4, 1, "T27"),
}
HOLDS.update({"pair_%d_%d" % p: (lambda c, p=p: (c.Cin, c.Cout) == p) for p in dc.PAIRS})
HOLDS.update({k: (lambda c, k=k: c.tapname == k) for k in dc.TAPS})


def test_coverage_rows():
    """Every row of the coverage table is reached by a case for which it holds, and no case claims a row that does not hold for it."""
    assert set(HOLDS) == set(dc.ROWS)
    for c in dc.CASES:
        for r in c.rows:
            assert r in dc.ROWS and HOLDS[r](c), (c.name, r)
    for r in dc.ROWS:
        assert any(r in c.rows for c in dc.CASES), r
    # what the tap lists are meant to be
    assert len(dc.T64A) == 64 == len(set(dc.T64A)) and {v for t in dc.T64A for v in t} == {-2, -1, 0, 1}
    assert len(set(dc.TDUP)) < len(dc.TDUP)
    assert sorted(dc.T27_SHUFFLED) == sorted(dc.T27) and dc.T27_SHUFFLED != dc.T27
    for c in dc.CASES:
        if c.tapname == "TFAR":
            assert any(abs(t[1]) >= c.H for t in c.taps)
        if c.tapname == "TW3":
            assert c.W == 3 and {t[2] for t in c.taps} >= {-2, 2}
        if c.tapname == "T9":
            assert c.D == 1
    big = [c for c in dc.CASES if dc.M_of(c) > 4096]
    assert [c.name for c in big] == ["big"] and big[0].ops == ("wgrad",), "one large case, and only for the weight gradient"
    assert all(c.ops == ("fwd", "dgrad", "wgrad") for c in dc.CASES if c.name != "big")


def test_wg_taps_and_tap_groups_per_pair():
    """wg_taps as the source comment states it, and for every pair a ragged and an exact last tap group (where a group holds more than one tap)."""
    want = {(4, 1): 4, (4, 2): 4, (4, 3): 4, (4, 4): 3, (8, 1): 4, (8, 2): 3, (8, 3): 2, (8, 4): 1, (16, 1): 3, (16, 2): 1, (16, 3): 1, (16, 4): 1}
    assert {p: dc.wg_taps(*p) for p in dc.PAIRS} == want
    for p in dc.PAIRS:
        tg = dc.wg_taps(*p)
        lens = [len(c.taps) for c in dc.CASES if (c.Cin, c.Cout) == p]
        assert len(lens) >= 2, p
        assert any(n % tg == 0 for n in lens), (p, "no exact last group")
        if tg > 1:
            assert any(n % tg != 0 for n in lens), (p, "no ragged last group")


def test_deterministic_slab_cap_cannot_bind():
    """direct_wgrad_grid caps the slab count of the deterministic twin at DET_SLAB_BYTES / (bytes of one slab). The largest slab is 64 taps x 4 x 16
    floats = 16 KiB, so the cap is at least 4096 - always above the grid cap of 2048: the branch is unreachable, not covered."""
    largest = 64 * max(ci * co for ci, co in dc.PAIRS) * 4
    assert largest == 16384 and dc.DET_SLAB_BYTES // largest == 4096 > dc.GRID_CAP


def test_workspace_bytes(L):
    for c in dc.CASES:
        want = dc.wgrad_grid(dc.M_of(c)) * len(c.taps) * c.Cout * c.Cin * 4
        assert L.forge_conv_direct_wgrad_det_ws_bytes(c.n, c.D, c.H, c.W, c.Cin, c.Cout, len(c.taps)) == want, c.name
    assert L.forge_conv_direct_wgrad_det_ws_bytes(1 << 10, 1 << 7, 1 << 7, 1 << 6, 16, 4, 64) == dc.GRID_CAP * 16384     # the cap at the largest slab
    assert L.forge_conv_direct_wgrad_det_ws_bytes(1, 1, 4, 4, 12, 1, 9) == -2 and L.forge_conv_direct_wgrad_det_ws_bytes(1, 1, 4, 4, 8, 1, 65) == -1


@pytest.mark.parametrize("name,muts", dc.MUTATION_CASES)
def test_wrong_readings_violate_the_bounds(name, muts):
    """The float32 yardstick stands in for the kernel: inside every bound against the float64 reference, outside one of them against each wrong reading."""
    c = dc.CASE[name]
    d = dc.reference(c)["d"]
    with dc.yardstick_threads():
        got = {"wgrad": dc.yard_wgrad(c, d)}
        if "fwd" in c.ops:
            got.update(fwd=dc.yard_fwd(c, d), dgrad=dc.yard_dgrad(c, d))
    key = {"fwd": "fwd", "dgrad": "dx", "wgrad": "dw"}

    def violates(ref):
        bad = False
        for op, g in got.items():
            try:
                bad |= bool(dc.violations(c, op, g, None if ref is None else ref[key[op]])[3])
            except AssertionError:          # an element no product reaches is not exact
                bad = True
        return bad
    assert not violates(None), name
    for mut in muts:
        assert violates(dc.explicit(c, d, mut=mut)), (name, mut, "a wrong reading passes: a case is missing")


def test_every_mutation_has_a_case():
    assert {m for _, ms in dc.MUTATION_CASES for m in ms} == set(dc.MUTATIONS)
    assert all(c.muts for c in dc.CASES), "every case names the wrong readings it must reject"


def test_refusals(L):
    """Argument checks run before any launch: the pointers are never dereferenced."""
    f = ctypes.c_void_p(0x1000)
    for what, rc, code in dc.refusal_calls(L, (f, f, f, f, f, f)):
        assert rc == code, (what, rc, L.forge_last_error())
