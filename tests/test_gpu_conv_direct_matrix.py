"""GPU (-m gpu): the direct convolutions over their dispatch space - 12 (Cin, Cout) instantiations x forward / data gradient / atomic and deterministic
weight gradient x tap lists x row strides x activation - against the float64 restatement of their contract (tests/direct_cases.py), through the C
entry points.

Per case:
  poison         gap columns [C, ld) and guard rows of every input are NaN: one element read too many into a sum fails loudly. Every output lives
                 inside an allocation filled with a NaN of a known bit pattern: afterwards the gap columns of the output and the floats before and
                 past it still hold the pattern, and every named element is finite.
  fwd, dgrad     inside the unconditional bound and SHARP x the float32 CPU yardstick (direct_cases' docstring).
  wgrad          atomic onto zeros, again, and onto a prior; deterministic over the pattern (accumulate = 0), a repeat bitwise identical,
                 accumulate = 1 bitwise fl(prior + first), the workspace exactly forge_conv_direct_wgrad_det_ws_bytes long inside a guarded
                 allocation. Two atomic runs, and the atomic and the deterministic entry, agree within twice the sharp bound. The dw slice of a tap
                 wholly outside the grid is exactly zero.
test_refusals_leave_the_output_alone runs every refusal on real buffers: the error code, and the pattern of the output intact.
Every line "conv_direct_matrix ..." printed under -s is a row of MEASURED in direct_cases.py.
"""
import ctypes

import pytest
import torch

import direct_cases as dc
from direct_cases import finish, finish_rows, guarded, guarded_rows
from forge_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def within_twice_sharp(c, a, b):
    S = dc.reference(c)["S_dw"]
    e = (a.double() - b.double()).abs()
    assert (e[S == 0] == 0).all(), (c.name, "elements no product reaches differ between two paths")
    return (e / (2 * dc.SHARP * dc.yardstick(c)["wgrad"][0] * dc.U * S).masked_fill(S == 0, 1.0)).max().item()


@pytest.mark.parametrize("name", [c.name for c in dc.CASES])
def test_case(dev, name):
    c = dc.CASE[name]
    r, y = dc.reference(c), dc.yardstick(c)
    d = r["d"]
    L, st = _lib.lib(), _lib.current_stream()
    M, T = dc.M_of(c), len(c.taps)
    taps = (ctypes.c_int * (3 * T))(*[v for t in c.taps for v in t])
    dims = (c.n, c.D, c.H, c.W, c.Cin, c.Cout, taps, T)
    w = d["w"].to(dev)
    x = guarded_rows(d["x"].reshape(M, c.Cin), c.ldi, dev)
    dy = guarded_rows(d["dout"].reshape(M, c.Cout), c.ldo, dev)
    fails, cols = [], []

    def record(op, what, got, prior=None):
        q, qr, ub, f = dc.violations(c, op, got, prior=prior)
        cols.append("%s q %.2f q_rms %.3f (%.2fx %.2fx) uncond %.1e" % (what, q, qr, q / y[op][0], qr / y[op][1], ub))
        fails.extend((name, what, m) for m in f)

    if "fwd" in c.ops:
        bias = None if d["bias"] is None else d["bias"].to(dev)
        raw, out = guarded((M, c.ldo), dev)
        _lib.check(L.forge_conv_direct_fwd(_lib.ptr(x), c.ldi, _lib.ptr(w), _lib.ptr(bias), c.slope, _lib.ptr(out), c.ldo, *dims, st), "forge_conv_direct_fwd")
        record("fwd", "fwd", finish_rows(raw, out, c.Cout, (name, "fwd")))
    if "dgrad" in c.ops:
        raw, dx = guarded((M, c.ldi), dev)
        _lib.check(L.forge_conv_direct_dgrad(_lib.ptr(dy), c.ldo, _lib.ptr(w), _lib.ptr(dx), c.ldi, *dims, st), "forge_conv_direct_dgrad")
        record("dgrad", "dgrad", finish_rows(raw, dx, c.Cin, (name, "dgrad")))

    # ---- atomic weight gradient: onto zeros, again, onto a prior
    shape = (T, c.Cout, c.Cin)
    atom = []
    for fill in (0.0, 0.0, d["prior"]):
        raw, dw = guarded(shape, dev, fill=fill)
        _lib.check(L.forge_conv_direct_wgrad(_lib.ptr(dy), c.ldo, _lib.ptr(x), c.ldi, _lib.ptr(dw), *dims, st), "forge_conv_direct_wgrad")
        atom.append(finish(raw, dw, (name, "wgrad")))
    record("wgrad", "wgrad", atom[0])
    record("wgrad", "wgrad#2", atom[1])
    record("wgrad", "wgrad+p", atom[2], prior=d["prior"])
    # ---- deterministic: over the pattern, repeated, onto a prior
    nbytes = L.forge_conv_direct_wgrad_det_ws_bytes(*dims[:6], T)
    assert nbytes == dc.wgrad_grid(M) * T * c.Cout * c.Cin * 4
    det = []
    for fill, acc in ((None, 0), (None, 0), (d["prior"], 1)):
        raw_ws, ws = guarded((nbytes // 4,), dev)
        raw, dw = guarded(shape, dev, fill=fill)
        _lib.check(L.forge_conv_direct_wgrad_det(_lib.ptr(dy), c.ldo, _lib.ptr(x), c.ldi, _lib.ptr(dw), *dims, acc, _lib.ptr(ws), nbytes, st),
                   "forge_conv_direct_wgrad_det")
        det.append(finish(raw, dw, (name, "wgrad det", acc)))
        finish(raw_ws, ws, (name, "wgrad det workspace"))
    record("wgrad", "det", det[0])
    assert torch.equal(det[0].view(torch.int32), det[1].view(torch.int32)), (name, "two deterministic runs differ")
    assert torch.equal(det[2].view(torch.int32), (d["prior"] + det[0]).view(torch.int32)), (name, "accumulate = 1 is not fl(prior + first)")
    for t, tap in enumerate(c.taps):
        if any(abs(v) >= s for v, s in zip(tap, (c.D, c.H, c.W))):
            assert (atom[0][t] == 0).all() and (det[0][t] == 0).all(), (name, tap, "a tap wholly outside the grid: dw slice not exactly zero")
    r_aa, r_da = within_twice_sharp(c, atom[0], atom[1]), within_twice_sharp(c, det[0], atom[0])
    print("conv_direct_matrix %-10s M %6d | %s | atomic vs atomic %.2f det vs atomic %.2f of 2x sharp" % (name, M, " | ".join(cols), r_aa, r_da))
    assert not fails, fails
    assert r_aa <= 1 and r_da <= 1, (name, r_aa, r_da)


def test_refusals_leave_the_output_alone(dev):
    """Every refusal on real buffers, each large enough for the launch the arguments describe: the error code, and not one float of the outputs touched."""
    L = _lib.lib()
    buf = lambda: torch.zeros(1 << 12, dtype=torch.float32, device=dev)
    pin, pw, pb = buf(), buf(), buf()
    raw, out = guarded((1 << 12,), dev)
    raw_x, px = guarded((1 << 12,), dev, fill=0.0)                 # the weight gradient's input and the data gradient's output
    raw_ws, ws = guarded((1 << 12,), dev)
    with torch.cuda.device(dev):
        for what, rc, code in dc.refusal_calls(L, tuple(_lib.ptr(t) for t in (pin, pw, pb, out, px, ws))):
            assert rc == code, (what, rc, L.forge_last_error())
        torch.cuda.synchronize()
    for r in (raw, raw_ws):
        assert (r.cpu() == dc.CANARY).all(), "a refused call wrote to its output"
    assert (finish(raw_x, px, "refusals") == 0).all(), "a refused data gradient wrote to dx"
