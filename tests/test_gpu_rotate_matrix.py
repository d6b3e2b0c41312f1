"""GPU (-m gpu): the pose warp over its dispatch space - traversal order x channel groups per thread x transform x mode / slot - against the float64
restatement of its contract (tests/rotate_cases.py), through the C entry points.

Per case:
  forward        forge_rotate_fwd (forge_rotate_fwd_slots where the case has slots) into a buffer filled with a NaN of a known bit pattern: every element
                 is written and finite, one element before and past the buffer still holds the pattern; inside the forward bound; mode-0 volumes
                 are bitwise copies; a volume thrown out of the grid is exactly zero.
  gather         forge_rotate_bwd[_slots] with dxf == NULL: dvox written over the pattern, inside 1e-4 of its maximum; mode-0: the bitwise gradient.
  affine         dvox == NULL (pose refinement). Atomic entry onto zeros; deterministic entry over the pattern (accumulate = 0), a repeat bitwise
                 identical, accumulate = 1 bitwise fl(prior + first); its workspace is fully written and the float past it keeps the pattern.
                 Mode-0 rows are exact zeros. Where the case clears the lattice (rotate_cases.Case.dxf, asserted on the CPU) each transform row is
                 inside SHARP x the float32 CPU yardstick (floor 64 u, cap 2e-3; the atomic entry + 1e-5).
Every line "rotate_matrix ..." printed under -s is a row of the table in the case notes.
"""
import pytest
import torch

import rotate_cases as rc
from forge_amd import _lib
from rotate_cases import finish, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


_REF = {}


def reference(c):
    """(data, float64 (out, dvox, dxf), float32 yardstick's dxf row errors), computed once per case."""
    if c.name not in _REF:
        d = rc.make_data(c)
        want = rc.gradients(c, d)
        with rc.yardstick_threads():
            yard = rc.row_errors(rc.gradients(c, d, torch.float32)[2], want[2])
        _REF[c.name] = (d, want, yard)
    return _REF[c.name]


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_case(dev, name):
    c = rc.CASE[name]
    d, (out_ref, dvox_ref, dxf_ref), yard = reference(c)
    L = _lib.lib()
    n, dims = len(c.views), (len(c.views), c.C, c.D, c.H, c.W)
    vox, dout, xf, mode = d["vox"].to(dev), d["dout"].to(dev), d["xf"].to(dev), d["mode"].to(dev)
    slot = None if d["slot"] is None else d["slot"].to(dev)
    sl = () if slot is None else (_lib.ptr(slot),)
    st = _lib.current_stream()
    shape = tuple(d["vox"].shape)
    dst = list(range(n)) if c.slot is None else list(c.slot)

    # ---- forward
    raw, out = guarded(shape, dev)
    fwd = L.forge_rotate_fwd if slot is None else L.forge_rotate_fwd_slots
    _lib.check(fwd(_lib.ptr(vox), _lib.ptr(xf), _lib.ptr(mode), *sl, _lib.ptr(out), *dims, st), "forge_rotate_fwd")
    got = finish(raw, out, (name, "forward"))
    e_fwd = (got.double() - out_ref).abs().max().item()
    assert e_fwd <= rc.fwd_bound(c, out_ref), (name, "forward", e_fwd, rc.fwd_bound(c, out_ref))
    for i, k in enumerate(c.views):
        if k == "copy":
            assert torch.equal(got[dst[i]], d["vox"][i]), (name, "a mode-0 volume is not a bitwise copy")
        if k == "out":
            assert (got[dst[i]] == 0).all(), (name, "a volume thrown out of the grid is not exactly zero")

    # ---- volume gradient alone (dxf == NULL)
    raw, dvox = guarded(shape, dev)
    bwd = L.forge_rotate_bwd if slot is None else L.forge_rotate_bwd_slots
    _lib.check(bwd(_lib.ptr(dout), _lib.ptr(vox), _lib.ptr(xf), _lib.ptr(mode), *sl, _lib.ptr(dvox), None, *dims, st), "forge_rotate_bwd")
    got = finish(raw, dvox, (name, "gather"))
    e_dv = (got.double() - dvox_ref).abs().max().item()
    assert e_dv <= rc.dvox_bound(c, dvox_ref), (name, "dvox", e_dv, rc.dvox_bound(c, dvox_ref))
    for i, k in enumerate(c.views):
        if k == "copy":
            assert torch.equal(got[i], d["dout"][dst[i]]), (name, "the gradient of a mode-0 volume is not the bitwise upstream gradient")
        if k == "out":
            assert (got[i] == 0).all(), (name, "dvox of a volume thrown out of the grid is not exactly zero")

    # ---- affine gradient alone (dvox == NULL): atomic onto zeros
    raw, dxf = guarded((n, 12), dev, fill=0.0)
    _lib.check(bwd(_lib.ptr(dout), _lib.ptr(vox), _lib.ptr(xf), _lib.ptr(mode), *sl, None, _lib.ptr(dxf), *dims, st), "forge_rotate_bwd")
    dxf_a = finish(raw, dxf, (name, "affine"))

    # ---- deterministic: over the pattern, repeated, onto a prior
    det = L.forge_rotate_bwd_det if slot is None else L.forge_rotate_bwd_slots_det
    nbytes = (L.forge_rotate_bwd_det_ws_bytes if slot is None else L.forge_rotate_bwd_slots_det_ws_bytes)(*dims)
    assert nbytes == n * rc.affine_blocks(c) * 48
    runs = []
    for fill, acc in ((None, 0), (None, 0), (d["prior"], 1)):
        raw_ws, ws = guarded((nbytes // 4,), dev)
        raw, dxf = guarded((n, 12), dev, fill=fill)
        _lib.check(det(_lib.ptr(dout), _lib.ptr(vox), _lib.ptr(xf), _lib.ptr(mode), *sl, None, _lib.ptr(dxf), *dims, acc, _lib.ptr(ws), nbytes, st),
                   "forge_rotate_bwd_det")
        runs.append(finish(raw, dxf, (name, "affine det", acc)))
        finish(raw_ws, ws, (name, "affine det workspace"))
    dxf_d = runs[0]
    assert torch.equal(runs[0], runs[1]), (name, "the deterministic affine gradient differs between two runs")
    assert torch.equal(runs[2], d["prior"] + runs[0]), (name, "accumulate = 1 is not fl(prior + gradient)")
    for g in (dxf_a, dxf_d):
        assert (g[d["mode"] == 0] == 0).all(), (name, "dxf of a mode-0 view is not zero")
        for i, k in enumerate(c.views):
            if k == "out":
                assert (g[i] == 0).all(), (name, "dxf of a volume thrown out of the grid is not exactly zero")
    line = "rotate_matrix %-8s fwd %.2e (bound %.2e) dvox %.2e (bound %.2e)" % (name, e_fwd, rc.fwd_bound(c, out_ref), e_dv, rc.dvox_bound(c, dvox_ref))
    if c.dxf:
        ea, ed = rc.row_errors(dxf_a, dxf_ref), rc.row_errors(dxf_d, dxf_ref)
        ba, bd = rc.dxf_bounds(yard, rc.ATOMIC_NOISE), rc.dxf_bounds(yard)
        ratio = lambda e: max(x / max(y, rc.DXF_FLOOR / rc.SHARP) for x, y in zip(e, yard))
        print(line + " dxf rows: yardstick %s atomic %s det %s; worst ratio to the yardstick: atomic %.2f det %.2f" % (
            " ".join("%.1e" % y for y in yard), " ".join("%.1e" % x for x in ea), " ".join("%.1e" % x for x in ed), ratio(ea), ratio(ed)))
        assert all(x <= b for x, b in zip(ea, ba)), (name, "atomic dxf", ea, ba)
        assert all(x <= b for x, b in zip(ed, bd)), (name, "deterministic dxf", ed, bd)
    else:
        print(line + " dxf not compared (samples on the lattice)")
