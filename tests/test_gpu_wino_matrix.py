"""GPU (-m gpu): the Winograd entry points forge_wino_* stage by stage against the float64 restatement of their contract (tests/wino_cases.py), through raw
ctypes calls (the strides the wrappers never pass: ld > C, ldv > C, ptv, ld1 / ld2 > C, pt1 / pt2, bs, ldo > Cout) - in the shape of
test_gpu_conv_igemm_matrix.py.

Per case, launch by launch:
  canaries       every output sits inside a larger allocation filled with the NaN pattern CANARY (guard rows, padding columns, the gap between point
                 planes); afterwards every element the contract does not name still holds it and every named one is finite. Operand padding (columns outside
                 the fed slice, other views' rows, guard rows) is NaN: the GEMM reads V from the canary-filled buffer the input transform wrote.
  exact stages   forge_wino_input (nsum = 1), forge_wino_dy, both outputs of forge_wino_input_dy: torch.equal with the float32 CPU evaluation in the
                 documented order; forge_wino_weights: torch.equal with the float64 product rounded once. nsum > 1: gamma_(nsum + 3).
  unconditional  every other stage, fed the float32 inputs it actually got: |got - ref| <= gamma_k sigma (+ EPI_ULPS 2 u sigma_A in the tails), k as counted
                 in wino_cases' docstring.
  sharp          the whole chain (forward / data gradient through both output kernels, weight gradient) against float64: q = max |got - ref| / (u sigma),
                 q_rms, no element excluded, within SHARP = 4x the float32 CPU yardstick's (documented order, one fused multiply-add per k; cases that are
                 real launches of the step: on a 3 x 8 x 8 corner). The direct kernel's q on the same case is printed beside it, not asserted.
  tiles          forge_wino_gemm under every forced tile and the rule's own: each within the GEMM stage's sharp bound, every pair within twice that of each
                 other. Two cases feed the GEMMs V1 as a view of a [n][views] stack (bs1, pt1), one of them through forge_wino_gemm_half.
  repeat         every launch once more, bitwise - except the atomic forge_wino_wgrad; forge_wino_wgrad_det with accumulate 0 and 1.
test_bounds_reject_wrong_references: the correct kernels against each wrong reference of MUTATIONS. test_refusals: no launch.
Every line "wino_matrix ..." printed under -s is a row of profiles/r11_wino_matrix.txt.
"""
import ctypes
import time

import pytest
import torch

import conv_igemm_cases as cc
import wino_cases as wc
from forge_amd import _lib, convops as co

pytestmark = pytest.mark.gpu
F32, NAN = torch.float32, float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def emit(line):
    print("wino_matrix " + line)


class OutBuf:
    """`planes` planes of `rows` rows of ld floats, pt floats apart, of which the columns `cols` = [(offset, width)] are named, inside a CANARY-filled
    allocation with guard rows on both sides."""

    def __init__(self, dev, planes, rows, ld, cols, pt=None):
        self.planes, self.rows, self.ld, self.pt = planes, rows, ld, pt or rows * ld
        self.G = (3 * ld + 7) // 4 * 4
        total = 2 * self.G + (planes - 1) * self.pt + rows * ld
        self.mask = torch.zeros(total, dtype=torch.bool)
        for p in range(planes):
            body = self.mask[self.G + p * self.pt:self.G + p * self.pt + rows * ld].view(rows, ld)
            for off, w in cols:
                body[:, off:off + w] = True
        self.t = torch.full((total,), cc.CANARY, dtype=torch.int32, device=dev)

    def ptr(self, off=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (self.G + off))

    def fill_named(self, planes_rows_width, off=0):
        """Named elements <- a float32 tensor [planes][rows][width] (zero-filled accumulators, priors); the rest keeps the canary."""
        self.t.fill_(cc.CANARY)
        f = self.t.view(F32)
        for p in range(self.planes):
            f[self.G + p * self.pt:self.G + p * self.pt + self.rows * self.ld].view(self.rows, self.ld)[:, off:off + planes_rows_width.shape[-1]] = \
                planes_rows_width[p].to(self.t.device)

    def reset(self):
        self.t.fill_(cc.CANARY)

    def fetch(self, what):
        torch.cuda.synchronize()
        raw = self.t.cpu()
        bad = int((raw[~self.mask] != cc.CANARY).sum())
        assert bad == 0, (what, "elements the contract does not name were written", bad)
        self.f = raw.view(F32)
        assert torch.isfinite(self.f[self.mask]).all(), (what, "a named element is not finite")
        return self

    def get(self, off, width):
        return torch.stack([self.f[self.G + p * self.pt:self.G + p * self.pt + self.rows * self.ld].view(self.rows, self.ld)[:, off:off + width]
                            for p in range(self.planes)]).clone()


def fed(x, ld, off, views, dev, planes=1):
    """x [planes * n][rows][C] float32 inside a NaN-filled buffer (cc.poisoned): (device tensor starting at the first fed element, batch stride in rows,
    plane stride in floats)."""
    buf, start, bs = cc.poisoned(x, ld, off, views, NAN)
    n = x.shape[0] // planes
    tv = views[0] if views else 1
    return buf.to(dev)[start:], bs, n * tv * x.shape[1] * ld


def side(t, dev):
    """A dense side operand (residual, aux_h, aux_z, bias ..) with NaN guard rows."""
    if t is None:
        return None
    t2 = t.reshape(1, -1, t.shape[-1]) if t.dim() > 1 else t.reshape(1, 1, -1)
    return fed(t2.contiguous(), t2.shape[-1], 0, None, dev)[0]


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def within(got, ref, bound, what):
    r = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    assert r <= 1, (what, "unconditional bound exceeded %.3g times" % r)
    return r


def twice(fn, bufs, what):
    """Launch, fetch, launch again on fresh canaries, assert the two results bitwise equal. Returns the first results."""
    outs = []
    for _ in range(2):
        for b in bufs:
            b.reset()
        fn()
        outs.append([b.fetch(what).f.clone() for b in bufs])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, "two runs differ")
    return outs[0]


class Chain:
    """The forward launches of one case on the device, stage by stage (module docstring); keeps what later stages and tests read."""

    def __init__(self, c, dev):
        self.c, self.dev, self.d = c, dev, wc.make_data(c)
        self.lib, self.grid, self.R, self.M = _lib.lib(), wc.grid_of(c), wc.R_of(c), c.n * c.D * c.H * c.W

    def st(self):
        return _lib.current_stream()

    # ---- forge_wino_input: exact
    def input_stage(self):
        c, d, L, R = self.c, self.d, self.lib, self.R
        rows = c.D * c.H * c.W
        Cin = c.C1 + c.C2
        if c.vcat:
            ldv, ptv = Cin + c.vcat, R * (Cin + c.vcat) + c.vcat
            self.Vb = OutBuf(self.dev, 16, R, ldv, [(0, Cin)], ptv)
            plan = [("x1", c.C1, 0, self.Vb), ("x2", c.C2, c.C1, self.Vb)]
        else:
            self.V1b = OutBuf(self.dev, 16, R, c.C1, [(0, c.C1)])
            self.V2b = OutBuf(self.dev, 16, R, c.C2, [(0, c.C2)]) if c.C2 else None
            plan = [("x1", c.C1, 0, self.V1b)] + ([("x2", c.C2, 0, self.V2b)] if c.C2 else [])
        ins = {}
        for key, C, voff, buf in plan:
            x = d[key]
            ld, off, views = (c.ld1, c.off1, c.views1) if key == "x1" else (c.ld2, c.off2, None)
            nsum = c.nsum if key == "x1" else 1
            if nsum > 1:                                          # the views of a scene lie `rows` rows apart, scenes nsum x rows
                t, bs, _ = fed(x.permute(1, 0, 2, 3, 4, 5).reshape(c.n, nsum * rows, C).contiguous(), ld, off, None, self.dev)
                bs = nsum * rows
            else:
                t, bs, _ = fed(x.reshape(c.n, rows, C), ld, off, views, self.dev)
            ins[key] = (t, ld, bs, C, voff, buf, nsum)
        bufs = [self.Vb] if c.vcat else [b for b in (self.V1b, self.V2b) if b is not None]

        def run():
            for key in ins:
                t, ld, bs, C, voff, buf, nsum = ins[key]
                _lib.check(L.forge_wino_input(P(t), ld, bs, buf.ptr(voff), buf.ld, buf.pt if c.vcat else 0, c.n, c.D, c.H, c.W, C, nsum, rows if nsum > 1 else 0,
                                              self.st()), "forge_wino_input")
        twice(run, bufs, (c.name, "input"))
        self.V = []
        for key in ins:
            t, ld, bs, C, voff, buf, nsum = ins[key]
            got = buf.get(voff, C)
            if nsum == 1:
                assert torch.equal(got, wc.input_transform(d[key], 1, F32)), (c.name, key, "forge_wino_input is not the float32 transform bit for bit")
                emit("%-9s input   %s C %3d ld %3d bs %5d ldv %3d  exact" % (c.name, key, C, ld, bs, buf.ld))
            else:
                r = within(got, wc.input_transform(d[key], nsum), wc.gamma(nsum + 3) * wc.input_transform(d[key], nsum, mag=True), (c.name, "input mean"))
                emit("%-9s input   %s C %3d nsum %d  uncond %.2e" % (c.name, key, C, nsum, r))
            self.V.append(got)
        self.Vcat = torch.cat(self.V, dim=-1)

    # ---- forge_wino_weights: the float64 product rounded once
    def weight_stage(self):
        c = self.c
        wp = self.d["wp"].to(self.dev)
        U = co.wino_pack_packed(wp, transpose=c.dgrad)
        assert torch.equal(U.cpu(), wc.weights(self.d["wp"], c.kd, c.dgrad, F32)), (c.name, "forge_wino_weights")
        assert torch.equal(U, co.wino_pack_packed(wp, transpose=c.dgrad)), (c.name, "forge_wino_weights: two runs differ")
        self.U, self.Ucpu = U, U.cpu()

    # ---- forge_wino_gemm (every tile), forge_wino_gemm_half
    def gemm_args(self):
        c = self.c
        if c.gviews:                                              # V1 as view `view` of a [n][views] stack: the transform's own output (bitwise what
            if not hasattr(self, "v1g"):                          # input_stage checked) re-laid with the other views' rows NaN
                self.v1g = fed(self.V[0].reshape(16 * c.n, self.R // c.n, c.C1), c.C1, 0, c.gviews, self.dev, planes=16)
            t, bs1, pt1 = self.v1g
            return (P(t), c.C1, c.C1, bs1, pt1, self.V2b.ptr() if c.C2 else None, c.C2, c.C2, 0, 0)
        if c.vcat:
            b = self.Vb
            return (b.ptr(0), c.C1, b.ld, 0, b.pt, b.ptr(c.C1) if c.C2 else None, c.C2, b.ld if c.C2 else 0, 0, b.pt if c.C2 else 0)
        return (self.V1b.ptr(), c.C1, c.C1, 0, 0, self.V2b.ptr() if c.C2 else None, c.C2, c.C2, 0, 0)

    def gemm_stage(self, tiles):
        c, L, R = self.c, self.lib, self.R
        Cin = c.C1 + c.C2
        ref, mg = wc.point_gemm(self.Vcat, self.Ucpu, self.grid), wc.point_gemm(self.Vcat, self.Ucpu, self.grid, mag=True)
        self.Mb = OutBuf(self.dev, 16, R, c.Cout, [(0, c.Cout)])
        yq = None
        if tiles:                                                 # the GEMM stage's own yardstick: the chain grain on the stage's inputs
            yq = wc.q_of(wc.point_gemm(self.Vcat, self.Ucpu, self.grid, F32, "chain"), ref, mg)
        rule = chr(L.forge_wino_gemm_tile(R, c.Cout, Cin))
        assert rule == wc.rule_tile(c), (c.name, rule)
        res = {}
        for tile in (0,) + tuple(tiles):
            args = self.gemm_args() + (P(self.U), self.Mb.ptr(), c.n, c.D, c.H // 2, c.W // 2, c.Cout, c.kd, ord(tile) if tile else 0, self.st())
            twice(lambda: _lib.check(L.forge_wino_gemm(*args), "forge_wino_gemm"), [self.Mb], (c.name, "gemm", tile))
            got = self.Mb.get(0, c.Cout)
            r = within(got, ref, wc.gamma(wc.k_gemm(c)) * mg, (c.name, "gemm", tile))
            q, qr = wc.q_of(got, ref, mg)
            emit("%-9s gemm    tile %s K %4d R %5d bs1 %5d  q %5.2f q_rms %5.3f yard %s uncond %.2e" % (
                c.name, tile or rule.lower(), c.kd * Cin, R, self.gemm_args()[3], q, qr, "%5.2f %5.3f" % yq if yq else "    -     -", r))
            if yq:
                assert q <= wc.SHARP * yq[0] and qr <= wc.SHARP * yq[1], (c.name, "gemm", tile, q, qr, yq)
            res[tile] = got
        for i, ta in enumerate(tiles):                            # every pair of tiles within twice the sharp bound of each other
            for tb in tiles[i + 1:]:
                r = ((res[ta].double() - res[tb].double()).abs() / (2 * wc.SHARP * yq[0] * wc.U * mg)).max().item()
                assert r <= 1, (c.name, "tiles", ta, tb, r)
        if tiles:
            assert torch.equal(res[0], res[rule]), (c.name, "tile 0 is not the rule's tile")
        self.Mm = res[0]
        self.Mb.reset()                                           # leave the rule's products on the device for the output stage
        _lib.check(L.forge_wino_gemm(*(self.gemm_args() + (P(self.U), self.Mb.ptr(), c.n, c.D, c.H // 2, c.W // 2, c.Cout, c.kd, 0, self.st()))), "forge_wino_gemm")
        self.M8b = OutBuf(self.dev, 8, R, c.Cout, [(0, c.Cout)])
        if rule == "B":                                           # the 8-plane form on its own feet: against the float64 row-combined point products
            args = self.gemm_args() + (P(self.U), self.M8b.ptr(), c.n, c.D, c.H // 2, c.W // 2, c.Cout, c.kd, self.st())
            twice(lambda: _lib.check(L.forge_wino_gemm_half(*args), "forge_wino_gemm_half"), [self.M8b], (c.name, "gemm_half"))
            got8 = self.M8b.get(0, c.Cout)
            mg8 = wc.row_combine(mg, mag=True)
            r = within(got8, wc.row_combine(ref), wc.gamma(wc.k_gemm(c) + 2) * mg8, (c.name, "gemm_half"))      # + the row stage's two additions
            q, qr = wc.q_of(got8, wc.row_combine(ref), mg8)
            emit("%-9s gemm8   tile B K %4d R %5d  q %5.2f q_rms %5.3f uncond %.2e" % (c.name, c.kd * Cin, R, q, qr, r))
            assert torch.equal(got8, wc.row_combine(self.Mm)), (c.name, "gemm_half is not the row-combined 16 planes bit for bit")
            self.Mm8 = got8
        else:                                                     # forge_wino_output_half takes any 8 planes: the float32 row stage of the 16
            self.Mm8 = wc.row_combine(self.Mm)
            self.M8b.fill_named(self.Mm8)

    # ---- forge_wino_output / forge_wino_output_half
    def output_stage(self):
        c, d, L, M = self.c, self.d, self.lib, self.M
        vol = self.R // c.n
        ops = {k: side(d[k], self.dev) for k in ("bias", "scale", "shift", "residual", "aux_h", "aux_z")}
        m2 = {16: None, 8: None}
        bs2 = pt2 = off2 = 0
        if c.mm2:
            views, view = c.mm2
            full = torch.full((16, c.n, views, vol, c.Cout), NAN)             # the other views' rows are NaN
            full[:, :, view] = d["mm2"].reshape(16, c.n, views, vol, c.Cout)[:, :, view]
            full = full.reshape(16, -1, c.Cout)
            m2[16] = side(full.reshape(-1, c.Cout), self.dev)
            m2[8] = side(wc.row_combine(full).reshape(-1, c.Cout), self.dev)
            bs2, pt2, off2 = views * vol, c.n * views * vol * c.Cout, view * vol * c.Cout
        named = wc.out_names(c)
        width = c.Cout // 2 if c.epi == 2 else c.Cout
        self.out = {}
        for form, fn, mb, mm in ((16, L.forge_wino_output, self.Mb, self.Mm), (8, L.forge_wino_output_half, self.M8b, self.Mm8)):
            bufs = {k: OutBuf(self.dev, 1, M, c.ldo, [(0, width)]) for k in named}
            p2 = None if m2[form] is None else ctypes.c_void_p(m2[form].data_ptr() + 4 * off2)
            args = (mb.ptr(), p2, bs2, pt2, P(ops["bias"]), P(ops["scale"]), P(ops["shift"]), c.slope, P(ops["residual"]), P(ops["aux_h"]), P(ops["aux_z"]),
                    bufs["out"].ptr(), bufs["out2"].ptr() if "out2" in bufs else None, bufs["out3"].ptr() if "out3" in bufs else None,
                    c.n, c.D, c.H, c.W, c.Cout, c.ldo, c.epi, self.st())
            name = "forge_wino_output" + ("_half" if form == 8 else "")
            twice(lambda: _lib.check(fn(*args), name), list(bufs.values()), (c.name, name))
            v2 = wc.mm2_view(c, d)
            v2 = None if v2 is None else (v2 if form == 16 else wc.row_combine(v2))
            S = wc.inverse_transform(mm, v2, self.grid, mag=True)
            ref, sS, sA = wc.tail(wc.inverse_transform(mm, v2, self.grid), S, c, d)
            self.out[form] = {}
            for k in named:
                got = bufs[k].get(0, width)[0]
                r = within(got, ref[k], wc.gamma(wc.k_out(c)) * sS[k] + wc.EPI_ULPS * 2 * wc.U * sA[k], (c.name, name, k))
                emit("%-9s output%-2d %-4s epi %d ldo %3d mm2 %s  uncond %.2e" % (c.name, form, k, c.epi, c.ldo, c.mm2, r))
                self.out[form][k] = got
        if not c.mm2:
            for k in named:
                assert torch.equal(self.out[16][k], self.out[8][k]), (c.name, k, "the 8-plane output differs from the 16-plane one")

    def forward(self, tiles=()):
        self.input_stage()
        self.weight_stage()
        self.gemm_stage(tiles)
        self.output_stage()
        return self


_YARD = {}


def chain_yardstick(c, d, half):
    """{output: (q, q_rms)} of the float32 CPU chain in the documented order, on the corner where the case is a real launch of the step."""
    key = (c.name, half)
    if key not in _YARD:
        cs, ds = wc.corner(c, d)
        ref, sS, sA = wc.chain(cs, ds, half=half, want_sigma=True)
        y = wc.chain(cs, ds, F32, half=half)[0]
        _YARD[key] = {k: wc.q_of(y[k], ref[k], sS[k] + sA[k]) for k in ref}
    return _YARD[key]


def direct_q(c, d, ref, sig, dev):
    """q of forge_conv_igemm on the same case, where the two kernels compute the same formula (no residual before an affine map, one addend, no view
    mean); None otherwise."""
    if c.mm2 or c.nsum > 1 or (c.residual and c.epi <= 1):
        return None
    taps = cc.T27 if c.kd == 3 else cc.T9
    wp = d["wp"]
    if c.dgrad:
        taps, wp = [(-a, -b, -e) for a, b, e in taps], wp.transpose(1, 2).contiguous()
    up = lambda t: None if t is None else t.contiguous().to(dev)
    width = c.Cout // 2 if c.epi == 2 else c.Cout
    outs = {k: torch.full((c.n * c.D * c.H * c.W, width), NAN, device=dev) for k in wc.out_names(c)}
    co.conv_igemm(up(d["x1"]), c.C1, c.C1, up(d["x2"]), c.C2, c.C2, up(wp), up(d["bias"]), up(d["scale"]), up(d["shift"]), c.slope, up(d["residual"]),
                  up(d["aux_h"]), up(d["aux_z"]), outs["out"], outs.get("out2"), (c.n, c.D, c.H, c.W), (c.D, c.H, c.W), c.Cout, c.Cout, taps, epilogue=c.epi,
                  out3=outs.get("out3"))
    return {k: wc.q_of(outs[k].cpu(), ref[k], sig[k]) for k in outs}


_CHAINS = {}


def launched(c, dev):
    """Every launch of the case - forward under all its tiles, then the backward - with the stage assertions; kept for test_bounds_reject_wrong_references
    where that test reads the case (small cases only), so that no case is launched or printed twice."""
    if c.name in _CHAINS:
        return _CHAINS[c.name]
    ch = Chain(c, dev).forward(c.tiles)
    if c.wgrad is not None or c.dy_ld:
        backward(ch)
    if any(c.name == n for n, _ in wc.MUTATION_CASES):
        _CHAINS[c.name] = ch
    return ch


@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_case(dev, name):
    c = wc.CASE[name]
    t0 = time.time()
    ch = launched(c, dev)
    d = ch.d
    # ---- the whole chain against float64, both output kernels; the direct kernel beside it
    fails = []
    ref, sS, sA = wc.chain(c, d, want_sigma=True)
    sig = {k: sS[k] + sA[k] for k in ref}
    ref8 = wc.chain(c, d, half=True)[0] if c.mm2 else ref
    dq = direct_q(c, d, ref, sig, dev)
    for form, rf in ((16, ref), (8, ref8)):
        yard = chain_yardstick(c, d, form == 8)
        for k in rf:
            q, qr = wc.q_of(ch.out[form][k], rf[k], sig[k])
            emit("%-9s chain%-2d  %-4s K %4d  q %5.2f q_rms %5.3f | yard %5.2f %5.3f r %4.2f %4.2f | direct %s" % (
                name, form, k, 9 * c.kd * (c.C1 + c.C2), q, qr, yard[k][0], yard[k][1], q / yard[k][0], qr / yard[k][1],
                "%5.2f %5.3f w/d %4.2f" % (dq[k] + (q / dq[k][0],)) if dq else "-"))
            if q > wc.SHARP * yard[k][0] or qr > wc.SHARP * yard[k][1]:
                fails.append((name, form, k, q, qr, yard[k]))
    assert not fails, fails
    emit("%-9s done in %.2f s" % (name, time.time() - t0))


def backward(ch):
    """forge_wino_input_dy, forge_wino_dy (exact), forge_wino_wgrad / _det (gamma_(R + 2)), forge_wino_dw onto a prior (gamma_5), and the weight-gradient chain
    against float64 autograd's value (wino_cases.wgrad_chain, pinned to it on the CPU)."""
    c, d, L, dev, R, grid = ch.c, ch.d, ch.lib, ch.dev, ch.R, ch.grid
    Cin, M, vol = c.C1 + c.C2, ch.M, ch.R // c.n
    dy5 = d["dy"].reshape(c.n, c.D, c.H, c.W, c.Cout)
    ld = c.dy_ld or c.Cout
    dyt, _, _ = fed(d["dy"].reshape(1, M, c.Cout), ld, ld - c.Cout, None, dev)        # the channel slice at the END of wider rows
    Vb, dMb, dM2b = (OutBuf(dev, 16, R, c.Cout, [(0, c.Cout)]) for _ in range(3))
    twice(lambda: _lib.check(L.forge_wino_input_dy(P(dyt), ld, Vb.ptr(), dMb.ptr(), c.n, c.D, c.H, c.W, c.Cout, ch.st()), "forge_wino_input_dy"), [Vb, dMb],
          (c.name, "input_dy"))
    twice(lambda: _lib.check(L.forge_wino_dy(P(dyt), ld, dM2b.ptr(), c.n, c.D, c.H, c.W, c.Cout, ch.st()), "forge_wino_dy"), [dM2b], (c.name, "dy"))
    dM = wc.dy_transform(dy5, F32)
    assert torch.equal(Vb.get(0, c.Cout), wc.input_transform(dy5, 1, F32)), (c.name, "forge_wino_input_dy: V")
    assert torch.equal(dMb.get(0, c.Cout), dM), (c.name, "forge_wino_input_dy: dM")
    assert torch.equal(dM2b.get(0, c.Cout), dM), (c.name, "forge_wino_dy")
    emit("%-9s input_dy / dy  C %3d ld %3d  exact" % (c.name, c.Cout, ld))
    if c.wgrad is None:
        return
    # ---- the point sums: V1 as view `view` of `views` per batch element (bs1, pt1), the other views' rows NaN
    views, view = c.wgrad or (1, 0)
    v1, bs1, pt1 = fed(ch.V[0].reshape(16 * c.n, vol, c.C1), c.C1, 0, (views, view) if views > 1 else None, dev, planes=16)
    v2 = fed(ch.V[1].reshape(16 * c.n, vol, c.C2), c.C2, 0, None, dev, planes=16)[0] if c.C2 else None
    if views == 1:
        bs1 = pt1 = 0
    ref, mg = wc.wgrad_points(dM, ch.Vcat, grid, c.kd), wc.wgrad_points(dM, ch.Vcat, grid, c.kd, mag=True)
    bound = wc.gamma(R + 2) * mg
    dUb = OutBuf(dev, 1, 16 * c.kd * c.Cout, Cin, [(0, Cin)])
    shape = (16, c.kd, c.Cout, Cin)
    head = (dMb.ptr(), P(v1), c.C1, bs1, pt1, P(v2), c.C2, 0, 0, dUb.ptr(), c.n, c.D, c.H // 2, c.W // 2, c.Cout, c.kd)
    dUb.fill_named(torch.zeros(1, 16 * c.kd * c.Cout, Cin))
    _lib.check(L.forge_wino_wgrad(*(head + (ch.st(),))), "forge_wino_wgrad")
    got_a = dUb.fetch((c.name, "wgrad")).get(0, Cin).reshape(shape)
    ra = within(got_a, ref, bound, (c.name, "wgrad"))
    nb = L.forge_wino_wgrad_det_ws_bytes(c.C1, c.C2, c.n, c.D, c.H // 2, c.W // 2, c.Cout, c.kd)
    assert nb > 0, (c.name, nb)
    ws = torch.full((nb // 4 + 64,), NAN, device=dev)
    det = lambda acc: _lib.check(L.forge_wino_wgrad_det(*(head + (acc, P(ws), nb, ch.st()))), "forge_wino_wgrad_det")
    twice(lambda: det(0), [dUb], (c.name, "wgrad_det 0"))                              # written over the canary NaNs: prior contents are ignored
    got_d = dUb.get(0, Cin).reshape(shape)
    rd = within(got_d, ref, bound, (c.name, "wgrad_det"))
    prior = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    accs = []
    for _ in range(2):
        dUb.fill_named(prior.reshape(1, -1, Cin))
        det(1)
        accs.append(dUb.fetch((c.name, "wgrad_det 1")).get(0, Cin).reshape(shape))
    assert torch.equal(accs[0], accs[1]), (c.name, "wgrad_det accumulate = 1: two runs differ")
    assert torch.equal(accs[0], prior + got_d), (c.name, "accumulate = 1 is not prior + S with one fp32 addition")
    q, qr = wc.q_of(got_d, ref, mg)
    emit("%-9s wgrad   Cin %3d+%3d kd %d R %4d views %s  q %5.2f q_rms %5.3f uncond atomic %.2e det %.2e" % (c.name, c.C1, c.C2, c.kd, R, c.wgrad, q, qr, ra, rd))
    # ---- G^T dU G onto a non-zero prior
    dwb = OutBuf(dev, 1, 9 * c.kd * c.Cout, Cin, [(0, Cin)])
    dUd = got_d.to(dev)
    runs = []
    for _ in range(2):
        dwb.fill_named(d["prior"].reshape(1, -1, Cin))
        _lib.check(L.forge_wino_dw(P(dUd), dwb.ptr(), c.Cout, Cin, c.kd, ch.st()), "forge_wino_dw")
        runs.append(dwb.fetch((c.name, "dw")).get(0, Cin).reshape(9 * c.kd, c.Cout, Cin))
    assert torch.equal(runs[0], runs[1]), (c.name, "forge_wino_dw: two runs differ")
    r = within(runs[0], wc.dw_transform(got_d, d["prior"]), wc.gamma(wc.K_DW) * wc.dw_transform(got_d, d["prior"], mag=True), (c.name, "dw"))
    # ---- the chain dy, x -> prior + dw against float64
    wref, wsig = wc.wgrad_chain(c, d), wc.wgrad_chain(c, d, mag=True)
    yq = wc.q_of(wc.wgrad_chain(c, d, F32), wref, wsig)
    q, qr = wc.q_of(runs[0], wref, wsig)
    emit("%-9s dw      uncond %.2e | chain q %5.2f q_rms %5.3f | yard %5.2f %5.3f r %4.2f %4.2f" % (c.name, r, q, qr, yq[0], yq[1], q / yq[0], qr / yq[1]))
    assert q <= wc.SHARP * yq[0] and qr <= wc.SHARP * yq[1], (c.name, "wgrad chain", q, qr, yq)
    ch.dw, ch.dw_ref, ch.dw_sig, ch.dw_yard = runs[0], wref, wsig, yq


@pytest.mark.parametrize("co_,ci_,kd", wc.WEIGHT_SHAPES)
def test_weights_of_odd_channel_counts(dev, co_, ci_, kd):
    wp = torch.randn(9 * kd, co_, ci_, generator=torch.Generator().manual_seed(co_ + ci_))
    for tr in (False, True):
        assert torch.equal(co.wino_pack_packed(wp.to(dev), transpose=tr).cpu(), wc.weights(wp, kd, tr, F32)), (co_, ci_, kd, tr)


@pytest.mark.parametrize("name,muts", wc.MUTATION_CASES)
def test_bounds_reject_wrong_references(dev, name, muts):
    """The correct kernels against deliberately wrong references: each must fail the sharp bound. Nothing faulty is launched."""
    c = wc.CASE[name]
    ch = launched(c, dev)
    d = ch.d
    _, sS, sA = wc.chain(c, d, want_sigma=True)
    yard = chain_yardstick(c, d, False)
    for mut in muts:
        if mut == "dw_g_swap" or (mut == "pt_transposed" and name == "bw32"):
            q, qr = wc.q_of(ch.dw, wc.wgrad_chain(c, d, mut=mut), ch.dw_sig)
            ratio = max(q / ch.dw_yard[0], qr / ch.dw_yard[1])
        else:
            wrong = wc.chain(c, d, mut=mut)[0]
            ratio = max(max(a / b for a, b in zip(wc.q_of(ch.out[16][k], wrong[k], sS[k] + sA[k]), yard[k])) for k in wrong)
        emit("%-9s wrong reference %-16s q / yardstick %.3g" % (name, mut, ratio))
        assert ratio > wc.SHARP, (name, mut, ratio)


def test_refusals(dev):
    """The refusals of the contract: a negative code and forge_last_error's text, before any launch. Every call passes real allocations large enough for
    the nearest accepted call (the baseline at the end, which is launched), so that a check that wrongly accepts touches nothing the test does not own."""
    L = _lib.lib()
    buf = lambda nfl: torch.zeros(nfl, dtype=F32, device=dev)
    x, V, Uw, Mm, o, o2, o3, aux, vec = buf(1 << 16), buf(1 << 18), buf(1 << 18), buf(1 << 20), buf(1 << 18), buf(1 << 18), buf(1 << 18), buf(1 << 18), buf(1024)
    ws = buf(1 << 20)
    st = _lib.current_stream
    b = dict(n=1, D=2, H=4, W=4, C=32, C2=0, Cout=32, ld=32, ldv=32, ldo=32, kd=3, tile=0, epi=0, v2=False, sc=False, ah=False, az=False, o2=False, o3=False)

    def inp(**kw):
        a = dict(b, **kw)
        return L.forge_wino_input(P(x), a["ld"], 0, P(V), a["ldv"], 0, a["n"], a["D"], a["H"], a["W"], a["C"], 1, 0, st())

    def gemm(**kw):
        a = dict(b, **kw)
        return L.forge_wino_gemm(P(V), a["C"], a["C"], 0, 0, P(V) if a["v2"] else None, a["C2"], a["C2"], 0, 0, P(Uw), P(Mm), a["n"], a["D"], a["H"] // 2,
                                 a["W"] // 2, a["Cout"], a["kd"], a["tile"], st())

    def outp(half=False, **kw):
        a = dict(b, **kw)
        fn = L.forge_wino_output_half if half else L.forge_wino_output
        return fn(P(Mm), None, 0, 0, P(vec), P(vec) if a["sc"] else None, P(vec) if a["sc"] else None, 1.0, None, P(aux) if a["ah"] else None,
                  P(aux) if a["az"] else None, P(o), P(o2) if a["o2"] else None, P(o3) if a["o3"] else None, a["n"], a["D"], a["H"], a["W"], a["Cout"], a["ldo"],
                  a["epi"], st())

    def wgrad(det=False, **kw):
        a = dict(b, **kw)
        head = (P(Mm), P(V), a["C"], 0, 0, P(V) if a["v2"] else None, a["C2"], 0, 0, P(Uw), a["n"], a["D"], a["H"] // 2, a["W"] // 2, a["Cout"], a["kd"])
        return L.forge_wino_wgrad_det(*(head + (0, P(ws), ws.numel() * 4, st()))) if det else L.forge_wino_wgrad(*(head + (st(),)))

    with torch.cuda.device(dev):
        for what, call, text in (
                ("odd H", lambda: inp(H=3), b"H, W even"), ("odd W", lambda: inp(W=5), b"H, W even"), ("C % 4", lambda: inp(C=30, ld=32), b"multiples of 4"),
                ("ld < C", lambda: inp(ld=28), b"forge_wino_input"), ("ldv < C", lambda: inp(ldv=28), b"forge_wino_input"),
                ("odd H, output", lambda: outp(H=3), b"H, W even"), ("odd W, dy", lambda: L.forge_wino_dy(P(x), 32, P(Mm), 1, 2, 4, 5, 32, st()), b"H, W even"),
                ("odd H, input_dy", lambda: L.forge_wino_input_dy(P(x), 32, P(V), P(Mm), 1, 2, 3, 4, 32, st()), b"H, W even"),
                ("C1 % 32", lambda: gemm(C=48), b"multiples of"), ("Cout <= 16", lambda: gemm(Cout=16), b"Cout > 16"), ("kd = 2", lambda: gemm(kd=2), b"kd not 1 or 3"),
                ("kd = 2, weights", lambda: L.forge_wino_weights(P(Uw), P(Mm), 32, 32, 2, 0, st()), b"kd = 1 or 3"),
                ("kd = 2, dw", lambda: L.forge_wino_dw(P(Uw), P(Mm), 32, 32, 2, st()), b"kd = 1 or 3"),
                ("V2 without C2", lambda: gemm(v2=True), b"V2 given iff"), ("C2 without V2", lambda: gemm(C2=32), b"V2 given iff"),
                ("tile F", lambda: gemm(tile=ord("F")), b"tile must be"), ("epilogue 4", lambda: outp(epi=4, sc=True, ah=True, az=True, o2=True), b"unknown epilogue"),
                ("affine without scale", lambda: outp(epi=1), b"needs scale/shift"), ("gates without aux_h", lambda: outp(epi=2, o2=True, ldo=16), b"needs aux_h, out2"),
                ("gates without out2", lambda: outp(epi=2, ah=True, ldo=16), b"needs aux_h, out2"), ("state without aux_z", lambda: outp(epi=3, ah=True), b"needs aux_h, aux_z"),
                ("state out2 without scale", lambda: outp(epi=3, ah=True, az=True, o2=True), b"needs aux_h, aux_z"),
                ("out3 with epilogue 0", lambda: outp(o3=True), b"out3 is a GRU"), ("out3 with epilogue 1", lambda: outp(epi=1, sc=True, o3=True), b"out3 is a GRU"),
                ("out3 with epilogue 1, half", lambda: outp(half=True, epi=1, sc=True, o3=True), b"out3 is a GRU"),
                ("ldo < Cout", lambda: outp(ldo=28), b"ldo >= Cout"), ("ldo = 0", lambda: outp(ldo=0), b"ldo >= Cout"), ("ldo < Cout, half", lambda: outp(half=True, ldo=16), b"ldo >= Cout"),
                ("ldo < Cout, state", lambda: outp(epi=3, ah=True, az=True, ldo=16), b"ldo >= Cout"),
                ("gates with ldo != Cout / 2", lambda: outp(epi=2, ah=True, o2=True, ldo=32), b"ldo == Cout / 2"),
                ("two-input wgrad with C1 % 128", lambda: wgrad(v2=True, C2=32), b"C1 a multiple of"),
                ("two-input wgrad_det with C1 % 128", lambda: wgrad(det=True, v2=True, C2=32), b"C1 a multiple of"), ("kd = 2, wgrad", lambda: wgrad(kd=2), b"kd not 1 or 3")):
            rc = call()
            msg = L.forge_last_error()
            assert rc < 0 and text in msg, (what, rc, msg)
        for what, call in (("input", inp), ("gemm", gemm), ("output", outp), ("output_half", lambda: outp(half=True)), ("gates", lambda: outp(epi=2, ah=True, o2=True, ldo=16)),
                           ("wgrad", wgrad), ("wgrad_det", lambda: wgrad(det=True))):
            assert call() == 0, (what, L.forge_last_error())              # the baselines themselves are legal launches
        torch.cuda.synchronize()


@pytest.mark.parametrize("wino", [True, False])
def test_frozen_layer_with_residual_keeps_its_formula_on_both_branches(dev, wino):
    """frozen.run_layer promises act((conv(x) + bias) * scale + shift + residual). A 3x3, 128 -> 128 folded-BatchNorm layer with a residual against float64,
    with the Winograd path on and off: forge_wino_output's affine epilogue adds the residual before the affine map, so run_layer must not hand it one."""
    from forge_amd import frozen
    g = torch.Generator().manual_seed(21)
    conv, bn = torch.nn.Conv3d(128, 128, 3, padding=1), torch.nn.BatchNorm3d(128)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(128, generator=g) + 0.5), bn.bias.copy_(torch.randn(128, generator=g))
        bn.running_mean.copy_(torch.randn(128, generator=g)), bn.running_var.copy_(torch.rand(128, generator=g) + 0.5)
    conv, bn = conv.to(dev).eval(), bn.to(dev).eval()
    x, res = torch.randn(2, 128, 4, 8, 8, generator=g), torch.randn(2, 128, 4, 8, 8, generator=g)
    with torch.no_grad():
        ref = torch.nn.functional.leaky_relu(bn.double()(conv.double()(x.double().to(dev))) + res.double().to(dev), 0.01).cpu()
        conv, bn = conv.float(), bn.float()
        Lp = frozen.pack_layer(conv, bn, 0.01)
        assert Lp["U"] is not None and co.wino_applies(Lp["taps"], 1, 2, 4, 8, 8, 128, 0, 128)
        with co.winograd(wino):
            got = frozen.run_layer(Lp, x.permute(0, 2, 3, 4, 1).contiguous().to(dev), res.permute(0, 2, 3, 4, 1).contiguous().to(dev))
    err = (got.permute(0, 4, 1, 2, 3).double().cpu() - ref).abs().max().item()
    emit("frozen residual layer winograd %s  max abs err %.2e of max %.2f" % (wino, err, ref.abs().max().item()))
    assert err < 1e-5 * max(1.0, ref.abs().max().item()), (wino, err)
