"""GPU (-m gpu): forge_conv_igemm over its launch space - tile x split-K x epilogue x output mapping x operand addressing x ragged edges - against
the float64 restatement of its contract (tests/conv_igemm_cases.py), through convops.conv_igemm (the launcher is under test too).

Per case x plan:
  canaries       every output lives inside a larger allocation filled with a NaN of a known bit pattern (guard rows before and after, padding columns
                 [Cout, ldo), rows of the output grid the launch does not name). Afterwards every element the contract does not name still holds the
                 pattern and every element it names is finite. Input padding (columns outside the fed channel slice, rows of skipped views, guard
                 rows, residual / aux rows of voxels the launch does not name) is NaN: one element read too many into a sum fails loudly.
  unconditional  |got - ref| <= gamma sigma_S + EPI_ULPS 2 u sigma_A per element (conv_igemm_cases' docstring): true of any fp32 evaluation in any order.
  sharp          q = max |got - ref| / (u sigma) and q_rms within SHARP = 4x the values of a float32 CPU evaluation of the same contract (the yardstick,
                 YARDSTICK below says at which grain); no element is excluded.
  determinism    the launch repeated once is bitwise identical (split-K and the statistics included).
Per case: all plans agree with each other within twice the sharp bound; merged phases equal the single-phase launches bitwise on every tile;
the statistics by-product equals float64 sums of the kernel's own outputs. test_bounds_reject_wrong_references runs the correct kernel against
deliberately wrong references, test_refusals_of_the_contract pins the refusals the matrix relies on (no launch).

Every line "conv_igemm_matrix ..." printed under -s is a row of profiles/r10_conv_igemm_matrix.txt.
"""
import ctypes
import time

import pytest
import torch

import conv_igemm_cases as cc
from forge_amd import _lib, convops as co

pytestmark = pytest.mark.gpu

# The grain of the float32 CPU yardstick of the sharp bound (conv_igemm_cases._accumulate):
#   "tap"    accumulated tap by tap, one blocked matmul over all input channels per tap - where the matrix started. A blocked matmul sums in many short
#            partial chains; the kernel's K loop is one fmaf chain of length K per output element (conv_igemm.hip: "bitwise an fmaf chain"), whose rounding
#            error grows with sqrt(K). Measured on the MI355X the kernel is up to 9.7x (q) / 4.5x (q_rms) this yardstick at K = 6912 and beyond 4x on
#            about a quarter of the launches (profiles/r10_conv_igemm_matrix.txt, columns "tap ... r"): the 4x does not hold at this grain.
#   "kstep"  one matmul per 32-channel K-step, the steps dealt to the plan's split-K slices, slice sums added in slice order: up to 6.6x / 4.7x, still beyond.
#   "chain"  the same order taken down to what the kernel documents: one fused multiply-add per k (taps outer, channels inner), per split-K slice,
#            then the fixed-order slice sum. The kernel measures 0.66-1.44x (q) and 0.86-1.05x (q_rms) of it over the whole matrix.
# A yardstick that a correct kernel exceeds is refined in the kernel's documented order; the factor is never raised. So the factor stays at 4x and the
# grain is "chain". All three are printed for every launch.
YARDSTICK = "chain"
CHAIN_BUDGET = 3e9              # M x Cout x K above which the chain-grain yardstick is evaluated on a 4 x 16 x 16 corner of the first batch element only


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


_REF, _YARD = {}, {}


def reference(case):
    if case.name not in _REF:
        d = cc.make_data(case)
        _REF[case.name] = (d, cc.evaluate(case, d))
    return _REF[case.name]


def yardstick(case, grain, ks):
    """{output: (q, q_rms)} of the float32 CPU evaluation at `grain`. A case too large for the chain grain is measured on a sub-grid of itself (same taps,
    weights and K; its own float64 reference): fewer elements can only lower a maximum, i.e. tighten the bound."""
    ks = 1 if grain == "tap" else ks
    key = (case.name, grain, ks)
    if key not in _YARD:
        d, ref = reference(case)
        c = case
        if grain == "chain" and case.n * case.D * case.H * case.W * case.Cout * cc.K_of(case) > CHAIN_BUDGET:
            assert case.epi == 0 and case.istride == 1 and case.ostride == 1 and not case.lift
            c = case._replace(n=1, D=4, H=16, W=16, in_grid=(4, 16, 16), out_grid=(4, 16, 16))
            d = dict(d, x1=d["x1"][:1, :4, :16, :16].contiguous(), x2=None if d["x2"] is None else d["x2"][:1, :4, :16, :16].contiguous())
            ref = cc.evaluate(c, d)
        y = cc.evaluate(c, d, torch.float32, grain=grain, ksplit=ks)
        _YARD[key] = {k: cc.q_stats(c, ref, y[k], k)[:2] for k in cc.out_desc(c)}
    return _YARD[key]


class Launch:
    """The device operands of a case, poisoned as the module docstring says, and launch(): fresh canary-filled outputs -> CPU copies."""

    def __init__(self, case, dev):
        self.case, self.dev = case, dev
        d, ref = reference(case)
        nan = float("nan")
        self.in1, self.bs1 = self._input(d["x1"], case.ld1, case.off1, case.views1)
        self.in2, self.bs2 = self._input(d["x2"], case.ld2, case.off2, case.views2) if case.C2 else (None, 0)
        up = lambda t: None if t is None else t.contiguous().to(dev)
        self.wp, self.bias, self.scale, self.shift = up(d["wp"]), up(d["bias"]), up(d["scale"]), up(d["shift"])
        named = ref["named"]

        def side(t, ld):                                   # residual / aux rows: NaN in rows the launch does not name and in the padding columns
            if t is None:
                return None
            t = t.clone()
            if not case.lift:
                t[~named] = nan
            buf, start, _ = cc.poisoned(t[None], ld, 0, None, nan)
            return buf.to(dev)[start:]
        gru = case.epi in (2, 3)
        self.residual = side(d["residual"], case.Cout if (gru or case.lift) else case.ldo)
        self.aux_h = side(d["aux_h"], case.Cout // 2 if case.epi == 2 else case.Cout)
        self.aux_z = side(d["aux_z"], case.Cout)
        self.desc = cc.out_desc(case)
        self.masks = {}
        for k, (rows, width, stride) in self.desc.items():
            G = (3 * stride + 3) // 4 * 4
            m = torch.zeros(rows, stride, dtype=torch.bool)
            m[named, :width] = True
            full = torch.zeros(G + rows * stride + G, dtype=torch.bool)
            full[G:G + rows * stride] = m.reshape(-1)
            self.masks[k] = (G, full)

    def _input(self, x, ld, off, views):
        n, C = x.shape[0], x.shape[-1]
        buf, start, bs = cc.poisoned(x.reshape(n, -1, C), ld, off, views, float("nan"))
        return buf.to(self.dev)[start:], bs

    def launch(self, tile, ks, phase=None, taps=None, wp=None, stats=None):
        """One conv_igemm under force_plan(tile, ks) (narrow cases: the library's own 'N'). Returns {output: float32 [rows][width] CPU copy of the
        named region's rows, NaN-patterned rows included}; asserts the canaries and the finiteness of every named element."""
        c = self.case
        outs = {}
        for k, (rows, width, stride) in self.desc.items():
            G, _ = self.masks[k]
            outs[k] = torch.full((2 * G + rows * stride,), cc.CANARY, dtype=torch.int32, device=self.dev)
        view = lambda k: None if k not in outs else outs[k].view(torch.float32)[self.masks[k][0]:]
        ph = (-1, -1, -1) if c.phase == "merged" else tuple(c.phase)
        if phase is not None:
            ph = phase
        args = (self.in1, c.C1, c.ld1, self.in2, c.C2, c.ld2, self.wp if wp is None else wp, self.bias, self.scale, self.shift, c.slope, self.residual,
                self.aux_h, self.aux_z, view("out"), view("out2"), (c.n, c.D, c.H, c.W), c.in_grid, c.Cout, c.ldo, c.taps if taps is None else taps)
        kw = dict(out_grid=c.out_grid, istride=c.istride, ostride=c.ostride, phase=ph, epilogue=c.epi, bs1=self.bs1, bs2=self.bs2, lift=c.lift,
                  out3=view("out3"), stats=stats)
        lim = cc.operand_limit(c)
        prev = co.MAX_OPERAND_BYTES
        if lim is not None:
            co.MAX_OPERAND_BYTES = lim
        try:
            if tile == "N":
                co.conv_igemm(*args, **kw)
            else:
                with co.force_plan(tile, ks):
                    co.conv_igemm(*args, **kw)
        finally:
            co.MAX_OPERAND_BYTES = prev
        torch.cuda.synchronize()
        res = {}
        for k, (rows, width, stride) in self.desc.items():
            G, full = self.masks[k]
            raw = outs[k].cpu()
            if phase is None:
                assert (raw[~full] == cc.CANARY).all(), (c.name, tile, ks, k, "an element the contract does not name was written",
                                                         int((raw[~full] != cc.CANARY).sum()))
                assert torch.isfinite(raw.view(torch.float32)[full]).all(), (c.name, tile, ks, k, "a named element is not finite")
            res[k] = raw.view(torch.float32)[G:G + rows * stride].view(rows, stride)[:, :width].clone()
        return res


LINES = []


def emit(line):
    LINES.append(line)
    print("conv_igemm_matrix " + line)


def measure(case, ref, got, tile, ks):
    """Prints every figure of the launch. Returns ({output: sharp bound per element}, the bounds it misses - asserted by the caller once every plan of
    the case has been printed)."""
    nm = ref["named"]
    yards = {g: yardstick(case, g, ks) for g in ("tap", "kstep", "chain")}
    fails, sharp = [], {}
    for k in cc.out_desc(case):
        q, qrms, at = cc.q_stats(case, ref, got[k], k)
        ub = ((got[k][nm].double() - ref[k][nm]).abs() / cc.unconditional_bound(case, ref, k)[nm]).max().item()
        yq, yr = yards[YARDSTICK][k]
        emit("%-10s %s%d %-4s K %5d  q %6.2f q_rms %6.3f | tap %5.2f %5.3f r %5.2f %5.2f | kstep %5.2f %5.3f r %5.2f %5.2f | chain %5.2f %5.3f r %5.2f %5.2f"
             " | uncond %.2e" % (case.name, tile, ks, k, cc.K_of(case) // cc.nphase(case), q, qrms,
                                 yards["tap"][k][0], yards["tap"][k][1], q / yards["tap"][k][0], qrms / yards["tap"][k][1],
                                 yards["kstep"][k][0], yards["kstep"][k][1], q / yards["kstep"][k][0], qrms / yards["kstep"][k][1],
                                 yards["chain"][k][0], yards["chain"][k][1], q / yards["chain"][k][0], qrms / yards["chain"][k][1], ub))
        sharp[k] = cc.SHARP * yq * cc.U * (ref["sig_S"][k] + ref["sig_A"][k])
        if ub > 1:
            fails.append((k, "unconditional bound exceeded %.3g times" % ub))
        if q > cc.SHARP * yq or qrms > cc.SHARP * yr:
            row = int(torch.nonzero(nm)[at // got[k].shape[1]])
            fails.append((k, "sharp bound: q %.2f (yardstick %.2f) q_rms %.3f (yardstick %.3f), worst at output row %d column %d"
                          % (q, yq, qrms, yr, row, at % got[k].shape[1])))
    return sharp, [(case.name, tile, ks) + tuple(f) for f in fails]


def check_stats(L, case, tile, got_out):
    M, C = case.n * case.D * case.H * case.W, case.Cout
    nb = cc.stats_blocks(M, tile)
    runs = []
    for _ in range(2):
        buf = torch.full(((nb + 2) * 2 * C,), float("nan"), dtype=torch.float64, device=L.dev)
        got = L.launch(tile, 1, stats=buf[2 * C:(nb + 1) * 2 * C])
        assert torch.equal(got["out"], got_out), (case.name, tile, "the output changes when statistics are asked for")
        raw = buf.cpu()
        assert torch.isnan(raw[:2 * C]).all() and torch.isnan(raw[(nb + 1) * 2 * C:]).all(), (case.name, tile, "statistics written outside their blocks")
        runs.append(raw[2 * C:(nb + 1) * 2 * C].view(nb, 2, C))
    st = runs[0]
    assert torch.isfinite(st).all(), (case.name, tile, "a statistics block was not written")
    assert torch.equal(runs[0], runs[1]), (case.name, tile, "statistics differ between two runs")
    want, scale = cc.stats_from_outputs(got_out, M, tile)
    err = ((st - want).abs() / scale.clamp_min(1e-300)).max().item()
    emit("%-10s %s1 stats blocks %d (past M: %d) rel err %.2e" % (case.name, tile, nb, nb - (M + 31) // 32, err))
    assert ((st - want).abs() <= 1e-12 * scale).all(), (case.name, tile, err)
    assert (st[(M + 31) // 32:] == 0).all(), (case.name, tile, "blocks past M are not zero")


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case(dev, name):
    case = cc.CASE[name]
    t0 = time.time()
    d, ref = reference(case)
    t_ref = time.time() - t0
    L = Launch(case, dev)
    results, sharps, fails = {}, {}, []
    for tile, ks in case.plans:
        got = L.launch(tile, ks)
        again = L.launch(tile, ks)
        for k in got:
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (name, tile, ks, k, "two runs differ")
        sharps[(tile, ks)], f = measure(case, ref, got, tile, ks)
        fails += f
        results[(tile, ks)] = got
        if case.stats:
            check_stats(L, case, tile, got["out"])
    assert not fails, fails
    # ---- all plans agree within twice the sharp bound
    nm = ref["named"]
    (p0, g0), worst = next(iter(results.items())), 0.0
    for p, g in results.items():
        for k in g:
            r = ((g[k][nm].double() - g0[k][nm].double()).abs() / (2 * torch.maximum(sharps[p0][k], sharps[p][k])[nm])).max().item()
            worst = max(worst, r)
            assert r <= 1, (name, p0, p, k, r)
    # ---- merged phases = the single-phase launches, bitwise, on every tile
    if case.phase == "merged":
        np_ = cc.nphase(case)
        tpp = len(case.taps) // np_
        for tile, ks in case.plans:
            merged = results[(tile, ks)]["out"]
            for p in range(np_):
                ph = ((p >> 2) & 1 if np_ == 8 else 0, (p >> 1) & 1, p & 1)
                single = L.launch(tile, ks, phase=ph, taps=case.taps[p * tpp:(p + 1) * tpp], wp=L.wp[p * tpp:(p + 1) * tpp].contiguous())["out"]
                rows = cc.out_rows(case, ph)
                assert torch.equal(single[rows].view(torch.int32), merged[rows].view(torch.int32)), (name, tile, ph, "merged != single phase")
                rest = torch.ones(single.shape[0], dtype=torch.bool)
                rest[rows] = False
                assert (single[rest].view(torch.int32) == cc.CANARY).all(), (name, tile, ph, "a single-phase launch wrote another phase's rows")
    emit("%-10s plans %d cross-plan %.2f of 2x sharp, reference %.2f s, case %.2f s" % (name, len(case.plans), worst, t_ref, time.time() - t0))


@pytest.mark.parametrize("name,muts", cc.MUTATION_CASES)
def test_bounds_reject_wrong_references(dev, name, muts):
    """The correct kernel against deliberately wrong references: each must fail the sharp bound. Nothing faulty is launched."""
    case = cc.CASE[name]
    d, ref = reference(case)
    tile, ks = case.plans[0]
    got = Launch(case, dev).launch(tile, ks)
    yard = yardstick(case, YARDSTICK, ks)
    for mut in muts:
        wrong = cc.evaluate(case, d, mut=mut)
        wrong.update(sig_S=ref["sig_S"], sig_A=ref["sig_A"])
        ratios = []
        for k in cc.out_desc(case):
            q, qrms, _ = cc.q_stats(case, wrong, got[k], k)
            ratios.append(max(q / yard[k][0], qrms / yard[k][1]))
        emit("%-10s %s%d wrong reference %-16s q / yardstick %.3g" % (name, tile, ks, mut, max(ratios)))
        assert max(ratios) > cc.SHARP, (name, mut, ratios)


def test_refusals_of_the_contract(dev):
    """The refusals the matrix relies on: FORGE_EINVAL and forge_last_error's text, before any launch. Every call has operands large enough for the launch
    it describes, so a refusal that failed to fire would run a harmless convolution and fail the assertion."""
    lib = _lib.lib()
    buf = lambda nfl: torch.zeros(nfl, dtype=torch.float32, device=dev)
    x, w, o, o2, aux, ws, vec = buf(1 << 14), buf(1 << 16), buf(1 << 16), buf(1 << 16), buf(1 << 16), buf(1 << 18), buf(256)
    st64 = torch.zeros(1 << 12, dtype=torch.float64, device=dev)
    base = dict(C1=32, ld1=32, Cout=96, ldo=96, n=1, D=1, H=4, W=4, ostride=1, ph=(0, 0, 0), og=None, taps=cc.T9, epi=0, lift=0, tile=ord("D"), ksplit=1,
                ws=None, stats=None, aux=False)

    def call(**kw):
        a = dict(base, **kw)
        Do, Ho, Wo = a["og"] or (a["D"], a["H"], a["W"])
        taps = (ctypes.c_int * (3 * len(a["taps"])))(*[v for t in a["taps"] for v in t])
        wsb = 0 if a["ws"] is None else a["ws"].numel() * 4
        rc = lib.forge_conv_igemm(_lib.ptr(x), a["C1"], a["ld1"], 0, None, 0, 0, 0, _lib.ptr(w), _lib.ptr(vec), _lib.ptr(vec), _lib.ptr(vec), 0.0, None,
                                  _lib.ptr(aux) if a["aux"] else None, _lib.ptr(aux) if a["aux"] else None, _lib.ptr(o), _lib.ptr(o2) if a["aux"] else None,
                                  None, a["n"], a["D"], a["H"], a["W"], 1, a["D"], a["H"], a["W"], a["Cout"], a["ldo"], taps, len(a["taps"]), a["ostride"],
                                  a["ph"][0], a["ph"][1], a["ph"][2], Do, Ho, Wo, a["epi"], a["lift"], a["tile"], a["ksplit"], _lib.ptr(a["ws"]), wsb,
                                  _lib.ptr(a["stats"]), _lib.current_stream())
        return rc, lib.forge_last_error()

    with torch.cuda.device(dev):
        for what, kw, text in (
                ("stats with the plan left to the call", dict(stats=st64, tile=0), b"explicit tile"),
                ("stats with split-K", dict(stats=st64, ksplit=2, ws=ws), b"output statistics need"),
                ("GRU gates on the narrow kernel", dict(epi=2, Cout=16, ldo=16, aux=True), b"GRU epilogues need Cout > 16"),
                ("GRU state on the narrow kernel", dict(epi=3, Cout=16, ldo=16, aux=True), b"GRU epilogues need Cout > 16"),
                ("lift on a 3-D grid", dict(epi=1, lift=2, D=2, taps=cc.T27), b"lift needs"),
                ("lift with Cout <= 64", dict(epi=1, lift=2, Cout=64, ldo=64), b"lift needs"),
                ("more K slices than K-steps", dict(taps=cc.T1, ksplit=2, ws=ws), b"ksplit=2 needs"),
                ("merged phases with ntaps % nphase != 0", dict(ostride=2, ph=(-1, -1, -1), og=(1, 8, 8), taps=cc.T9), b"merged phases need ntaps"),
                ("a row stride that breaks the 16-byte alignment", dict(ld1=34), b"row strides must"),
                ("a tap component outside a signed byte", dict(taps=cc.T9[:8] + [(0, 0, 128)]), b"outside [-128, 127]")):
            rc, msg = call(**kw)
            assert rc == -1 and text in msg, (what, rc, msg)
        rc, msg = call()                                              # the baseline itself is a legal launch
        assert rc == 0, msg
        torch.cuda.synchronize()
