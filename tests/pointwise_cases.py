"""The pointwise training kernels and the data movers - csrc/gru.hip, csrc/loss.hip, csrc/stem.hip, csrc/layout.hip - restated in plain torch, one section
per kernel, and their case tables.

tests/test_gpu_pointwise_matrix.py launches every case through the C entry points into canary-guarded buffers; tests/test_pointwise_reference_cpu.py
pins every restatement to an independent one, validates the wrong readings (the MUTATIONS of each section) with the float32 yardstick standing in for
the kernel, and runs the refusals - before a GPU is spent on any of it. Both import this module, so the tables cannot drift between them.

Every restatement returns its outputs IN BUFFER LAYOUT: a tensor per output buffer, NaN wherever the launch must leave the buffer's pattern alone (gap
columns of strided rows, accumulator rows between the batches, channels of a wider tensor). compare() then asks two things of a result: the pattern is
intact exactly where the reference has NaN, and the rest is inside the bound. u = 2^-24; the bounds:
  GRU halves      max |got - ref| <= max(SHARP x the float32 CPU yardstick's error, EPI_ULPS u max(1, |ref|_max)) per output buffer: the yardstick is
                  the same expression in float32 torch on one thread; the floor is conv_igemm_cases' allowance for an epilogue (EPI_ULPS = 16: 4 ulps for
                  each of expf / tanhf / a division / a chain of up to 4 roundings).
  sums of squares relative to the float64 sum: max(SHARP x the yardstick's, EPI_ULPS u).
  Adam, and the gradient through train.grouped_mse (torch scales the upstream gradient there, so it is not bitwise)
                  max |got - ref| <= SHARP x the yardstick's error per buffer, with no floor.
  data movers and two-product kernels (affine_act_bwd, sse_groups_bwd, im2col, max-pool, transposes)   bitwise equal to the float32 CPU evaluation.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_igemm_cases as cc
from rotate_cases import GUARD, finish, guarded, yardstick_threads          # noqa: F401  (re-exported to the two tests)

U, SHARP, CANARY, EPI_ULPS = cc.U, cc.SHARP, cc.CANARY, cc.EPI_ULPS
NAN = float("nan")

# Measured on the MI355X: every line "pointwise_matrix <case> ..." that tests/test_gpu_pointwise_matrix.py prints under -s, as printed. Per output
# buffer: the error, its bound, and (GRU, Adam) its ratio to the float32 CPU yardstick's error.
MEASURED = {
    "g1_c4": "z 2.06e-09 (bound 9.54e-07, 1.00x) | r 4.70e-08 (bound 9.54e-07, 1.00x) | hr 6.92e-08 (bound 1.18e-06, 1.00x) | cand 2.10e-08 (bound 9.54e-07, 1.00x) | hn 5.65e-08 (bound 1.23e-06, 1.00x) | s_dh 2.20e-08 (bound 1.18e-06, 1.00x) | s_dz 7.22e-08 (bound 2.62e-06, 1.00x) | s_dc 7.01e-12 (bound 9.54e-07, 0.00x) | g_dg 4.87e-09 (bound 9.54e-07, 1.00x) | g_dh 1.73e-09 (bound 1.06e-06, 0.06x)",
    "g7_c4": "z 4.67e-08 (bound 9.54e-07, 1.00x) | r 5.58e-08 (bound 9.54e-07, 1.00x) | hr 1.32e-07 (bound 2.31e-06, 1.00x) | cand 3.14e-08 (bound 9.54e-07, 1.10x) | hn 5.53e-08 (bound 2.10e-06, 1.00x) | s_dh 8.52e-08 (bound 1.23e-06, 1.00x) | s_dz 1.06e-07 (bound 2.88e-06, 1.00x) | s_dc 6.08e-09 (bound 9.54e-07, 1.00x) | s_acc 6.89e-08 (bound 2.18e-06, 1.00x) | g_dg 2.91e-08 (bound 9.54e-07, 1.00x) | g_dh_out 5.96e-08 (bound 2.44e-06, 0.77x) | g_acc 1.09e-07 (bound 2.28e-06, 1.00x)",
    "g7_c8": "z 6.80e-08 (bound 9.54e-07, 1.00x) | r 7.07e-08 (bound 9.54e-07, 1.00x) | hr 1.04e-07 (bound 1.94e-06, 1.00x) | cand 3.28e-08 (bound 9.54e-07, 1.17x) | hn 1.05e-07 (bound 1.99e-06, 0.88x) | s_dh 6.42e-08 (bound 2.12e-06, 1.00x) | s_dz 2.36e-07 (bound 5.52e-06, 1.00x) | s_dc 5.37e-08 (bound 1.07e-06, 1.00x) | s_acc 5.37e-08 (bound 1.07e-06, 1.00x) | g_dg 3.26e-08 (bound 9.54e-07, 1.00x) | g_dh_out 8.06e-08 (bound 3.55e-06, 0.51x) | g_acc 3.26e-08 (bound 9.54e-07, 1.00x)",
    "g7_c128": "z 8.52e-08 (bound 9.54e-07, 1.00x) | r 8.31e-08 (bound 9.54e-07, 1.00x) | hr 1.74e-07 (bound 3.41e-06, 1.00x) | cand 4.70e-08 (bound 9.54e-07, 1.57x) | hn 1.59e-07 (bound 2.83e-06, 0.67x) | s_dh 1.57e-07 (bound 2.65e-06, 1.00x) | s_dz 3.78e-07 (bound 6.04e-06, 1.00x) | s_dc 1.67e-07 (bound 2.03e-06, 1.00x) | g_dg 5.16e-08 (bound 1.01e-06, 1.00x) | g_dh 2.38e-07 (bound 3.82e-06, 1.00x)",
    "g1000_c4": "z 8.84e-08 (bound 9.54e-07, 1.00x) | r 8.73e-08 (bound 9.54e-07, 1.00x) | hr 3.40e-07 (bound 3.41e-06, 1.00x) | cand 6.67e-08 (bound 9.54e-07, 2.19x) | hn 1.52e-07 (bound 3.41e-06, 0.55x) | s_dh 1.71e-07 (bound 3.57e-06, 1.00x) | s_dz 5.45e-07 (bound 6.59e-06, 1.00x) | s_dc 1.31e-07 (bound 1.96e-06, 1.00x) | s_acc 1.69e-07 (bound 3.88e-06, 1.00x) | g_dg 1.01e-07 (bound 1.27e-06, 1.00x) | g_dh_out 2.38e-07 (bound 4.43e-06, 1.00x) | g_acc 1.30e-07 (bound 3.65e-06, 1.00x)",
    "g1000_c8": "z 8.66e-08 (bound 9.54e-07, 1.00x) | r 8.50e-08 (bound 9.54e-07, 1.00x) | hr 2.94e-07 (bound 4.08e-06, 1.00x) | cand 5.84e-08 (bound 9.54e-07, 1.95x) | hn 1.96e-07 (bound 3.69e-06, 0.71x) | s_dh 1.67e-07 (bound 3.73e-06, 1.00x) | s_dz 5.81e-07 (bound 1.08e-05, 1.00x) | s_dc 1.29e-07 (bound 2.42e-06, 1.17x) | s_acc 1.29e-07 (bound 2.42e-06, 1.17x) | g_dg 7.29e-08 (bound 1.21e-06, 1.00x) | g_dh_out 2.38e-07 (bound 4.92e-06, 0.81x) | g_acc 7.29e-08 (bound 1.21e-06, 1.00x)",
    "g1_c128": "z 8.22e-08 (bound 9.54e-07, 1.00x) | r 6.39e-08 (bound 9.54e-07, 1.00x) | hr 5.98e-08 (bound 2.21e-06, 1.00x) | cand 3.87e-08 (bound 9.54e-07, 1.33x) | hn 7.42e-08 (bound 2.41e-06, 0.64x) | s_dh 9.08e-08 (bound 1.99e-06, 1.00x) | s_dz 4.20e-07 (bound 6.23e-06, 1.00x) | s_dc 4.14e-08 (bound 9.54e-07, 0.70x) | s_acc 4.14e-08 (bound 9.54e-07, 0.70x) | g_dg 2.12e-08 (bound 1.60e-06, 1.00x) | g_dh_out 1.19e-07 (bound 3.24e-06, 0.93x) | g_acc 2.12e-08 (bound 1.60e-06, 1.00x)",
    "g1000_c128": "z 8.90e-08 (bound 9.54e-07, 1.00x) | r 8.82e-08 (bound 9.54e-07, 1.00x) | hr 3.17e-07 (bound 4.50e-06, 1.00x) | cand 7.52e-08 (bound 9.54e-07, 2.47x) | hn 2.03e-07 (bound 4.35e-06, 0.71x) | s_dh 2.63e-07 (bound 3.92e-06, 1.00x) | s_dz 8.04e-07 (bound 1.09e-05, 1.00x) | s_dc 2.58e-07 (bound 3.18e-06, 1.03x) | s_acc 2.50e-07 (bound 5.24e-06, 0.97x) | g_dg 1.60e-07 (bound 1.76e-06, 1.00x) | g_dh 2.38e-07 (bound 5.57e-06, 0.70x) | g_acc 2.32e-07 (bound 4.34e-06, 1.00x)",
    "a_c1": "affine_act_bwd bitwise: 0 elements differ",
    "a_c3": "affine_act_bwd bitwise: 0 elements differ",
    "a_c8": "affine_act_bwd bitwise: 0 elements differ",
    "a_c16": "affine_act_bwd bitwise: 0 elements differ",
    "a_c16s": "affine_act_bwd bitwise: 0 elements differ",
    "s222": "sse_groups C entry: sums rel 1.66e-08, dpred bitwise yes; grouped_mse: sums rel 1.66e-08 (bound 9.54e-07, yardstick 1.11e-07), gradient 4.79e-09 (bound 1.91e-08)",
    "s422": "sse_groups C entry: sums rel 5.55e-08, dpred bitwise yes; grouped_mse: sums rel 1.18e-07 (bound 9.54e-07, yardstick 1.18e-07), gradient 8.67e-10 (bound 3.47e-09)",
    "s442": "sse_groups C entry: sums rel 2.98e-09, dpred bitwise yes; grouped_mse: sums rel 6.57e-08 (bound 9.54e-07, yardstick 1.49e-08), gradient 1.77e-10 (bound 4.21e-10)",
    "s421": "sse_groups C entry: sums rel 1.46e-08, dpred bitwise yes; grouped_mse: sums rel 9.10e-08 (bound 9.54e-07, yardstick 9.10e-08), gradient 3.18e-10 (bound 1.27e-09)",
    "s632": "sse_groups C entry: sums rel 3.37e-08, dpred bitwise yes; grouped_mse: sums rel 7.51e-08 (bound 9.54e-07, yardstick 9.28e-08), gradient 2.07e-09 (bound 8.29e-09)",
    "s311": "sse_groups C entry: sums rel 1.38e-08, dpred bitwise yes; grouped_mse: sums rel 7.77e-08 (bound 9.54e-07, yardstick 7.45e-08), gradient 2.17e-10 (bound 8.66e-10)",
    "s632g": "sse_groups grouped_mse: sums rel 7.93e-08 (bound 9.54e-07, yardstick 6.43e-08), gradient 5.28e-09 (bound 2.11e-08)",
    "adam n=1": "p 2.49e-08 (bound 9.95e-08, 1.00x) | m 1.84e-08 (bound 7.35e-08, 1.00x) | v 2.40e-10 (bound 9.60e-10, 1.00x)",
    "adam n=255": "p 1.88e-07 (bound 7.54e-07, 1.00x) | m 2.63e-08 (bound 1.05e-07, 1.00x) | v 5.10e-09 (bound 2.04e-08, 1.00x)",
    "adam n=256": "p 2.58e-07 (bound 1.03e-06, 1.00x) | m 3.34e-08 (bound 1.33e-07, 1.00x) | v 1.02e-08 (bound 4.09e-08, 1.00x)",
    "adam n=257": "p 4.95e-07 (bound 1.98e-06, 1.00x) | m 2.98e-08 (bound 1.19e-07, 1.00x) | v 4.89e-09 (bound 1.96e-08, 1.00x)",
    "adam n=1000": "p 2.86e-07 (bound 1.14e-06, 1.00x) | m 3.75e-08 (bound 1.31e-07, 1.14x) | v 1.24e-08 (bound 4.95e-08, 1.00x)",
    "i7": "im2col bitwise: 0 elements differ",
    "i3": "im2col bitwise: 0 elements differ",
    "i3c": "im2col bitwise: 0 elements differ",
    "i_small": "im2col bitwise: 0 elements differ",
    "p3_c4": "maxpool bitwise: True; NaN windows 2 of 2",
    "p3_c64": "maxpool bitwise: True; NaN windows 1 of 1",
    "p2_c4": "maxpool bitwise: True; NaN windows 0 of 0",
    "p2_c64": "maxpool bitwise: True; NaN windows 1 of 1",
    "tr n=1 C=1 P=1": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=3 C=1 P=1": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=1 C=3 P=33": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=3 C=3 P=33": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=1 C=12 P=210": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=3 C=12 P=210": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=1 C=32 P=32": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=3 C=32 P=32": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=1 C=33 P=31": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=3 C=33 P=31": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=1 C=130 P=65": "to_ndhwc, to_ncdhw and the round trip bitwise",
    "tr n=3 C=130 P=65": "to_ndhwc, to_ncdhw and the round trip bitwise",
}


def _seed(name):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))


def f32(v):
    """A float argument as the entry point receives it."""
    return torch.tensor(v, dtype=torch.float32).double().item()


def strided(x, ld, dtype=None):
    """[M][C] -> [M][ld] with NaN gap columns."""
    out = torch.full((x.shape[0], ld), NAN, dtype=dtype or x.dtype)
    out[:, :x.shape[1]] = x
    return out


def bound(ref, yard, floor=True):
    """The arithmetic kernels' bound for one output buffer (module docstring). floor False: SHARP x the yardstick's error and nothing else."""
    nm = ~torch.isnan(ref)
    ey = (yard.double()[nm] - ref[nm]).abs().max().item()
    return max(SHARP * ey, EPI_ULPS * U * max(1.0, ref[nm].abs().max().item()) if floor else 0.0), ey


def compare(got, ref, yard=None, true=None, floor=True):
    """(error, bound, yardstick error, [failures]) of one output buffer in buffer layout. yard None: bitwise against ref (a float32 tensor).
    true: the float64 reference the bound is taken from when `ref` is a deliberately wrong one."""
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return float("inf"), 0.0, 0.0, ["the pattern is not where the contract leaves it: %d elements" % int((torch.isnan(got) != torch.isnan(ref)).sum())]
    nm = ~torch.isnan(ref)
    if yard is None:
        assert ref.dtype == torch.float32 and got.dtype == torch.float32
        bad = int((got[nm].view(torch.int32) != ref[nm].view(torch.int32)).sum())
        return float(bad), 0.0, 0.0, (["%d elements differ bitwise" % bad] if bad else [])
    b, ey = bound(ref if true is None else true, yard, floor)
    e = (got.double()[nm] - ref[nm]).abs().max().item()
    return e, b, ey, (["error %.3e beyond the bound %.3e (yardstick %.3e)" % (e, b, ey)] if not e <= b else [])


def compare_all(got, ref, yard=None, true=None, floor=True):
    """Over a dict of buffers: ({name: (error, bound, yardstick error)}, [failures])."""
    figs, fails = {}, []
    for k in ref:
        e, b, ey, f = compare(got[k], ref[k], None if yard is None else yard[k], None if true is None else true[k], floor)
        figs[k] = (e, b, ey)
        fails += [(k, m) for m in f]
    return figs, fails


# =====================================================================================================================================
# gru.hip: forge_gru_gates_fwd / forge_gru_state_fwd / forge_gru_state_bwd / forge_gru_gates_bwd
#   gates  fwd: z = sigma(g[:, :C]), r = sigma(g[:, C:]), hr = h r            bwd: dg = (dz z (1-z) | dhr h r (1-r)), dh_out = dh + dhr r
#   state  fwd: cand = tanh(c) (stored over c), hn = h (1 - z) + cand z       bwd: dh = dhn (1-z), dz = dhn (cand - h), dc = dhn z (1 - cand^2)
#   accumulator (acc_mode 1 stores, 2 adds): row bi acc_bs + (m - bi vol) of the shared buffer, bi = m / vol, takes dc (state) / dg (gates).
# The backward kernels are fed float32 saved values (z, r, cand as the float32 CPU forward gives them): the reference is the float64 derivative at
# those same values.
GruCase = namedtuple("GruCase", "name M C ld_dhn ld_dhr dh_out acc_mode vol muts note")
# dh_out: None = NULL (dh updated in place), "alias" = the very view dhr is read from, an int = its own row stride
GRU_CASES = [
    GruCase("g1_c4", 1, 4, 4, 4, None, 0, 1, "dz_sign dh_no_dhr", "one float4"),
    GruCase("g7_c4", 7, 4, 8, 4, 8, 2, 7, "acc2_store", "7 float4; one batch of the accumulator"),
    GruCase("g7_c8", 7, 8, 12, 16, "alias", 1, 1, "dz_sign acc_bs_vol", "dhr and dh_out the same strided view; 7 batches of one row, 3 rows apart"),
    GruCase("g7_c128", 7, 128, 128, 132, None, 0, 1, "dh_no_dhr", "224 float4: less than one workgroup"),
    GruCase("g1000_c4", 1000, 4, 8, 4, 12, 2, 250, "dz_sign dh_no_dhr acc2_store acc_bs_vol", "1000 float4: no multiple of 256; 4 batches"),
    GruCase("g1000_c8", 1000, 8, 8, 12, "alias", 1, 500, "acc_bs_vol", "2 batches"),
    GruCase("g1_c128", 1, 128, 132, 128, 136, 1, 1, "dh_no_dhr", ""),
    GruCase("g1000_c128", 1000, 128, 128, 128, None, 2, 200, "acc2_store acc_bs_vol dz_sign", "32000 float4 on 125 workgroups; 5 batches"),
]
GRU_CASE = {c.name: c for c in GRU_CASES}
GRU_MUTATIONS = ("dz_sign", "dh_no_dhr", "acc2_store", "acc_bs_vol")


def gru_data(c):
    """float32 operands. Pre-activations ~ N(0, 6^2) with +-20 planted: sigmoid and tanh saturate."""
    g = _seed(c.name)
    rn = lambda *s: torch.randn(*s, generator=g)
    M, C = c.M, c.C
    gates, cpre = rn(M, 2 * C) * 6, rn(M, C) * 6
    gates.view(-1)[0::7], gates.view(-1)[3::7] = 20.0, -20.0
    cpre.view(-1)[1::5], cpre.view(-1)[2::5] = 20.0, -20.0
    d = {"g": gates.clamp(-20, 20), "c": cpre.clamp(-20, 20), "h": rn(M, C), "dhn": rn(M, C), "dhr": rn(M, C), "dh_in": rn(M, C), "dz_in": rn(M, C)}
    with yardstick_threads():                  # the saved float32 forward values the backward kernels are fed
        d["z"], d["r"], d["cand"] = torch.sigmoid(d["g"][:, :C]), torch.sigmoid(d["g"][:, C:]), torch.tanh(d["c"])
    nb = M // c.vol
    d["acc_rows"] = (nb - 1) * 3 * c.vol + c.vol
    d["prior_c"], d["prior_g"] = rn(d["acc_rows"], C), rn(d["acc_rows"], 2 * C)
    return d


def _acc(c, d, val, prior, mut):
    """The accumulator buffer after the launch: NaN in the rows between the batches."""
    if c.acc_mode == 0:
        return None
    bs = c.vol if mut == "acc_bs_vol" else 3 * c.vol
    m = torch.arange(c.M)
    rows = (m // c.vol) * bs + m % c.vol
    out = torch.full((d["acc_rows"], val.shape[1]), NAN, dtype=val.dtype)
    out[rows] = val + prior.to(val.dtype)[rows] if (c.acc_mode == 2 and mut != "acc2_store") else val
    return out


def gru_eval(c, d, dtype=torch.float64, mut=None):
    """Every output buffer of the four kernels in `dtype`, in buffer layout."""
    assert mut is None or mut in GRU_MUTATIONS
    C = c.C
    t = lambda k: d[k].to(dtype)
    o = {}
    # forward halves, each fed float32 operands
    z, r = torch.sigmoid(t("g")[:, :C]), torch.sigmoid(t("g")[:, C:])
    o["z"], o["r"], o["hr"] = z, r, t("h") * r
    cand = torch.tanh(t("c"))
    o["cand"], o["hn"] = cand, t("h") * (1 - t("z")) + cand * t("z")
    # state backward at the saved values
    zs, rs, cs, h, dhn = t("z"), t("r"), t("cand"), t("h"), t("dhn")
    o["s_dh"], o["s_dz"] = dhn * (1 - zs), dhn * ((h - cs) if mut == "dz_sign" else (cs - h))
    o["s_dc"] = dhn * zs * (1 - cs * cs)
    a = _acc(c, d, o["s_dc"], d["prior_c"], mut)
    if a is not None:
        o["s_acc"] = a
    # gates backward
    dz, dhr = t("dz_in"), t("dhr")
    dg = torch.cat([dz * zs * (1 - zs), dhr * h * rs * (1 - rs)], dim=1)
    dh = t("dh_in") if mut == "dh_no_dhr" else t("dh_in") + dhr * rs
    o["g_dg"] = dg
    if c.dh_out is None:
        o["g_dh"] = dh
    else:
        o["g_dh_out"] = strided(dh, c.ld_dhr if c.dh_out == "alias" else c.dh_out)
    a = _acc(c, d, dg, d["prior_g"], mut)
    if a is not None:
        o["g_acc"] = a
    return o


GRU_REFUSALS = [          # (what, entry point: "s" state_bwd / "g" gates_bwd / "f" the two forwards, changed arguments, code)
    ("C % 4", "fsg", dict(C=6), -2), ("ld < C", "sg", dict(ld=4), -2), ("ld % 4", "sg", dict(ld=10), -2), ("ld_dh_out < C", "g", dict(ld_out=4), -2),
    ("acc_mode 3", "sg", dict(mode=3), -1), ("mode 1 with a NULL buffer", "sg", dict(mode=1, acc=False), -1), ("M % vol != 0", "sg", dict(mode=1, vol=5), -1),
    ("acc_bs < vol", "sg", dict(mode=2, vol=4, bs=3), -1),
]


def gru_refusal_calls(L, p, pout):
    """[(what, rc, code)]; p: a readable pointer, pout: the pointer every output gets."""
    res = []
    for what, eps, kw, code in GRU_REFUSALS:
        a = dict(dict(M=8, C=8, ld=8, ld_out=8, mode=0, acc=True, vol=4, bs=12), **kw)
        acc = pout if a["acc"] else None
        if "f" in eps:
            res.append((what + " (gates_fwd)", L.forge_gru_gates_fwd(p, p, pout, pout, pout, a["M"], a["C"], None), code))
            res.append((what + " (state_fwd)", L.forge_gru_state_fwd(pout, p, p, pout, a["M"], a["C"], None), code))
        if "s" in eps:
            res.append((what + " (state_bwd)", L.forge_gru_state_bwd(p, a["ld"], p, p, p, pout, pout, pout, a["M"], a["C"], acc, a["bs"], a["vol"], a["mode"], None), code))
        if "g" in eps:
            res.append((what + " (gates_bwd)", L.forge_gru_gates_bwd(p, p, a["ld"], p, p, p, pout, pout, pout, a["ld_out"], a["M"], a["C"], acc, a["bs"], a["vol"],
                                                                      a["mode"], None), code))
    return res


# =====================================================================================================================================
# gru.hip: forge_affine_act_bwd    dx = dy * scale[c] * (y > 0 ? 1 : slope); two float32 products: bitwise. A zero of either sign takes the slope side.
AffCase = namedtuple("AffCase", "name M C ld_dy ld_y ld_dx scale slope inplace muts")
AFF_CASES = [
    AffCase("a_c1", 37, 1, 3, 2, 5, False, 0.0, False, "zero_pos"),
    AffCase("a_c3", 300, 3, 4, 7, 3, True, 0.01, False, "zero_pos no_scale"),
    AffCase("a_c8", 37, 8, 12, 8, 12, True, 1.0, True, "no_scale"),
    AffCase("a_c16", 300, 16, 20, 24, 20, False, 0.01, True, "zero_pos"),
    AffCase("a_c16s", 37, 16, 16, 16, 16, True, 0.0, False, "zero_pos no_scale"),
]
AFF_CASE = {c.name: c for c in AFF_CASES}
AFF_MUTATIONS = ("zero_pos", "no_scale")
DENORM = 2.0 ** -149


def aff_data(c):
    g = _seed(c.name)
    y = torch.randn(c.M, c.C, generator=g)
    y.view(-1)[0], y.view(-1)[1], y.view(-1)[2] = 0.0, -0.0, DENORM            # known places: +0 and -0 take the slope side, the denormal does not
    y.view(-1)[5::11] = 0.0
    return {"dy": torch.randn(c.M, c.C, generator=g), "y": y, "scale": torch.rand(c.C, generator=g) + 0.5 if c.scale else None}


def aff_eval(c, d, mut=None):
    """{"dx": [M][ld_dx] float32}: the two products in float32."""
    g = d["dy"] * d["scale"] if (d["scale"] is not None and mut != "no_scale") else d["dy"].clone()
    pos = d["y"] >= 0 if mut == "zero_pos" else d["y"] > 0
    return {"dx": strided(torch.where(pos, g, g * torch.tensor(c.slope, dtype=torch.float32)), c.ld_dx)}


# =====================================================================================================================================
# loss.hip: forge_sse_groups_fwd / _bwd   rendered view v of scene b <-> target view v % Vt, group v / gsize;
#   sums[g] = sum (pred - target)^2 over the group; dpred = coef[g] (pred - target) in pred's own layout
SseCase = namedtuple("SseCase", "name B Vp Vt gsize C H W layout muts")
# layout: "contig", "cl" (channels-last memory behind the NCHW view), "slice" (channels [1, 1 + C) of a C + 3 wide tensor),
#         "batch_gap" (views [0, Vp) of a Vp + 1 view stack: stride(0) != Vp stride(1), grouped_mse's contiguous fallback; through grouped_mse only)
SSE_CASES = [
    SseCase("s222", 1, 2, 2, 2, 1, 5, 7, "contig", ""),
    SseCase("s422", 2, 4, 2, 2, 3, 5, 7, "cl", "g_mod contig_strides"),
    SseCase("s442", 1, 4, 4, 2, 3, 33, 65, "slice", "vt_gsize g_mod"),
    SseCase("s421", 2, 4, 2, 1, 1, 33, 65, "cl", "vt_gsize"),
    SseCase("s632", 1, 6, 3, 2, 3, 5, 7, "contig", "vt_gsize g_mod"),
    SseCase("s311", 2, 3, 1, 1, 3, 33, 65, "cl", "contig_strides"),
    SseCase("s632g", 2, 6, 3, 2, 1, 5, 7, "batch_gap", ""),
]
SSE_CASE = {c.name: c for c in SSE_CASES}
SSE_MUTATIONS = ("vt_gsize", "g_mod", "contig_strides")


def sse_data(c):
    """pred as a view of `base` (the buffer the backward's pattern is checked on), target, coef."""
    g = _seed(c.name)
    rn = lambda *s: torch.randn(*s, generator=g)
    B, Vp, C, H, W = c.B, c.Vp, c.C, c.H, c.W
    if c.layout == "contig":
        base = rn(B, Vp, C, H, W)
        pred = base
    elif c.layout == "cl":
        base = rn(B, Vp, H, W, C)
        pred = base.permute(0, 1, 4, 2, 3)
    elif c.layout == "slice":
        base = rn(B, Vp, C + 3, H, W)
        pred = base[:, :, 1:1 + C]
    else:
        base = rn(B, Vp + 1, C, H, W)
        pred = base[:, :Vp]
    return {"base": base, "pred": pred, "target": rn(B, c.Vt, C, H, W), "coef": rn(Vp // c.gsize)}


def sse_view(c, base):
    """pred as a view of a buffer shaped like sse_data's base."""
    return {"contig": lambda b: b, "cl": lambda b: b.permute(0, 1, 4, 2, 3), "slice": lambda b: b[:, :, 1:1 + c.C], "batch_gap": lambda b: b[:, :c.Vp]}[c.layout](base)


def sse_eval(c, d, dtype=torch.float64, mut=None):
    """{"sums": [G], "dpred": base-shaped, NaN where pred does not live} - view by view, as the kernel's comment maps them."""
    assert mut is None or mut in SSE_MUTATIONS
    G = c.Vp // c.gsize
    pred = d["pred"]
    if mut == "contig_strides":                 # the memory read as if it were plain NCHW
        pred = d["base"].contiguous().view(-1)[:pred.numel()].view(pred.shape)
    pred, target = pred.to(dtype), d["target"].to(dtype)
    sums = torch.zeros(G, dtype=dtype)
    dbase = torch.full(d["base"].shape, NAN, dtype=dtype)
    dp = sse_view(c, dbase)
    for v in range(c.Vp):
        g = v % G if mut == "g_mod" else v // c.gsize
        vt = v % c.gsize if mut == "vt_gsize" else v % c.Vt
        diff = pred[:, v] - target[:, vt]
        sums[g] = sums[g] + diff.square().sum()
        dp[:, v] = d["coef"].to(dtype)[g] * diff
    return {"sums": sums, "dpred": dbase}


def sse_mse(c, d):
    """What grouped_mse documents: [F.mse_loss(pred[:, g gsize:(g + 1) gsize], the target views (g gsize + j) % Vt) for g], float64."""
    pred, target = d["pred"].double(), d["target"].double()
    out = []
    for g in range(c.Vp // c.gsize):
        idx = [(g * c.gsize + j) % c.Vt for j in range(c.gsize)]
        out.append(F.mse_loss(pred[:, g * c.gsize:(g + 1) * c.gsize], target[:, idx]))
    return torch.stack(out)


def sse_bound(ref, yard):
    """Relative to the float64 sums (all terms are non-negative): SHARP x the yardstick's, at least EPI_ULPS u."""
    return max(SHARP * ((yard.double() - ref).abs() / ref).max().item(), EPI_ULPS * U)


# =====================================================================================================================================
# loss.hip: forge_adam_small   k = step + 1; m = m + (g - m)(1 - b1); v = v b2 + (1 - b2) g^2; p -= lr / (1 - b1^k) * m / (sqrt(v) / sqrt(1 - b2^k) + eps)
ADAM_N = (1, 255, 256, 257, 1000)
ADAM_HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)
ADAM_STEP0, ADAM_STEPS = 5.0, 3
ADAM_MUTATIONS = ("stale_step",)


def adam_data(n):
    g = _seed("adam%d" % n)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"p": rn(n), "m": rn(n) * 0.1, "v": rn(n).square() * 0.01, "grads": [rn(n) for _ in range(ADAM_STEPS)]}


def adam_eval(d, dtype=torch.float64, mut=None):
    """{"p", "m", "v"} after ADAM_STEPS steps from step count ADAM_STEP0, the hyper-parameters as the floats the entry point receives."""
    lr, b1, b2, eps = (torch.tensor(f32(ADAM_HYPER[k]), dtype=dtype) for k in ("lr", "b1", "b2", "eps"))
    p, m, v = d["p"].to(dtype), d["m"].to(dtype), d["v"].to(dtype)
    k = ADAM_STEP0
    for g in d["grads"]:
        g = g.to(dtype)
        k += 1
        kk = torch.tensor(k - 1 if mut == "stale_step" else k, dtype=dtype)
        m = m + (g - m) * (1 - b1)
        v = v * b2 + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** kk) * (m / (v.sqrt() / (1 - b2 ** kk).sqrt() + eps))
    return {"p": p, "m": m, "v": v}


# =====================================================================================================================================
# stem.hip: forge_im2col_nchw   rows [n Ho Wo][Kpad], k = (ky kw + kx) C + c, zero outside the image and for k >= kh kw C
ColCase = namedtuple("ColCase", "name N C H W k stride pad Kpad muts")
COL_CASES = [
    ColCase("i7", 2, 3, 9, 11, 7, 2, 3, 160, "c_major no_pad_cols"),
    ColCase("i3", 2, 1, 9, 11, 3, 1, 1, 9, "xy_swap"),
    ColCase("i3c", 1, 3, 6, 5, 3, 1, 1, 32, "c_major xy_swap"),
    ColCase("i_small", 1, 3, 5, 4, 7, 2, 3, 147, "c_major"),
]
COL_CASE = {c.name: c for c in COL_CASES}
COL_MUTATIONS = ("c_major", "xy_swap", "no_pad_cols")


def col_out(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def col_data(c):
    return {"img": torch.randn(c.N, c.C, c.H, c.W, generator=_seed(c.name))}


def col_eval(c, d, mut=None):
    """{"out": [N Ho Wo][Kpad] float32} by indexing the zero-padded image."""
    Ho, Wo = col_out(c)
    img = F.pad(d["img"], (c.pad, c.pad, c.pad, c.pad))
    out = torch.full((c.N, Ho, Wo, c.Kpad), NAN if mut == "no_pad_cols" else 0.0)
    oy, ox = torch.arange(Ho) * c.stride, torch.arange(Wo) * c.stride
    for ky in range(c.k):
        for kx in range(c.k):
            for ch in range(c.C):
                col = ch * c.k * c.k + ky * c.k + kx if mut == "c_major" else ((kx * c.k + ky) if mut == "xy_swap" else (ky * c.k + kx)) * c.C + ch
                out[:, :, :, col] = img[:, ch][:, oy + ky][:, :, ox + kx]
    return {"out": out.reshape(c.N * Ho * Wo, c.Kpad)}


def col_unfold(c, d):
    """The same matrix from F.unfold (whose columns are channel-major)."""
    Ho, Wo = col_out(c)
    u = F.unfold(d["img"], c.k, padding=c.pad, stride=c.stride).view(c.N, c.C, c.k * c.k, Ho * Wo).permute(0, 3, 2, 1).reshape(c.N * Ho * Wo, c.k * c.k * c.C)
    return torch.cat([u, torch.zeros(u.shape[0], c.Kpad - u.shape[1])], dim=1)


# =====================================================================================================================================
# stem.hip: forge_maxpool2d_nhwc   -inf padding; a NaN in a window is that window's result (nn.MaxPool2d)
PoolCase = namedtuple("PoolCase", "name N H W C k stride pad nan muts")
POOL_CASES = [
    PoolCase("p3_c4", 2, 7, 9, 4, 3, 2, 1, (1, 3, 4, 2), "zero_init fmax"),
    PoolCase("p3_c64", 1, 9, 7, 64, 3, 2, 1, (0, 8, 6, 63), "zero_init fmax"),                 # the NaN in the last corner: one window
    PoolCase("p2_c4", 2, 7, 9, 4, 2, 2, 0, (0, 6, 2, 1), "zero_init"),                         # odd H: row 6 is in no window: the NaN appears nowhere
    PoolCase("p2_c64", 1, 5, 11, 64, 2, 2, 0, (0, 2, 3, 17), "zero_init fmax"),
]
POOL_CASE = {c.name: c for c in POOL_CASES}
POOL_MUTATIONS = ("zero_init", "fmax")


def pool_data(c):
    """All-negative inputs with -inf entries and one NaN at c.nan = (n, y, x, channel)."""
    g = _seed(c.name)
    x = -torch.rand(c.N, c.H, c.W, c.C, generator=g) - 0.5
    x.view(-1)[3::13] = float("-inf")
    x[c.nan] = NAN
    return {"x": x}


def pool_eval(c, d, mut=None):
    """{"out": [N][Ho][Wo][C] float32} as F.max_pool2d places it. The reference has real NaNs: compare with pool_equal."""
    x = d["x"].permute(0, 3, 1, 2)
    if mut == "fmax":
        x = x.nan_to_num(nan=float("-inf"))
    out = F.max_pool2d(x, c.k, c.stride, c.pad).permute(0, 2, 3, 1).contiguous()
    return {"out": out.clamp_min(0.0) if mut == "zero_init" else out}


def pool_windows(c, d):
    """The same by explicit windows over the -inf padded input; also the number of windows that hold the NaN."""
    x = F.pad(d["x"], (0, 0, c.pad, c.pad, c.pad, c.pad), value=float("-inf"))
    Ho, Wo = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    out = torch.empty(c.N, Ho, Wo, c.C)
    for oy in range(Ho):
        for ox in range(Wo):
            out[:, oy, ox] = x[:, oy * c.stride:oy * c.stride + c.k, ox * c.stride:ox * c.stride + c.k].reshape(c.N, -1, c.C).amax(1)
    _, ny, nx, _ = c.nan
    hit = sum(1 for oy in range(Ho) for ox in range(Wo)
              if oy * c.stride - c.pad <= ny < oy * c.stride - c.pad + c.k and ox * c.stride - c.pad <= nx < ox * c.stride - c.pad + c.k)
    return out, hit


def pool_equal(got, ref):
    """Bitwise where the reference is a number, a NaN exactly where it is one."""
    nan = torch.isnan(ref)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan].view(torch.int32), ref[~nan].view(torch.int32))


# =====================================================================================================================================
# layout.hip: forge_ncdhw_to_ndhwc  src [n][C][P] -> dst [n][P][C];  forge_ndhwc_to_ncdhw the inverse (32 x 32 tiles)
TR_SHAPES = [(1, 1), (3, 33), (12, 210), (32, 32), (33, 31), (130, 65)]
TR_N = (1, 3)
TR_MUTATIONS = ("no_batch_stride",)


def tr_data(n, C, P):
    return torch.randn(n, C, P, generator=_seed("tr%d_%d_%d" % (n, C, P)))


def tr_eval(x, mut=None):
    """[n][R][Cc] -> [n][Cc][R]."""
    if mut == "no_batch_stride":
        return x[:1].expand_as(x).transpose(1, 2).contiguous()
    return x.transpose(1, 2).contiguous()


# =====================================================================================================================================
def other_refusal_calls(L, p, pout):
    """The refusals of every entry point of this module but the GRU ones: [(what, rc, code)]; p: a readable pointer, pout: the pointer every output
    gets. Each call is refused on its sizes (or a NULL) before anything is launched."""
    sse = lambda fn, *tail: fn(p, 35, 35, 7, 1, p, *tail)
    dims = lambda Vp, Vt, gs: (1, Vp, Vt, gs, 1, 5, 7, None)
    return [
        ("affine_act_bwd ld_dy < C", L.forge_affine_act_bwd(p, 4, p, 8, None, 0.0, pout, 8, 8, 8, None), -2),
        ("affine_act_bwd ld_dx < C", L.forge_affine_act_bwd(p, 8, p, 8, None, 0.0, pout, 7, 8, 8, None), -2),
        ("affine_act_bwd NULL y", L.forge_affine_act_bwd(p, 8, None, 8, None, 0.0, pout, 8, 8, 8, None), -1),
        ("sse_groups_fwd 5 groups", sse(L.forge_sse_groups_fwd, pout, *dims(5, 1, 1)), -2),
        ("sse_groups_bwd 5 groups", sse(L.forge_sse_groups_bwd, p, pout, *dims(5, 5, 1)), -2),
        ("sse_groups_fwd Vp % Vt != 0", sse(L.forge_sse_groups_fwd, pout, *dims(4, 3, 2)), -2),
        ("sse_groups_bwd Vp % Vt != 0", sse(L.forge_sse_groups_bwd, p, pout, *dims(4, 3, 2)), -2),
        ("sse_groups_fwd NULL partial", sse(L.forge_sse_groups_fwd, None, *dims(4, 2, 2)), -1),
        ("sse_groups_bwd NULL coef", sse(L.forge_sse_groups_bwd, None, pout, *dims(4, 2, 2)), -1),
        ("adam_small n = 2^20 + 1", L.forge_adam_small(pout, p, pout, pout, pout, (1 << 20) + 1, 0.01, 0.9, 0.999, 1e-8, None), -2),
        ("maxpool C % 4", L.forge_maxpool2d_nhwc(p, pout, 1, 7, 9, 6, 3, 2, 1, None), -1),
        ("maxpool 2 pad > k", L.forge_maxpool2d_nhwc(p, pout, 1, 7, 9, 4, 3, 2, 2, None), -1),
        ("im2col Kpad < kh kw C", L.forge_im2col_nchw(p, pout, 1, 3, 9, 11, 7, 7, 2, 3, 146, None), -1),
        ("ndhwc_to_ncdhw P / 32 = 65535", L.forge_ndhwc_to_ncdhw(p, pout, 1, 4, 65535 * 32, None), -2),
    ]
