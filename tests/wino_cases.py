"""The contract of the Winograd F(2x2, 3x3) x depth-tap entry points (forge_wino_*), stage by stage, in plain torch - and the case table.

Written from the header blocks above forge_wino_weights / forge_wino_wgrad_det in include/forge_hip.h, not from the kernels. tests/test_gpu_wino_matrix.py
launches every case of CASES stage by stage and measures it against these functions; tests/test_wino_reference_cpu.py pins their composition to
F.conv3d / F.conv2d and autograd in float64, checks the coverage rows and validates the wrong references (MUTATIONS) before a GPU is spent on them.
The matrices B^T, G, A^T live here; tests/test_winograd_math.py imports them.

Every stage function takes a dtype. In float64 it is the reference; in float32 it performs the stage's additions in the order the header documents (row
stage first, then the column stage; (a + b) + c; the point GEMM as one fused multiply-add per k, taps outer, channels inner) and is the exact stage / the
yardstick. With mag=True the same linear map is applied with absolute coefficients to absolute operands: the magnitude sum that gives every bound a scale.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u), k = the roundings on the longest path of the stage, true of any fp32 evaluation in any order):
  input, nsum > 1   k = nsum + 3: nsum - 1 additions of views, the reciprocal, the multiplication, two levels of transform additions
  point GEMM        k = kd (C1 + C2) + 2
  output            k = k_out(case): the roundings the magnitude sum S is carried through - 2 + 2 additions of the two transform stages, then one each for
                    what the case has: Mm2, bias, residual, the fmaf of epilogue 1, its slope multiplication (slope not 0 or 1). At most 9; the issue words it as
                    "4 + 1 for Mm2 + the tail's budget" - the tail's share is counted here operation by operation instead of granted. What the tail adds or
                    evaluates itself (shift, residual, expf, tanhf, h (1 - z), the fmaf of out2) gets EPI_ULPS 2 u of its own magnitude sigma_A, as in conv_igemm_cases
  wgrad             k = R + 2 (R = n D Ht Wt products per element, summed in any order over chunks)
  dw                k = 5: u1 + u2 | + u0 (row stage, 2), the same in the column stage (2), the accumulation onto the prior (1); the factors 1/2 are exact
The GRU epilogues 2 / 3 and their sigma rules are conv_igemm_cases.gru_tail, the one statement both matrices call; epilogues 0 / 1 are this file's own
branch, because here the residual comes first: v = y + bias + residual, out = lrelu(v scale + shift).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_igemm_cases as cc
from conv_igemm_cases import ALL_TILES, CANARY, EPI_ULPS, SHARP, U  # noqa: F401  (one family: the same constants)

BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1.]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1.]], dtype=torch.float64)

K_DW = 5


def gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------------------------------- stages
def _bt(a, mag):
    """B^T applied along one axis of four operands: (a0 - a2, a1 + a2, a2 - a1, a1 - a3)."""
    if mag:
        return [a[0] + a[2], a[1] + a[2], a[2] + a[1], a[1] + a[3]]
    return [a[0] - a[2], a[1] + a[2], a[2] - a[1], a[1] - a[3]]


def _a(y, mag):
    """A = (A^T)^T applied along one axis of two operands: (y0, y0 + y1, y0 - y1, -y1)."""
    if mag:
        return [y[0], y[0] + y[1], y[0] + y[1], y[1]]
    return [y[0], y[0] + y[1], y[0] - y[1], 0 - y[1]]


def _at(m, mag, flip=False):
    """A^T applied along one axis of four operands: ((m0 + m1) + m2, (m1 - m2) - m3). flip: the wrong reference with + m3."""
    if mag:
        return [(m[0] + m[1]) + m[2], (m[1] + m[2]) + m[3]]
    return [(m[0] + m[1]) + m[2], ((m[1] - m[2]) + m[3]) if flip else ((m[1] - m[2]) - m[3])]


def input_transform(x, nsum=1, dtype=torch.float64, mag=False, mut=None):
    """x [n][D][H][W][C] (nsum > 1: [nsum][n][D][H][W][C], the views whose mean is transformed) -> V [16][R][C], V[4 i + j][r] = (B^T d B)[i][j] of the
    4 x 4 patch d at rows 2 th - 1 .., cols 2 tw - 1 .., zero outside the plane, r = ((n D + z) Ht + th) Wt + tw."""
    x = x.to(dtype)
    if mag:
        x = x.abs()
    if nsum > 1:
        v = x[0]
        for k in range(1, nsum):
            v = v + x[k]
        x = v * (torch.ones((), dtype=dtype) / nsum)          # the kernel multiplies by the reciprocal in its own precision
    n, D, H, W, C = x.shape
    Ht, Wt = H // 2, W // 2
    o = 1 if mut == "origin_2th" else 0
    xp = F.pad(x, (0, 0, 1, 2, 1, 2))
    d = [[xp[:, :, i + o:i + o + 2 * Ht:2, j + o:j + o + 2 * Wt:2].reshape(-1, C) for j in range(4)] for i in range(4)]
    w = [_bt([d[i][j] for i in range(4)], mag) for j in range(4)]                 # w[j][i]: rows B^T d
    v = [_bt([w[j][i] for j in range(4)], mag) for i in range(4)]                 # v[i][j]: columns (B^T d) B
    if mut == "pt_transposed":
        return torch.stack([v[i][j] for j in range(4) for i in range(4)])
    return torch.stack([v[i][j] for i in range(4) for j in range(4)])


def dy_transform(dy, dtype=torch.float64, mag=False):
    """dy [n][D][H][W][C] -> dM [16][R][C] = A y A^T of each tile's own 2 x 2 pixels (the adjoint of the inverse transform), rows first."""
    dy = dy.to(dtype)
    if mag:
        dy = dy.abs()
    C = dy.shape[-1]
    y = [[dy[:, :, i::2, j::2].reshape(-1, C) for j in range(2)] for i in range(2)]
    s = [_a([y[0][j], y[1][j]], mag) for j in range(2)]                           # s[j][i]
    m = [_a([s[0][i], s[1][i]], mag) for i in range(4)]                           # m[i][j]
    return torch.stack([m[i][j] for i in range(4) for j in range(4)])


def weights(wp, kd, transpose=False, dtype=torch.float64, mag=False):
    """wp [9 kd][Cout][Cin] -> U [16][kd][Cout][Cin] = G w[kd] G^T; transpose: the data gradient's U [16][kd][Cin][Cout] from
    w'[kd][a][b][ci][co] = wp[(kd - 1 - k, 2 - a, 2 - b)][co][ci]. Evaluated in float64; dtype float32 rounds the result once."""
    _, Co, Ci = wp.shape
    w = wp.double().reshape(kd, 3, 3, Co, Ci)
    if transpose:
        w = w.flip(0, 1, 2).transpose(3, 4)
    g = G.abs() if mag else G
    u = torch.einsum("ia,jb,kaboc->ijkoc", g, g, w.abs() if mag else w)
    return u.reshape(16, kd, u.shape[3], u.shape[4]).to(dtype)


def _depth_shift(Vv, dz, cross):
    """Vv [16][n][D][rows][C] -> the operand of depth tap dz: plane z + dz of the SAME batch element, zero outside; cross: the wrong reference that walks
    the flattened (n, D) axis."""
    if dz == 0:
        return Vv
    P, n, D, rows, C = Vv.shape
    flat = Vv.reshape(P, n * D, rows, C) if cross else Vv.reshape(P * n, D, rows, C)
    out = torch.zeros_like(flat)
    if flat.shape[1] > abs(dz):
        if dz > 0:
            out[:, :-dz] = flat[:, dz:]
        else:
            out[:, -dz:] = flat[:, :dz]
    return out.reshape(Vv.shape)


def point_gemm(V, Uw, grid, dtype=torch.float64, grain="tap", mag=False, mut=None):
    """V [16][R][Cin] (the channel concatenation V1 | V2), Uw [16][kd][Cout][Cin], grid = (n, D, Ht, Wt) -> Mm [16][R][Cout]:
    Mm[p][r][co] = sum_kd sum_ci Uw[p][kd][co][ci] V[p][r + (kd - 1) plane][ci], depth taps -1, 0, +1 inside a batch element (kd = 1: the plane itself).
    grain 'tap': one batched matmul per tap; 'chain': one fused multiply-add per k, taps outer, channels inner (the float32 yardstick)."""
    n, D, Ht, Wt = grid
    kd, Cout, Cin = Uw.shape[1:]
    V, Uw = V.to(dtype), Uw.to(dtype)
    if mag:
        V, Uw = V.abs(), Uw.abs()
    Vv = V.reshape(16, n, D, Ht * Wt, Cin)
    acc = torch.zeros(16, V.shape[1], Cout, dtype=dtype)
    for t in range(kd):
        dz = (t - 1) if kd == 3 else 0
        X = _depth_shift(Vv, -dz if mut == "tap_sign" else dz, mut == "tap_cross_batch").reshape(16, -1, Cin)
        w = Uw[:, t]
        if mut == "drop_last_k" and t == kd - 1:
            w = w.clone()
            w[:, :, Cin - 32:] = 0
        if grain == "chain":
            for k in range(Cin):
                acc = (X[:, :, k, None].double() * w[:, None, :, k].double() + acc.double()).to(dtype)
        else:
            acc = acc + X @ w.transpose(1, 2)
    return acc


def row_combine(Mm, mag=False, flip=False):
    """The 16 point products -> the 8 planes [2][4] forge_wino_gemm_half stores: s[i'][j] = (A^T m)[i'][j] over the point index i."""
    s = _at([Mm[0:4], Mm[4:8], Mm[8:12], Mm[12:16]], mag, flip)
    return torch.cat(s)


def inverse_transform(Mm, Mm2, grid, dtype=torch.float64, mag=False, mut=None):
    """Mm [16 | 8][R][C] (+ Mm2 in the same form) -> y rows [n D H W][C] = A^T (Mm + Mm2) A per tile. 16 planes: m + m2 first, then rows, then columns;
    8 planes: the row stage is in the operands, s + s2, then columns."""
    n, D, Ht, Wt = grid
    m = Mm.to(dtype)
    if mag:
        m = m.abs()
    if Mm2 is not None:
        m = m + (Mm2.to(dtype).abs() if mag else Mm2.to(dtype))
    s = m if m.shape[0] == 8 else row_combine(m, mag, mut == "s1_sign")
    C = s.shape[-1]
    y = [_at([s[4 * i + j] for j in range(4)], mag) for i in range(2)]             # y[i][j]
    Y = torch.stack([torch.stack(y[i], dim=-2) for i in range(2)], dim=1)          # [R][i][j][C]
    return Y.reshape(n, D, Ht, Wt, 2, 2, C).permute(0, 1, 2, 4, 3, 5, 6).reshape(-1, C)


def wgrad_points(dM, V, grid, kd, dtype=torch.float64, grain="tap", mag=False):
    """dM [16][R][Cout], V [16][R][Cin] -> dU [16][kd][Cout][Cin] = sum_r dM[p][r][co] V[p][r + (kd - 1) plane][ci]. grain 'chain': one fused
    multiply-add per tile row r, in row order."""
    n, D, Ht, Wt = grid
    dM, V = dM.to(dtype), V.to(dtype)
    if mag:
        dM, V = dM.abs(), V.abs()
    Vv = V.reshape(16, n, D, Ht * Wt, V.shape[-1])
    out = []
    for t in range(kd):
        X = _depth_shift(Vv, (t - 1) if kd == 3 else 0, False).reshape(16, -1, V.shape[-1])
        if grain == "chain":
            acc = torch.zeros(16, dM.shape[-1], V.shape[-1], dtype=dtype)
            for r in range(X.shape[1]):
                acc = (dM[:, r, :, None].double() * X[:, r, None, :].double() + acc.double()).to(dtype)
            out.append(acc)
        else:
            out.append(dM.transpose(1, 2) @ X)
    return torch.stack(out, dim=1)


def dw_transform(dU, prior, dtype=torch.float64, mag=False, mut=None):
    """dU [16][kd][Cout][Cin], prior dw [9 kd][Cout][Cin] -> prior + G^T dU G: rows first, g0 = u0 + (u1 + u2) / 2, g1 = (u1 - u2) / 2,
    g2 = (u1 + u2) / 2 + u3, the same over j, then one addition onto the prior (5 roundings)."""
    kd = dU.shape[1]
    u = dU.to(dtype)
    p = prior.to(dtype)
    if mag:
        u, p = u.abs(), p.abs()
    sgn = 1.0 if mag else -1.0

    def gt(a):
        if mut == "dw_g_swap":                                                    # rows 1 and 2 of G exchanged
            a = [a[0], a[2], a[1], a[3]]
        return [a[0] + 0.5 * (a[1] + a[2]), 0.5 * (a[1] + sgn * a[2]), 0.5 * (a[1] + a[2]) + a[3]]
    g = [gt([u[4 * i + j] for i in range(4)]) for j in range(4)]                   # g[j][a]
    o = [gt([g[j][a] for j in range(4)]) for a in range(3)]                        # o[a][b]  [kd][Cout][Cin]
    d = torch.stack([torch.stack(o[a], dim=1) for a in range(3)], dim=1)           # [kd][a][b][Cout][Cin]
    return p + d.reshape(9 * kd, *d.shape[3:])


def tail(y, S, case, d, dtype=torch.float64, mut=None):
    """The element-wise tail on the inverse-transformed rows y (S: their magnitude sum, None for a float32 evaluation). Returns ({out, out2, out3}, sig_S,
    sig_A). v = y + bias + residual in every epilogue; 0: v; 1: lrelu(v scale + shift); 2 / 3: forge_conv_igemm's GRU gates / state on v."""
    cv = lambda t: None if t is None else t.to(dtype)
    bias, scale, shift, res, h, z = (cv(d.get(k)) for k in ("bias", "scale", "shift", "residual", "aux_h", "aux_z"))
    want = S is not None
    v = y if bias is None else y + bias
    if want and bias is not None:
        S = S + bias.abs()
    late = res is not None and mut == "res_after"
    if res is not None and not late and case.epi < 2:
        v = v + res
    rA = (res.abs() if res is not None else torch.zeros((), dtype=dtype)) + torch.zeros_like(v)
    o, sS, sA = {}, {}, {}
    if case.epi == 0:
        o["out"] = v
        if want:
            sS["out"], sA["out"] = S, rA
    elif case.epi == 1:
        t = v * scale + shift
        if late:
            t = t + res
        o["out"] = torch.where(t > 0, t, t * case.slope)
        if want:
            L = max(1.0, abs(case.slope))
            sS["out"], sA["out"] = L * scale.abs() * S, L * (scale.abs() * rA + shift.abs())
    else:                                                       # the GRU epilogues: conv_igemm_cases' statement, for both kernels (it adds the residual)
        o, sS, sA = cc.gru_tail(case.epi, v, S, res, h, z, scale, shift, case.out2)
    keep = out_names(case)
    return {k: o[k] for k in keep}, ({k: sS[k] for k in keep} if want else None), ({k: sA[k] for k in keep} if want else None)


# ---------------------------------------------------------------------------------------------------------------- the case table
_FIELDS = ("name rows n D H W C1 C2 Cout kd epi slope bias residual out2 out3 mm2 tiles gviews ld1 off1 views1 ld2 off2 vcat ldo nsum dgrad wgrad dy_ld big note")
Case = namedtuple("Case", _FIELDS)
_DEFAULTS = dict(C2=0, kd=3, epi=0, slope=1.0, bias=True, residual=False, out2=False, out3=False, mm2=None, tiles=(), gviews=None, ld1=None, off1=0, views1=None,
                 ld2=None, off2=0, vcat=0, ldo=None, nsum=1, dgrad=False, wgrad=None, dy_ld=None, big=False, note="")


def mk(name, rows, n, D, H, W, C1, Cout, **kw):
    """mm2 = (views, view): a second addend with `views` views per batch element, this launch adds view `view`. tiles: the forced tiles of forge_wino_gemm
    besides the rule's own. gviews = (views, view): the GEMMs read V1 as view `view` of a [n][views] stack of transformed inputs (bs1 = views x
    the volume's tile rows, pt1 = the whole stack; the other views' rows NaN), as convops.wino_gemm feeds them in the product. ld1 / off1 / views1 (ld2 / off2): x1 (x2) as a channel slice at column off of rows of ld floats, view ti of a [n][tv] stack.
    vcat = g > 0: V1 and V2 are written into ONE buffer of rows of C1 + C2 + g floats whose point planes lie g floats apart (ldv > C, ptv not dense) and the
    GEMM reads them from there (ld1 = ld2 > C, pt1 = pt2 not dense). dgrad: the launch is the data gradient (U from forge_wino_weights' transposed
    form; Cout of the case = the convolution's input channels). wgrad = (views, view) or (): the weight gradient of the case's convolution runs too, V1 fed as
    view `view` of `views`. dy_ld: row stride of dy for forge_wino_input_dy. big: a real launch of the step - the rule's tile only, yardstick on a corner."""
    d = dict(_DEFAULTS, **kw)
    d["ld1"] = d["ld1"] or C1
    d["ld2"] = d["ld2"] or d["C2"]
    d["ldo"] = d["ldo"] or (Cout // 2 if d["epi"] == 2 else Cout)
    return Case(name=name, rows=frozenset(rows.split()), n=n, D=D, H=H, W=W, C1=C1, Cout=Cout, **d)


ROWS = ("step_gates step_state step_conv1 step_conv1_dgrad trunk320 trunk80 many2d_n many2d_d forced_tiles rule_tile ragged_r cout96 cout160 cout200 odd_wt "
        "straddle d1 d2 d3 n_gt1 hw2 ld bs gemm_bs ldv_ptv ld12 pt12 mm2_views ldo epi0 epi1 epi2 epi3 no_bias residual0 residual1 residual2 residual3 out2 out3_2 out3_3 "
        "plain2 plain3 mm2 nsum input_dy_ld wgrad32 wgrad64 wgrad128 wgrad_two wgrad_bs_pt wgrad_kd1 wgrad_kd3 dw_prior weights_kd1 weights_kd3 weights_t "
        "half_form").split()

CASES = [
    # ---- the real launches of the step (R = 8192 tile rows: 32^3 voxels) and of the 2-D trunk
    mk("gates", "step_gates epi2 out3_2 half_form rule_tile", 1, 32, 32, 32, 128, 256, C2=128, epi=2, out3=True, big=True),
    mk("state", "step_state epi3 out2 half_form", 1, 32, 32, 32, 128, 128, C2=128, epi=3, out2=True, big=True),
    mk("conv1", "step_conv1 epi1 half_form", 1, 32, 32, 32, 64, 128, epi=1, slope=0.01, big=True),
    mk("conv1_dx", "step_conv1_dgrad epi0 no_bias", 1, 32, 32, 32, 128, 64, dgrad=True, bias=False, big=True, note="rule tile C"),
    mk("trunk320", "trunk320 epi1", 5, 1, 16, 16, 256, 256, kd=1, epi=1, slope=0.0, note="rule tile D"),
    mk("trunk80", "trunk80 d1", 5, 1, 8, 8, 512, 512, kd=1, epi=1, slope=0.0),
    mk("many_n", "many2d_n odd_wt ragged_r half_form gemm_bs pt12", 37, 1, 16, 14, 64, 128, kd=1, epi=1, slope=0.0, bias=False, gviews=(2, 1), note="R = 2072: not a multiple of 64"),
    mk("many_d", "many2d_d cout96 weights_kd1", 1, 9, 12, 12, 96, 96, kd=1, wgrad=(), note="images on D: the planes must not mix"),
    # ---- every forced tile on wide, ragged cases; operand addressing
    mk("wide_a", "forced_tiles ragged_r cout96 odd_wt straddle d3 n_gt1 ld ldv_ptv ld12 pt12 ldo residual0 epi0", 2, 3, 10, 14, 64, 96, C2=32, residual=True,
       tiles=ALL_TILES, ld1=72, off1=4, ld2=40, off2=8, vcat=8, ldo=104, note="Ht x Wt = 35 < 64: tiles straddle depth planes and batch elements"),
    mk("wide_b", "forced_tiles cout160 d2 n_gt1 bs gemm_bs pt12 mm2 mm2_views residual1 epi1 wgrad128 wgrad_bs_pt wgrad_kd3", 2, 2, 16, 18, 128, 160, epi=1, slope=0.01,
       residual=True, tiles=ALL_TILES, views1=(3, 1), gviews=(3, 2), mm2=(3, 2), wgrad=(2, 1)),
    mk("wide_c", "forced_tiles cout200 d1 no_bias mm2 mm2_views", 1, 1, 12, 12, 32, 200, bias=False, tiles=ALL_TILES, mm2=(2, 1), note="D = 1 with three depth taps: both outer taps are zero"),
    mk("edge22", "hw2 n_gt1 d1", 3, 1, 2, 2, 32, 32, note="H = W = 2: every patch border is padding"),
    mk("mean5", "nsum bs", 2, 2, 6, 8, 32, 40, nsum=5, epi=1, slope=0.01),
    # ---- the GRU epilogues with every optional operand, and plain
    mk("gates_s", "epi2 residual2 out3_2 mm2", 2, 3, 8, 6, 32, 64, C2=32, epi=2, residual=True, out3=True, mm2=(1, 0)),
    mk("gates_p", "plain2 no_bias", 2, 3, 8, 6, 32, 64, C2=32, epi=2, bias=False),
    mk("state_s", "epi3 residual3 out2 out3_3 ldo mm2 mm2_views", 2, 3, 8, 6, 32, 40, C2=32, epi=3, residual=True, out2=True, out3=True, mm2=(2, 1), ldo=44),
    mk("state_p", "plain3 no_bias", 2, 3, 8, 6, 32, 40, C2=32, epi=3, bias=False),
    # ---- the backward
    mk("bw32", "wgrad32 wgrad_kd3 input_dy_ld dw_prior weights_kd3 weights_t", 2, 2, 8, 8, 32, 72, wgrad=(), dgrad=False, dy_ld=80),
    mk("bw64", "wgrad64 wgrad_kd1", 3, 1, 8, 10, 64, 40, kd=1, wgrad=()),
    mk("bw_two", "wgrad_two wgrad_kd3", 2, 2, 8, 8, 128, 64, C2=64, wgrad=()),
    mk("dx_s", "weights_t d2", 1, 2, 8, 8, 64, 32, dgrad=True, bias=False),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# forge_wino_weights alone: channel counts that are multiples of nothing
WEIGHT_SHAPES = [(40, 24, 3), (7, 5, 1), (33, 1, 3), (1, 130, 1)]

MUTATIONS = ("pt_transposed", "origin_2th", "tap_sign", "tap_cross_batch", "mm2_view", "s1_sign", "drop_last_k", "res_after", "dw_g_swap")
# (case, wrong references it must reject)
MUTATION_CASES = [
    ("wide_a", ("pt_transposed", "origin_2th", "tap_sign", "tap_cross_batch", "s1_sign", "drop_last_k")),
    ("wide_b", ("mm2_view", "res_after", "tap_sign", "dw_g_swap")),
    ("state_s", ("mm2_view", "tap_cross_batch", "s1_sign")),
    ("bw32", ("dw_g_swap", "pt_transposed")),
]


def grid_of(c):
    return (c.n, c.D, c.H // 2, c.W // 2)


def R_of(c):
    return c.n * c.D * (c.H // 2) * (c.W // 2)


def k_out(c):
    """Roundings on the longest path of S through forge_wino_output (module docstring)."""
    return 4 + bool(c.mm2) + bool(c.bias) + bool(c.residual) + (c.epi == 1) + (c.epi == 1 and c.slope not in (0.0, 1.0))


def k_gemm(c):
    return c.kd * (c.C1 + c.C2) + 2


def out_names(c):
    if c.epi == 2:
        return ("out", "out2", "out3") if c.out3 else ("out", "out2")
    if c.epi == 3:
        return ("out",) + (("out2",) if c.out2 else ()) + (("out3",) if c.out3 else ())
    return ("out",)


def rule_tile(c):
    """forge_wino_gemm_tile as the header states it: Cout <= 64 -> 'D' below 2048 tile rows, 'C' from there; else 'D' / 'B'."""
    R = R_of(c)
    return ("D" if R < 2048 else "C") if c.Cout <= 64 else ("D" if R < 2048 else "B")


def corner(c, d):
    """A big case cut down to a 3 x 8 x 8 corner of its first batch element (same channels and weights): what the chain-grain yardstick and the CPU
    tests evaluate. Fewer elements can only lower a maximum, i.e. tighten the sharp bound."""
    if not c.big:
        return c, d
    cs = c._replace(n=1, D=3, H=8, W=8, big=False)
    cut = lambda t, w: None if t is None else t.reshape(c.n, c.D, c.H, c.W, w)[:1, :3, :8, :8].reshape(-1, w).contiguous()
    ds = dict(d, x1=d["x1"][..., :1, :3, :8, :8, :].contiguous(), x2=None if d["x2"] is None else d["x2"][:1, :3, :8, :8].contiguous())
    for k in ("residual", "aux_h", "aux_z", "dy"):
        if d.get(k) is not None:
            ds[k] = cut(d[k], d[k].shape[-1])
    ds["mm2"] = None
    return cs, ds


def make_data(c):
    """Seeded float32 operands in their logical (dense) form. x1 [n][D][H][W][C1] ([nsum][n].. with nsum > 1), x2, wp [9 kd][Co][Ci] ~ N(0, 1 / K) in the
    FORWARD layout of the convolution (a dgrad case's convolution maps Cout -> C1 channels, so that its data gradient maps C1 -> Cout), bias, scale in
    [0.5, 1.5), shift / residual / h ~ N(0, 1), z in (0, 1), mm2 [16][n views vol][Cout] ~ N(0, 1/4), dy [n D H W][Cout], a prior dw."""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) + 1000)
    rn = lambda *s: torch.randn(*s, generator=g)
    Cin, M = c.C1 + c.C2, c.n * c.D * c.H * c.W
    K = 9 * c.kd * Cin
    shape = ((c.nsum,) if c.nsum > 1 else ()) + (c.n, c.D, c.H, c.W)
    d = {"x1": rn(*shape, c.C1), "x2": rn(c.n, c.D, c.H, c.W, c.C2) if c.C2 else None,
         "wp": (rn(9 * c.kd, Cin, c.Cout) if c.dgrad else rn(9 * c.kd, c.Cout, Cin)) / K ** 0.5,
         "bias": rn(c.Cout) if c.bias else None, "scale": None, "shift": None, "residual": None, "aux_h": None, "aux_z": None, "mm2": None}
    if c.epi == 1 or (c.epi == 3 and c.out2):
        d["scale"], d["shift"] = torch.rand(c.Cout, generator=g) + 0.5, rn(c.Cout)
    if c.residual:
        d["residual"] = rn(M, c.Cout)
    if c.epi == 2:
        d["aux_h"] = rn(M, c.Cout // 2)
    if c.epi == 3:
        d["aux_h"], d["aux_z"] = rn(M, c.Cout), torch.rand(M, c.Cout, generator=g) * 0.98 + 0.01
    if c.mm2:
        d["mm2"] = rn(16, c.n * c.mm2[0] * (R_of(c) // c.n), c.Cout) * 0.5
    if c.wgrad is not None or c.dy_ld:
        d["dy"], d["prior"] = rn(M, c.Cout), rn(9 * c.kd, c.Cout, Cin)
    return d


def mm2_view(c, d, mut=None):
    """The rows of the second addend this launch names: view `view` of `views` per batch element ([16][R][Cout]). mm2_view: the next view instead."""
    if d.get("mm2") is None:
        return None
    views, view = c.mm2
    if mut == "mm2_view":
        view = (view + 1) % views if views > 1 else view
    vol = R_of(c) // c.n
    m = d["mm2"].reshape(16, c.n, views, vol, c.Cout)
    if mut == "mm2_view" and views == 1:                        # one view per element: the neighbouring batch element's rows
        return m[:, :, 0].roll(1, dims=1).reshape(16, -1, c.Cout)
    return m[:, :, view].reshape(16, -1, c.Cout)


def direct_sums(c, d, mag):
    """The convolution itself, tap by tap in float64 (conv_igemm_cases.gather): [n D H W][Cout] without bias - or, mag, its magnitude sum sum |x||w|."""
    taps = cc.T27 if c.kd == 3 else cc.T9
    x1 = d["x1"].double()
    if c.nsum > 1:
        x1 = x1.mean(0)
    x = x1 if d["x2"] is None else torch.cat([x1, d["x2"].double()], dim=-1)
    wp = d["wp"].double()
    if c.dgrad:                                                  # dx: the taps negated, the weights transposed
        taps, wp = [(-a, -b, -e) for a, b, e in taps], wp.transpose(1, 2)
    if mag:
        x, wp = x.abs(), wp.abs()
    acc = torch.zeros(x.shape[0] * c.D * c.H * c.W, c.Cout, dtype=torch.float64)
    for t, tap in enumerate(taps):
        acc += cc.gather(x, c.D, c.H, c.W, 1, tap) @ wp[t].t()
    return acc


def chain(c, d, dtype=torch.float64, half=False, mut=None, want_sigma=False):
    """Forward (or data gradient) of the case through input -> point GEMM -> output in `dtype`; float32: every stage in its documented order, the GEMM at
    the chain grain. Returns (outs, sig_S, sig_A); the sigmas (float64 only, want_sigma) scale with the DIRECT convolution's magnitude sum, as the
    conv_igemm matrix's q does, plus the second addend's."""
    grain = "tap" if dtype == torch.float64 else "chain"
    V = input_transform(d["x1"], c.nsum, dtype, mut=mut)
    if d["x2"] is not None:
        V = torch.cat([V, input_transform(d["x2"], 1, dtype, mut=mut)], dim=-1)
    Uw = weights(d["wp"], c.kd, c.dgrad, dtype)
    Mm = point_gemm(V, Uw, grid_of(c), dtype, grain, mut=mut)
    m2 = mm2_view(c, d, mut)
    if half:
        Mm = row_combine(Mm)
        m2 = None if m2 is None else row_combine(m2.to(dtype))
    y = inverse_transform(Mm, m2, grid_of(c), dtype, mut=mut)
    S = None
    if want_sigma:
        S = direct_sums(c, d, True)
        if m2 is not None:
            S = S + inverse_transform(mm2_view(c, d), None, grid_of(c), mag=True)
    return tail(y, S, c, d, dtype, mut)


def wgrad_chain(c, d, dtype=torch.float64, mut=None, mag=False):
    """prior + the weight gradient of the case's convolution for the upstream gradient dy: dy -> A dy A^T, x -> V, 16 x kd point sums, G^T dU G."""
    grain = "tap" if dtype == torch.float64 else "chain"
    V = input_transform(d["x1"], 1, dtype, mag=mag, mut=mut)
    if d["x2"] is not None:
        V = torch.cat([V, input_transform(d["x2"], 1, dtype, mag=mag, mut=mut)], dim=-1)
    dM = dy_transform(d["dy"].reshape(c.n, c.D, c.H, c.W, c.Cout), dtype, mag=mag)
    return dw_transform(wgrad_points(dM, V, grid_of(c), c.kd, dtype, grain, mag=mag), d["prior"], dtype, mag=mag, mut=mut)


def q_of(got, ref, sigma):
    """(q, q_rms) = max and rms of |got - ref| / (u sigma) over every element."""
    e = (got.double() - ref).abs() / (U * sigma)
    assert torch.isfinite(e).all(), "non-finite error ratio"
    return e.max().item(), e.square().mean().sqrt().item()
