"""The F(4, 3) depth nest with F(4, 3) along H ("dn4h": forge_wino_input_dn4h / forge_wino_weights_dn4h / forge_wino_gemm_dn4h / forge_wino_output_dn4h)
restated in plain torch from the header block above forge_wino_input_dn4h in include/forge_hip.h - the companion of wino_dn4_cases.py, on its depth stage
and on the stages of wino_cases.py.

Tiles of 4 x 2 output voxels, Ht = H / 4, Wt = W / 2, 24 points p = 4 i + j (i = 0..5 the H point, j = 0..3 the W point), groups of four planes:
    operand      q_k = the six depth lines of wino_dn4_cases.depth_stage on the input elements; w_k[i'] = THE SAME six lines over the six patch rows
                 4 th - 1 .. 4 th + 4 of q_k; V[4 i' + j'][g][k] = (w_k[i'] B)[j'], B of F(2, 3)
    weights      U[4 i + j][k] = G4(depth)[k] (x) G4(H)[i] (x) G2(W)[j] in float64, depth rows first, then H, then W, rounded once
    product      forge_wino_gemm_dn4's schedule per point (positions 1, 2 | 3, 4 | 0 accumulated onto s + S | 5 onto d + 8 D) -> Mm [24][n D Ht Wt][Cout]
    inverse      over i: s = m1 + m2, d = m1 - m2, S = m3 + m4, D = m3 - m4 -> (s + S) + m0 | d + 2 D | s + 4 S | (d + 8 D) + m5; then wino_cases' A^T over j
Every multiplier of the operand and output sides is a power of two, so float32 torch (a multiplication and an addition) reproduces the kernels' fused
multiply-adds bit for bit. Every function takes a dtype: float64 is the reference, float32 performs the kernel's operations in the kernel's order and is
the yardstick; mag=True applies the same map with absolute coefficients to absolute operands. MUTATIONS are the wrong references the GPU test must reject.
"""
import torch
import torch.nn.functional as F

import wino_cases as wc
import wino_dn4_cases as d4

POINTS = 24
# one of the 24 points left out of the inverse transform; depth position 3's product left out; patch row 5 (the row below the tile) read as zero
MUTATIONS = ("drop_point", "drop_position", "drop_row")


def six_lines(p, mag=False):
    """The six lines of B^T of F(4, 3) on six operands, in the kernels' order (wino_dn4_cases.depth_stage applies the same lines to planes)."""
    if mag:
        return [4 * (p[0] + p[2]) + (p[2] + p[4]), (p[3] + p[4]) + 4 * (p[1] + p[2]), (p[4] + p[3]) + 4 * (p[1] + p[2]),
                (p[4] + p[2]) + 2 * (p[3] + p[1]), (p[4] + p[2]) + 2 * (p[3] + p[1]), 4 * (p[1] + p[3]) + (p[3] + p[5])]
    d42, d31 = p[4] - p[2], p[3] - p[1]
    return [4 * (p[0] - p[2]) - (p[2] - p[4]), (p[3] + p[4]) - 4 * (p[1] + p[2]), (p[4] - p[3]) + 4 * (p[1] - p[2]),
            d42 + 2 * d31, d42 - 2 * d31, 4 * (p[1] - p[3]) - (p[3] - p[5])]


def grid_of(c):
    return (c.n, c.D, c.H // 4, c.W // 2)


def input_transform_dn4h(x, nsum=1, dtype=torch.float64, mag=False, mut=None):
    """x [n][D][H][W][C] (nsum > 1: [nsum][n]..., the views whose mean is transformed), D % 4 == 0, H % 4 == 0 -> V [24][n (D/4) 6 Ht Wt][C]."""
    x = x.to(dtype)
    if nsum > 1:
        v = x[0]
        for k in range(1, nsum):
            v = v + x[k]
        x = v * (torch.ones((), dtype=dtype) / nsum)
    q = d4.depth_stage(x, dtype, mag)                                              # [n][D/4][6][H][W][C]
    n, Dg, _, H, W, C = q.shape
    Ht, Wt = H // 4, W // 2
    xp = F.pad(q.reshape(n * Dg * 6, H, W, C), (0, 0, 1, 2, 1, 4))
    d = [[xp[:, i:i + 4 * Ht:4, j:j + 2 * Wt:2].reshape(-1, C) for j in range(4)] for i in range(6)]
    if mut == "drop_row":
        d[5] = [torch.zeros_like(t) for t in d[5]]
    w = [six_lines([d[i][j] for i in range(6)], mag) for j in range(4)]           # w[j][i']: rows
    v = [wc._bt([w[j][i] for j in range(4)], mag) for i in range(6)]              # v[i'][j']: columns
    return torch.stack([v[i][j] for i in range(6) for j in range(4)])


def _rows43(w0, w1, w2):
    """The six rows of G of F(4, 3) on three taps, in the kernel's float64 order."""
    return [0.25 * w0, -((w0 + w2) + w1) / 6.0, -((w0 + w2) - w1) / 6.0, ((0.25 * w0 + w2) + 0.5 * w1) / 6.0, ((0.25 * w0 + w2) - 0.5 * w1) / 6.0, w2]


def weights_dn4h(wp, dtype=torch.float64, mag=False):
    """wp [27][Cout][Cin] -> U [24][6][Cout][Cin] = G4(depth) (x) G4(H) (x) G2(W) in float64, in the kernel's order of operations; float32 rounds once."""
    _, Co, Ci = wp.shape
    w = wp.double().reshape(3, 3, 3, Co, Ci)
    if mag:
        u = torch.einsum("kt,ia,jb,taboc->ijkoc", d4.GD.abs(), d4.GD.abs(), wc.G.abs(), w.abs())
        return u.reshape(POINTS, 6, Co, Ci).to(dtype)
    out = []
    for dk in _rows43(w[0], w[1], w[2]):                                           # dk [a][b][o][c]
        g = _rows43(dk[0], dk[1], dk[2])                                           # rows i, each [b][o][c]
        u = [[gi[0], 0.5 * (gi[0] + gi[1] + gi[2]), 0.5 * (gi[0] - gi[1] + gi[2]), gi[2]] for gi in g]
        out.append(torch.stack([u[i][j] for i in range(6) for j in range(4)]))
    return torch.stack(out, dim=1).to(dtype)


def nest_gemm(V, Ud, grid, dtype=torch.float64, grain="tap", mag=False, mut=None):
    """V [24][n (D/4) 6 Ht Wt][Cin], Ud [24][6][Cout][Cin], grid = (n, D, Ht, Wt) -> Mm [24][n D Ht Wt][Cout]: wino_dn4_cases.nest_gemm4's schedule on 24
    points. grain 'chain': one fused multiply-add per k in channel order, positions 0 and 5 accumulated onto s + S and d + 8 D."""
    n, D, Ht, Wt = grid
    Cout, Cin = Ud.shape[2:]
    V, Ud = V.to(dtype), Ud.to(dtype)
    if mag:
        V, Ud = V.abs(), Ud.abs()
    X = V.reshape(POINTS, n * (D // 4), 6, Ht * Wt, Cin)
    X = [X[:, :, k].reshape(POINTS, -1, Cin) for k in range(6)]
    zero = torch.zeros(POINTS, X[0].shape[1], Cout, dtype=dtype)
    prod = (lambda k, acc: d4._chain(X[k], Ud[:, k], acc, dtype)) if grain == "chain" else (lambda k, acc: acc + X[k] @ Ud[:, k].transpose(1, 2))
    m1, m2, m3, m4 = (prod(k, zero) for k in (1, 2, 3, 4))
    if mut == "drop_position":
        m3 = zero
    if mag:
        s, d, S, Dl = m1 + m2, m1 + m2, m3 + m4, m3 + m4
    else:
        s, d, S, Dl = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    y = [prod(0, s + S), 2 * Dl + d, 4 * S + s, prod(5, 8 * Dl + d)]
    y = [t.reshape(POINTS, n * (D // 4), Ht * Wt, Cout) for t in y]
    return torch.stack(y, dim=2).reshape(POINTS, n * D * Ht * Wt, Cout)


def inverse_transform_dn4h(Mm, grid, dtype=torch.float64, mag=False, mut=None):
    """Mm [24][n D Ht Wt][C] -> y rows [n D H W][C]: A^T of F(4, 3) over the six H points, then A^T of F(2, 3) over the four W points."""
    n, D, Ht, Wt = grid
    m = Mm.to(dtype)
    if mag:
        m = m.abs()
    if mut == "drop_point":
        m = m.clone()
        m[13] = 0
    C = m.shape[-1]
    s = []                                                                         # s[j][i']
    for j in range(4):
        m0, m1, m2, m3, m4, m5 = (m[4 * i + j] for i in range(6))
        if mag:
            sl, dl, Sl, Dl = m1 + m2, m1 + m2, m3 + m4, m3 + m4
        else:
            sl, dl, Sl, Dl = m1 + m2, m1 - m2, m3 + m4, m3 - m4
        s.append([(sl + Sl) + m0, 2 * Dl + dl, 4 * Sl + sl, (8 * Dl + dl) + m5])
    y = [wc._at([s[j][i] for j in range(4)], mag) for i in range(4)]               # y[i'][j']
    Y = torch.stack([torch.stack(y[i], dim=-2) for i in range(4)], dim=1)          # [R][4][2][C]
    return Y.reshape(n, D, Ht, Wt, 4, 2, C).permute(0, 1, 2, 4, 3, 5, 6).reshape(-1, C)


def conv_rows(c, d, dtype=torch.float64, mut=None):
    """The case's convolution rows [n D H W][Cout] WITHOUT bias through input transform -> 24-point nest -> inverse transform in `dtype`."""
    grain = "tap" if dtype == torch.float64 else "chain"
    V = input_transform_dn4h(d["x1"], c.nsum, dtype, mut=mut)
    if d["x2"] is not None:
        V = torch.cat([V, input_transform_dn4h(d["x2"], 1, dtype, mut=mut)], dim=-1)
    Mm = nest_gemm(V, weights_dn4h(d["wp"], dtype), grid_of(c), dtype, grain, mut=mut)
    return inverse_transform_dn4h(Mm, grid_of(c), dtype, mut=mut)


def chain_dn4h(c, d, dtype=torch.float64, mut=None, want_sigma=False):
    """conv_rows through the case's tail (wino_cases.tail: bias, then the GRU epilogue): (outs, sig_S, sig_A) as wino_cases.chain returns them."""
    S = wc.direct_sums(c, d, True) if want_sigma else None
    return wc.tail(conv_rows(c, d, dtype, mut), S, c, d, dtype)
