"""The F(4, 3) depth nest with F(4, 3) along H and W ("dn4hw": forge_wino_input_dn4hw / forge_wino_weights_dn4hw / forge_wino_gemm_dn4hw /
forge_wino_output_dn4hw) restated in plain torch from the header block above forge_wino_input_dn4hw in include/forge_hip.h - the companion of
wino_dn4h_cases.py, on its depth and row stages.

Tiles of 4 x 4 output voxels, Ht = H / 4, Wt = W / 4, 36 points p = 6 i + j (i = 0..5 the H point, j = 0..5 the W point), groups of four planes:
    operand      q_k = the six depth lines of wino_dn4_cases.depth_stage on the input elements; w_k[i'] = THE SAME six lines over the six patch rows
                 4 th - 1 .. 4 th + 4 of q_k; V[6 i' + j'][g][k] = THE SAME six lines over the six patch columns 4 tw - 1 .. 4 tw + 4 of w_k[i']
    weights      U[6 i + j][k] = G4(depth)[k] (x) G4(H)[i] (x) G4(W)[j] in float64, depth rows first, then H, then W, rounded once
    product      wino_dn4h_cases.nest_gemm's schedule on 36 points -> Mm [36][n D Ht Wt][Cout]
    inverse      over i, per j: s = m1 + m2, d = m1 - m2, S = m3 + m4, D = m3 - m4 -> (s + S) + m0 | d + 2 D | s + 4 S | (d + 8 D) + m5; then the same four
                 lines over j, per output row
Every multiplier of the operand and output sides is a power of two, so float32 torch (a multiplication and an addition) reproduces the kernels' fused
multiply-adds bit for bit. Every function takes a dtype: float64 is the reference, float32 performs the kernel's operations in the kernel's order and is
the yardstick; mag=True applies the same map with absolute coefficients to absolute operands. MUTATIONS are the wrong references the GPU test must reject.
"""
import torch
import torch.nn.functional as F

import wino_cases as wc
import wino_dn4_cases as d4
import wino_dn4h_cases as dh

POINTS = 36
# column line 3 computed as line 4 (a sign in the W stage); the points read as 6 j' + i' (H and W points swapped); the group's positions written in the
# order 1, 0, 2 .. 5
MUTATIONS = ("wrong_column_line", "swap_points", "position_order")


def grid_of(c):
    return (c.n, c.D, c.H // 4, c.W // 4)


def input_transform_dn4hw(x, nsum=1, dtype=torch.float64, mag=False, mut=None):
    """x [n][D][H][W][C] (nsum > 1: [nsum][n]..., the views whose mean is transformed), D, H, W % 4 == 0 -> V [36][n (D/4) 6 Ht Wt][C]."""
    x = x.to(dtype)
    if nsum > 1:
        v = x[0]
        for k in range(1, nsum):
            v = v + x[k]
        x = v * (torch.ones((), dtype=dtype) / nsum)
    q = d4.depth_stage(x, dtype, mag)                                              # [n][D/4][6][H][W][C]
    if mut == "position_order":
        q = q[:, :, [1, 0, 2, 3, 4, 5]]
    n, Dg, _, H, W, C = q.shape
    Ht, Wt = H // 4, W // 4
    xp = F.pad(q.reshape(n * Dg * 6, H, W, C), (0, 0, 1, 4, 1, 4))
    d = [[xp[:, i:i + 4 * Ht:4, j:j + 4 * Wt:4].reshape(-1, C) for j in range(6)] for i in range(6)]
    w = [dh.six_lines([d[i][j] for i in range(6)], mag) for j in range(6)]        # w[j][i']: rows
    v = [dh.six_lines([w[j][i] for j in range(6)], mag) for i in range(6)]        # v[i'][j']: columns
    if mut == "wrong_column_line":
        for i in range(6):
            v[i][3] = v[i][4]
    return torch.stack([v[i][j] for i in range(6) for j in range(6)])


def weights_dn4hw(wp, dtype=torch.float64, mag=False, mut=None):
    """wp [27][Cout][Cin] -> U [36][6][Cout][Cin] = G4(depth) (x) G4(H) (x) G4(W) in float64, in the kernel's order of operations; float32 rounds once."""
    _, Co, Ci = wp.shape
    w = wp.double().reshape(3, 3, 3, Co, Ci)
    if mag:
        u = torch.einsum("kt,ia,jb,taboc->ijkoc", d4.GD.abs(), d4.GD.abs(), d4.GD.abs(), w.abs())
        return u.reshape(POINTS, 6, Co, Ci).to(dtype)
    out = []
    for dk in dh._rows43(w[0], w[1], w[2]):                                        # dk [a][b][o][c]
        g = dh._rows43(dk[0], dk[1], dk[2])                                        # rows i, each [b][o][c]
        u = [dh._rows43(gi[0], gi[1], gi[2]) for gi in g]
        out.append(torch.stack([u[j][i] if mut == "swap_points" else u[i][j] for i in range(6) for j in range(6)]))
    return torch.stack(out, dim=1).to(dtype)


def nest_gemm(V, Ud, grid, dtype=torch.float64, grain="tap", mag=False):
    """V [36][n (D/4) 6 Ht Wt][Cin], Ud [36][6][Cout][Cin], grid = (n, D, Ht, Wt) -> Mm [36][n D Ht Wt][Cout]: wino_dn4h_cases.nest_gemm's schedule (which
    reads the number of points from its module) on 36 points."""
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
    if mag:
        s, d, S, Dl = m1 + m2, m1 + m2, m3 + m4, m3 + m4
    else:
        s, d, S, Dl = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    y = [prod(0, s + S), 2 * Dl + d, 4 * S + s, prod(5, 8 * Dl + d)]
    y = [t.reshape(POINTS, n * (D // 4), Ht * Wt, Cout) for t in y]
    return torch.stack(y, dim=2).reshape(POINTS, n * D * Ht * Wt, Cout)


def four_lines(m, mag=False):
    """A^T of F(4, 3) on six operands, in the kernels' order."""
    m0, m1, m2, m3, m4, m5 = m
    if mag:
        sl, dl, Sl, Dl = m1 + m2, m1 + m2, m3 + m4, m3 + m4
    else:
        sl, dl, Sl, Dl = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    return [(sl + Sl) + m0, 2 * Dl + dl, 4 * Sl + sl, (8 * Dl + dl) + m5]


def inverse_transform_dn4hw(Mm, grid, dtype=torch.float64, mag=False):
    """Mm [36][n D Ht Wt][C] -> y rows [n D H W][C]: A^T of F(4, 3) over the six H points, then over the six W points."""
    n, D, Ht, Wt = grid
    m = Mm.to(dtype)
    if mag:
        m = m.abs()
    C = m.shape[-1]
    s = [four_lines([m[6 * i + j] for i in range(6)], mag) for j in range(6)]      # s[j][i']
    y = [four_lines([s[j][i] for j in range(6)], mag) for i in range(4)]           # y[i'][j']
    Y = torch.stack([torch.stack(y[i], dim=-2) for i in range(4)], dim=1)          # [R][4][4][C]
    return Y.reshape(n, D, Ht, Wt, 4, 4, C).permute(0, 1, 2, 4, 3, 5, 6).reshape(-1, C)


def conv_rows(c, d, dtype=torch.float64, mut=None):
    """The case's convolution rows [n D H W][Cout] WITHOUT bias through input transform -> 36-point nest -> inverse transform in `dtype`."""
    grain = "tap" if dtype == torch.float64 else "chain"
    V = input_transform_dn4hw(d["x1"], c.nsum, dtype, mut=mut)
    if d["x2"] is not None:
        V = torch.cat([V, input_transform_dn4hw(d["x2"], 1, dtype, mut=mut)], dim=-1)
    Mm = nest_gemm(V, weights_dn4hw(d["wp"], dtype, mut=mut), grid_of(c), dtype, grain)
    return inverse_transform_dn4hw(Mm, grid_of(c), dtype)


def chain_dn4hw(c, d, dtype=torch.float64, mut=None, want_sigma=False):
    """conv_rows through the case's tail (wino_cases.tail: bias, then the GRU epilogue): (outs, sig_S, sig_A) as wino_cases.chain returns them."""
    S = wc.direct_sums(c, d, True) if want_sigma else None
    return wc.tail(conv_rows(c, d, dtype, mut), S, c, d, dtype)
