"""The F(4, 3) depth nest (forge_wino_input_dn4 / forge_wino_weights_dn4 / forge_wino_gemm_dn4) restated in plain torch, from the header block above
forge_wino_input_dn4 in include/forge_hip.h - the companion of wino_dn_cases.py, on the stages of wino_cases.py.

Per point p and group g of four planes (4g .. 4g + 3), with p_e = plane 4g - 1 + e of the batch element (zero outside ITS grid), e = 0..5:
    operand k    q0 = 4 (p0 - p2) - (p2 - p4)   q1 = (p3 + p4) - 4 (p1 + p2)   q2 = (p4 - p3) + 4 (p1 - p2)
                 q3 = (p4 - p2) + 2 (p3 - p1)   q4 = (p4 - p2) - 2 (p3 - p1)   q5 = 4 (p1 - p3) - (p3 - p5)         (the rows of BT6, per INPUT element)
                 V6[p][g][k] = (B^T q_k B)[p]
    product      m_k = V6[p][g][k] (x) U''[p][k],   U''[p][k] = sum_kd GD[k][kd] U[p][kd]
    rows         s = m1 + m2, d = m1 - m2, S = m3 + m4, D = m3 - m4:  y0 = (s + S) + m0,  y1 = d + 2 D,  y2 = s + 4 S,  y3 = (d + 8 D) + m5   (the rows of AT6)
                 where m0 / m5 are ACCUMULATED onto s + S / d + 8 D (the K loop starts from them).
Every multiplier of the operand and output sides is a power of two: a fused multiply-add with such a multiplier is one rounded addition of an exact product,
which float32 torch reproduces bit for bit with a multiplication and an addition. Every function takes a dtype: float64 is the reference, float32 performs
the kernel's operations in the kernel's order and is the yardstick. mag=True applies the same map with absolute coefficients to absolute operands.
MUTATIONS are the wrong references the GPU test must reject.
"""
import torch
import torch.nn.functional as F

import wino_cases as wc

BT6 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1.]],
                   dtype=torch.float64)
GD = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1.]],
                  dtype=torch.float64)
AT6 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1.]], dtype=torch.float64)

# swapped +- pair: positions 1 and 2 read each other's operand; a wrong sign in row 3 of A^T (d - 8 D); the four output planes of a group rotated by one;
# the operand planes taken along the flattened (n, D) axis, across the batch boundary
MUTATIONS = ("swap_pm", "row3_sign", "plane_rot", "cross_batch")
# Roundings a product term of y0 / y3 meets: the Cin steps of its own K loop, its combination (s, d, S or D), one more (s + S, or the fused
# d + 8 D), then the Cin steps of position 0 / 5 accumulated onto it: 2 Cin + K_OPS. y1 and y2 meet fewer.
K_OPS = 2


def k_point(Cin):
    """k of the unconditional bound gamma_k sum |operand||weight| on forge_wino_gemm_dn4's point products."""
    return 2 * Cin + K_OPS


def depth_stage(x, dtype=torch.float64, mag=False, cross=False):
    """x [n][D][H][W][C], D % 4 == 0 -> q [n][D/4][6][H][W][C], the six depth-combined planes of every group, in the kernel's order of operations."""
    x = x.to(dtype)
    n, D = x.shape[:2]
    if cross:
        x = x.reshape(1, n * D, *x.shape[2:])
    xp = F.pad(x, (0, 0, 0, 0, 0, 0, 1, 1))                   # index z + 1
    p = [xp[:, e::4][:, :x.shape[1] // 4] for e in range(6)]   # p[e][g] = plane 4 g - 1 + e
    if mag:
        p = [t.abs() for t in p]
        q = [4 * (p[0] + p[2]) + (p[2] + p[4]), (p[3] + p[4]) + 4 * (p[1] + p[2]), (p[4] + p[3]) + 4 * (p[1] + p[2]),
             (p[4] + p[2]) + 2 * (p[3] + p[1]), (p[4] + p[2]) + 2 * (p[3] + p[1]), 4 * (p[1] + p[3]) + (p[3] + p[5])]
    else:
        d42, d31 = p[4] - p[2], p[3] - p[1]
        q = [4 * (p[0] - p[2]) - (p[2] - p[4]), (p[3] + p[4]) - 4 * (p[1] + p[2]), (p[4] - p[3]) + 4 * (p[1] - p[2]),
             d42 + 2 * d31, d42 - 2 * d31, 4 * (p[1] - p[3]) - (p[3] - p[5])]
    return torch.stack(q, dim=2).reshape(n, D // 4, 6, *x.shape[2:])


def input_transform_dn4(x, nsum=1, dtype=torch.float64, mag=False, mut=None):
    """x [n][D][H][W][C] (nsum > 1: [nsum][n]..., the views whose mean is transformed) -> V6 [16][n (D/4) 6 Ht Wt][C]: the depth stage on the input
    elements, then wino_cases.input_transform's B^T q B on each of the 6 planes per group."""
    x = x.to(dtype)
    if nsum > 1:
        v = x[0]
        for k in range(1, nsum):
            v = v + x[k]
        x = v * (torch.ones((), dtype=dtype) / nsum)
    q = depth_stage(x, dtype, mag, mut == "cross_batch")
    n, Dg = q.shape[:2]
    return wc.input_transform(q.reshape(n, Dg * 6, *q.shape[3:]), 1, dtype, mag=mag)


def weights_dn4(wp, dtype=torch.float64, mag=False):
    """wp [27][Cout][Cin] -> U'' [16][6][Cout][Cin] = G_depth (x) (G w G^T) in float64, in the kernel's order of operations (the sixths are not exact in
    float64, so the order is part of the contract); float32 rounds once."""
    _, Co, Ci = wp.shape
    w = wp.double().reshape(3, 3, 3, Co, Ci)
    if mag:
        u = torch.einsum("kt,ia,jb,taboc->ijkoc", GD.abs(), wc.G.abs(), wc.G.abs(), w.abs())
        return u.reshape(16, 6, Co, Ci).to(dtype)
    w0, w1, w2 = w[0], w[1], w[2]
    d = [0.25 * w0, -((w0 + w2) + w1) / 6.0, -((w0 + w2) - w1) / 6.0, ((0.25 * w0 + w2) + 0.5 * w1) / 6.0, ((0.25 * w0 + w2) - 0.5 * w1) / 6.0, w2]
    out = []
    for dk in d:                                               # dk [a][b][o][c]
        g = [dk[0], 0.5 * (dk[0] + dk[1] + dk[2]), 0.5 * (dk[0] - dk[1] + dk[2]), dk[2]]          # G d: rows i, each [b][o][c]
        u = [[gi[0], 0.5 * (gi[0] + gi[1] + gi[2]), 0.5 * (gi[0] - gi[1] + gi[2]), gi[2]] for gi in g]
        out.append(torch.stack([u[i][j] for i in range(4) for j in range(4)]))
    return torch.stack(out, dim=1).to(dtype)


def _chain(X, w, acc, dtype):
    """acc + X (x) w with one fused multiply-add per k in channel order (the float32 yardstick's grain)."""
    for c in range(X.shape[-1]):
        acc = (X[:, :, c, None].double() * w[:, None, :, c].double() + acc.double()).to(dtype)
    return acc


def nest_gemm4(V6, Ud, grid, dtype=torch.float64, grain="tap", mag=False, mut=None):
    """V6 [16][n (D/4) 6 Ht Wt][Cin], Ud [16][6][Cout][Cin], grid = (n, D, Ht, Wt), D % 4 == 0 -> Mm [16][R][Cout] as forge_wino_gemm_dn4 makes it.
    grain 'chain': one fused multiply-add per k in channel order, positions 0 and 5 accumulated onto s + S and d + 8 D (the float32 yardstick)."""
    n, D, Ht, Wt = grid
    Cout, Cin = Ud.shape[2:]
    V6, Ud = V6.to(dtype), Ud.to(dtype)
    if mag:
        V6, Ud = V6.abs(), Ud.abs()
    X = V6.reshape(16, n * (D // 4), 6, Ht * Wt, Cin)
    X = [X[:, :, k].reshape(16, -1, Cin) for k in range(6)]
    if mut == "swap_pm":
        X[1], X[2] = X[2], X[1]
    zero = torch.zeros(16, X[0].shape[1], Cout, dtype=dtype)
    prod = (lambda k, acc: _chain(X[k], Ud[:, k], acc, dtype)) if grain == "chain" else (lambda k, acc: acc + X[k] @ Ud[:, k].transpose(1, 2))
    m1, m2, m3, m4 = (prod(k, zero) for k in (1, 2, 3, 4))
    if mag:
        s, d, S, Dl = m1 + m2, m1 + m2, m3 + m4, m3 + m4
        y2, y1, a0, a1 = 4 * S + s, 2 * Dl + d, s + S, 8 * Dl + d
    else:
        s, d, S, Dl = m1 + m2, m1 - m2, m3 + m4, m3 - m4
        y2, y1, a0 = 4 * S + s, 2 * Dl + d, s + S
        a1 = (-8 * Dl + d) if mut == "row3_sign" else (8 * Dl + d)
    y = [prod(0, a0), y1, y2, prod(5, a1)]
    if mut == "plane_rot":
        y = y[1:] + y[:1]
    y = [t.reshape(16, n * (D // 4), Ht * Wt, Cout) for t in y]
    return torch.stack(y, dim=2).reshape(16, n * D * Ht * Wt, Cout)


def chain_dn4(c, d, dtype=torch.float64, mut=None):
    """The case's convolution rows [n D H W][Cout] (+ bias) through input transform with depth stage -> F(4, 3) nest -> inverse transform in `dtype`."""
    grain = "tap" if dtype == torch.float64 else "chain"
    V = input_transform_dn4(d["x1"], c.nsum, dtype, mut=mut)
    if d["x2"] is not None:
        V = torch.cat([V, input_transform_dn4(d["x2"], 1, dtype, mut=mut)], dim=-1)
    Mm = nest_gemm4(V, weights_dn4(d["wp"], dtype), wc.grid_of(c), dtype, grain, mut=mut)
    y = wc.inverse_transform(Mm, None, wc.grid_of(c), dtype)
    return y if d["bias"] is None else y + d["bias"].to(dtype)
