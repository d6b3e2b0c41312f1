"""The depth nest (forge_wino_gemm_dn / forge_wino_weights_dn) restated in plain torch, from the header block above forge_wino_gemm_dn in
include/forge_hip.h - the companion of wino_cases.py, whose stages (input transform, 2-D weights, inverse transform, tails) it reuses.

A Winograd F(2, 3) over the three depth taps, on top of the 16 points of F(2x2, 3x3): per point p and pair of planes (z, z + 1), z even,
    operand k    V[z-1] - V[z+1] | V[z] + V[z+1] | V[z+1] - V[z] | V[z] - V[z+2]        (planes outside the batch element's grid are zero)
    product      m_k = operand_k (x) U'[p][k],   U'[p][k] = sum_kd G[k][kd] U[p][kd]      (depth rows of G: w0, (w0 + w1 + w2) / 2, (w0 - w1 + w2) / 2, w2)
    rows         Mm[p][z] = (m0 + m1) + m2,   Mm[p][z + 1] = (m1 - m2) - m3
Every function takes a dtype: float64 is the reference, float32 performs the kernel's operations in the kernel's order (one rounded addition per operand
element, one fused multiply-add per k, the three output additions) and is the yardstick. mag=True applies the same map with absolute coefficients to
absolute operands. MUTATIONS are the wrong references the GPU test must reject.
"""
import torch

import wino_cases as wc

# (a_k, b_k, sign): operand k = V[z - 1 + a_k] + sign V[z - 1 + b_k]
POSITIONS = ((0, 2, -1), (1, 2, 1), (2, 1, -1), (1, 3, -1))
MUTATIONS = ("swap_ab", "k2_sign", "plane_swap", "cross_batch")


def weights_dn(wp, dtype=torch.float64, mag=False):
    """wp [27][Cout][Cin] -> U' [16][4][Cout][Cin] = G_depth (x) (G w G^T): the depth stage first, then the 2-D stage, in float64; float32 rounds once."""
    _, Co, Ci = wp.shape
    w = wp.double().reshape(3, 3, 3, Co, Ci)
    g = wc.G.abs() if mag else wc.G
    if mag:
        w = w.abs()
    d = torch.einsum("kt,taboc->kaboc", g, w)
    u = torch.einsum("ia,jb,kaboc->ijkoc", g, g, d)
    return u.reshape(16, 4, Co, Ci).to(dtype)


def _planes(Vv, cross):
    """Vv [16][n][D][rows][C] -> the four operand planes d[e] = V[z - 1 + e] of every pair, each [16][n][D/2][rows][C]; zero outside the batch element
    (cross: the wrong reference that walks the flattened (n, D) axis instead)."""
    P, n, D, rows, C = Vv.shape
    out = []
    for e in range(4):
        sh = wc._depth_shift(Vv, e - 1, cross)                   # plane z + (e - 1) at index z
        out.append(sh[:, :, 0::2])
    return out


def nest_gemm(V, Ud, grid, dtype=torch.float64, grain="tap", mag=False, mut=None):
    """V [16][R][Cin], Ud [16][4][Cout][Cin], grid = (n, D, Ht, Wt), D even -> Mm [16][R][Cout] as forge_wino_gemm_dn makes it. grain 'chain': one fused
    multiply-add per k in channel order (the float32 yardstick)."""
    n, D, Ht, Wt = grid
    Cout, Cin = Ud.shape[2:]
    V, Ud = V.to(dtype), Ud.to(dtype)
    if mag:
        V, Ud = V.abs(), Ud.abs()
    d = _planes(V.reshape(16, n, D, Ht * Wt, Cin), mut == "cross_batch")
    m = []
    for k, (ia, ib, sg) in enumerate(POSITIONS):
        if mut == "swap_ab":
            ia, ib = ib, ia
        if mut == "k2_sign" and k == 2:
            sg = 1
        X = (d[ia] + d[ib]) if (mag or sg > 0) else (d[ia] - d[ib])
        X = X.reshape(16, -1, Cin)
        w = Ud[:, k]
        if grain == "chain":
            acc = torch.zeros(16, X.shape[1], Cout, dtype=dtype)
            for c in range(Cin):
                acc = (X[:, :, c, None].double() * w[:, None, :, c].double() + acc.double()).to(dtype)
        else:
            acc = X @ w.transpose(1, 2)
        m.append(acc.reshape(16, n, D // 2, Ht * Wt, Cout))
    y0, y1 = wc._at(m, mag)
    if mut == "plane_swap":
        y0, y1 = y1, y0
    return torch.stack([y0, y1], dim=3).reshape(16, n * D * Ht * Wt, Cout)


def chain_dn(c, d, dtype=torch.float64, mut=None):
    """The case's convolution rows [n D H W][Cout] (+ bias) through input transform -> depth nest -> inverse transform in `dtype`."""
    grain = "tap" if dtype == torch.float64 else "chain"
    V = wc.input_transform(d["x1"], 1, dtype)
    if d["x2"] is not None:
        V = torch.cat([V, wc.input_transform(d["x2"], 1, dtype)], dim=-1)
    Mm = nest_gemm(V, weights_dn(d["wp"], dtype), wc.grid_of(c), dtype, grain, mut=mut)
    y = wc.inverse_transform(Mm, None, wc.grid_of(c), dtype)
    return y if d["bias"] is None else y + d["bias"].to(dtype)
