"""The dispatch-space matrix of the pose warp (forge_amd/csrc/rotate.hip): the contract restated in plain torch, and the case table.

tests/test_gpu_rotate_matrix.py launches every case of CASES through the C entry points (forge_rotate_fwd[_slots], forge_rotate_bwd[_slots][_det])
and measures it against evaluate() in float64; tests/test_rotate_reference_cpu.py pins evaluate() to independent index arithmetic (explicit()), to
the oracle and to finite differences, checks that every coverage row is reached and every derivative case clears the lattice, and validates the
wrong references (MUTATIONS) before a GPU is spent on them. Both import this module, so the table cannot drift between them.

The contract (models/rotate.py:127-141 of the reference, include/forge_hip.h):
    out[slot[i]] = vox[i]                                                    mode[i] == 0
    out[slot[i]] = grid_sample(vox[i], s, trilinear, zeros, align_corners=False),  s = A_i [gx gy gz 1]^T,  g_a = linspace(-1, 1, N_a)
evaluate() is that sentence in torch; gradients() differentiates <out, dout> by autograd for vox and xf. explicit() is the same contract by floor /
8-tap index arithmetic with a hand-written adjoint: it shares nothing with grid_sample or autograd, and it carries the wrong readings (MUTATIONS).

Bounds (the ones the project already states for this kernel; u = 2^-24):
  forward   max(2e-5, 3 N_max 2^-23) max(1, |ref|_max)
  dvox      1e-4 |ref|_max
  dxf       per transform row a (the four entries of row a, over all views), relative to that row's maximum: SHARP x the float32 CPU evaluation of
            evaluate() (the yardstick), at least 64 u, never more than 2e-3; the atomic entry gets its stated run-to-run noise of 1e-5 on top.
            Compared on cases that clear the lattice only (clearance()): the trilinear derivative jumps where a sample sits on an integer plane.
  exact     a volume thrown out of the grid: zeros forward, zero dvox, zero dxf; mode-0 rows of dxf: zeros; mode-0 volumes: bitwise copies.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_igemm_cases as cc

U = cc.U
SHARP = cc.SHARP
CANARY = cc.CANARY
DXF_CAP = 2e-3            # the only figure the project had for the affine gradient (against the fp32 oracle)
DXF_FLOOR = 64 * U
ATOMIC_NOISE = 1e-5       # test_rotate_bwd_det's stated run-to-run noise of the atomic sums

_FIELDS = "name rows C D H W views slot seed dxf muts note"
Case = namedtuple("Case", _FIELDS)


def mk(name, rows, C, grid, views, slot=None, seed=0, dxf=True, muts="", note=""):
    """views: one transform kind per view (KINDS; 'copy' = mode 0). slot: where view i is stored (None: the plain entries). dxf: the affine gradient is
    compared (the case must then clear the lattice: test_rotate_reference_cpu asserts it)."""
    D, H, W = grid
    return Case(name, frozenset(rows.split()), C, D, H, W, tuple(views.split()), None if slot is None else tuple(slot), seed, dxf, tuple(muts.split()), note)


KINDS = ("copy", "orbit", "orbit_z", "s055", "s19", "reflect", "aniso", "quarter", "quarter_lattice", "out", "clip")

# The rows of the coverage table; test_rotate_reference_cpu.test_coverage_rows asserts that every one is reached and holds what its name says.
# Every case runs the forward, the gather alone (dxf == NULL), both affine gradients alone (dvox == NULL) and the deterministic one onto a prior.
ROWS = ("plain_small plain_one_side tile_cubic tile_noncubic fwd_nq1 fwd_nq2 gather_nq1 gather_nq2 gather_nq4 c8 c64 c72 c128 c136 "
        "tile_nq4 orbit orbit_z s055 s19 reflect aniso quarter quarter_lattice out clip mode_mix slots slots_not_involution dxf_plain dxf_tile "
        "dxf_nq1 dxf_nq2 dxf_nq4").split()

CASES = [
    mk("p8", "plain_small c8 orbit s055 s19 reflect aniso mode_mix slots slots_not_involution", 8, (6, 10, 14), "copy orbit s055 s19 reflect aniso",
       slot=(2, 0, 3, 5, 1, 4), seed=0, muts="lin_mismatch swap_n drop_corner lost_sign slot_side",
       note="840 voxels in x-fastest order; D != H != W; a 6-cycle of slots (the inverse permutation is another one)"),
    mk("p64", "plain_small c64 orbit reflect s055", 64, (6, 10, 14), "orbit reflect s055", seed=0, muts="swap_n", note="C4 = 16: the first width with two channel groups per thread, forward and gather"),
    mk("p72", "plain_small c72 orbit s19", 72, (6, 10, 14), "orbit s19", seed=0, note="C4 = 18: even, not a multiple of 4: two groups in both directions"),
    mk("p128", "plain_small c128 orbit s055 clip", 128, (6, 10, 14), "orbit s055 clip", seed=0, muts="drop_corner", note="C4 = 32: four groups in the gather, two forward"),
    mk("p136", "plain_small c136 orbit aniso", 136, (5, 6, 7), "orbit aniso", seed=0, note="C4 = 34 >= 32 but not a multiple of 4: back to two groups in the gather"),
    mk("p_side", "plain_one_side c8 orbit_z s19 out mode_mix", 8, (16, 32, 24), "orbit_z s19 out copy", seed=0, muts="swap_n",
       note="W = 24 is the one side that is no multiple of 16: x-fastest order on a grid of tile size"),
    mk("t16", "tile_cubic c8 orbit_z reflect clip mode_mix slots", 8, (16, 16, 16), "copy orbit_z reflect clip", slot=(1, 0, 3, 2), seed=0, muts="lost_sign",
       note="one 16^3 cube per volume in tile order"),
    mk("t_nc", "tile_noncubic c8 orbit_z aniso", 8, (16, 32, 48), "orbit_z aniso", seed=1, muts="swap_n lin_mismatch", note="2 x 3 cubes of 16^3: nsx = 3, nsy = 2 in voxel_of"),
    mk("t_c128", "tile_cubic tile_nq4 c128 orbit_z s055", 128, (16, 16, 16), "orbit_z s055", seed=1, note="four channel groups per thread in tile order"),
    mk("t_c64", "tile_cubic c64 orbit_z", 64, (16, 16, 16), "orbit_z s19", seed=0, note="two channel groups per thread in tile order"),
    mk("quarter", "tile_cubic c8 quarter quarter_lattice", 8, (16, 16, 16), "quarter quarter_lattice copy", dxf=False,
       note="zero translation; scaled by (N - 1) / N the samples fall on the lattice points themselves: forward and dvox only"),
    mk("q_plain", "plain_small c8 quarter", 8, (6, 10, 10), "quarter", dxf=False, note="the quarter turn in x-fastest order, H = W"),
    mk("edge", "plain_small c8 out clip mode_mix slots", 8, (6, 10, 14), "out clip copy clip", slot=(3, 2, 1, 0), seed=0,
       note="a volume thrown out of the grid: exact zeros everywhere; two clipped to about half"),
]
# Measured on the MI355X, per case (forward and dvox: absolute; dxf: the three transform rows). A ratio is the worst group's error over the float32 CPU yardstick's (at least 64 u / SHARP); the bound is SHARP = 4.
MEASURED = {
    "p8": "fwd 3.17e-06 dvox 2.89e-06 dxf rows atomic [2.2e-07 2.5e-07 1.1e-06] det [2.2e-07 2.5e-07 1.1e-06] of yardstick [4.9e-07 5.0e-07 1.7e-06]: 0.64x / 0.64x",
    "p64": "fwd 3.77e-06 dvox 4.06e-06 dxf rows atomic [7.2e-07 8.3e-07 1.4e-06] det [7.2e-07 8.3e-07 1.5e-06] of yardstick [1.0e-06 1.2e-06 2.4e-06]: 0.71x / 0.71x",
    "p72": "fwd 3.76e-06 dvox 2.96e-06 dxf rows atomic [2.0e-07 1.3e-06 1.8e-06] det [2.1e-07 1.3e-06 1.8e-06] of yardstick [1.1e-06 8.4e-07 1.5e-06]: 1.41x / 1.38x",
    "p128": "fwd 3.89e-06 dvox 3.78e-06 dxf rows atomic [2.7e-07 5.5e-07 5.0e-07] det [2.8e-07 5.8e-07 5.3e-07] of yardstick [9.0e-07 1.0e-06 1.3e-06]: 0.53x / 0.56x",
    "p136": "fwd 1.90e-06 dvox 1.75e-06 dxf rows atomic [1.3e-07 1.1e-06 5.8e-07] det [1.3e-07 1.1e-06 5.8e-07] of yardstick [2.9e-07 1.2e-06 1.4e-06]: 0.93x / 0.93x",
    "p_side": "fwd 9.85e-06 dvox 8.28e-06 dxf rows atomic [2.3e-06 1.3e-06 2.5e-06] det [2.2e-06 1.3e-06 2.4e-06] of yardstick [3.1e-06 1.1e-06 2.3e-06]: 1.24x / 1.24x",
    "t16": "fwd 6.17e-06 dvox 4.58e-06 dxf rows atomic [1.3e-06 1.5e-06 1.3e-06] det [1.3e-06 1.5e-06 1.3e-06] of yardstick [1.8e-06 1.8e-06 1.6e-06]: 0.86x / 0.85x",
    "t_nc": "fwd 1.98e-05 dvox 1.24e-05 dxf rows atomic [2.5e-06 1.6e-06 2.2e-06] det [2.4e-06 1.6e-06 2.2e-06] of yardstick [3.1e-06 4.2e-06 6.9e-06]: 0.80x / 0.78x",
    "t_c128": "fwd 4.24e-06 dvox 7.01e-06 dxf rows atomic [8.0e-07 7.6e-07 1.3e-06] det [1.2e-06 8.1e-07 1.3e-06] of yardstick [2.0e-06 8.1e-07 1.1e-06]: 1.16x / 1.16x",
    "t_c64": "fwd 4.08e-06 dvox 3.82e-06 dxf rows atomic [8.4e-07 3.4e-06 4.6e-07] det [9.4e-07 3.4e-06 4.6e-07] of yardstick [2.9e-07 4.6e-06 4.6e-07]: 0.88x / 0.99x",
    "quarter": "fwd 5.67e-06 dvox 5.61e-06 dxf not compared",
    "q_plain": "fwd 2.15e-06 dvox 2.87e-06 dxf not compared",
    "edge": "fwd 4.19e-06 dvox 2.71e-06 dxf rows atomic [1.2e-06 1.2e-06 2.0e-06] det [1.2e-06 1.2e-06 2.0e-06] of yardstick [8.0e-07 1.3e-06 2.2e-06]: 1.30x / 1.30x",
}
CASES = [c._replace(note=(c.note + "; " if c.note else "") + "MI355X: " + MEASURED[c.name]) for c in CASES]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

MUTATIONS = ("lin_mismatch", "swap_n", "drop_corner", "lost_sign", "slot_side")
MUTATION_CASES = [(c.name, c.muts) for c in CASES if c.muts]


def nq_forward(C):
    C4 = C // 4
    return 2 if (C4 >= 16 and C4 % 2 == 0) else 1


def nq_gather(C):
    C4 = C // 4
    return 4 if (C4 >= 32 and C4 % 4 == 0) else 2 if (C4 >= 16 and C4 % 2 == 0) else 1


def tile_order(c):
    return ((c.W | c.H | c.D) & 15) == 0


def affine_blocks(c):
    """workgroups per volume of the affine-gradient kernel: 256 threads x 8 float4 elements each"""
    per_vol = c.D * c.H * c.W * (c.C // 4)
    return (per_vol + 2047) // 2048


def _rot(axis, ang):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


def transform(kind, g, N):
    """The 3 x 4 affine of one view, in normalised grid coordinates (float64; make_data rounds it to float32). g: the case's generator (jitter)."""
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    A, t = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    if kind == "copy":
        return torch.zeros(3, 4, dtype=torch.float64)
    if kind == "orbit":
        A, t = _rot((r(3) - 0.5).tolist(), 0.25 + 0.3 * r(1).item()), (r(3) - 0.5) * 0.2
    elif kind == "orbit_z":          # a pose that turns about the grid's z axis: z planes map to z planes
        A, t = _rot((0.0, 0.0, 1.0), 0.25 + 0.3 * r(1).item()), (r(3) - 0.5) * 0.2
    elif kind == "s055":
        A, t = torch.diag(0.55 + 0.02 * r(3)), (r(3) - 0.5) * 0.2
    elif kind == "s19":
        A, t = torch.diag(1.9 + 0.05 * r(3)), (r(3) - 0.5) * 0.1
    elif kind == "reflect":
        A, t = _rot((0.0, 0.0, 1.0), 0.2 + 0.2 * r(1).item()) @ torch.diag(torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64)), (r(3) - 0.5) * 0.2
    elif kind == "aniso":
        A, t = _rot((0.0, 0.0, 1.0), 0.15 + 0.2 * r(1).item()) @ torch.diag(torch.tensor([0.7, 1.3, 1.6], dtype=torch.float64) + 0.05 * r(3)), (r(3) - 0.5) * 0.2
    elif kind in ("quarter", "quarter_lattice"):
        A = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
        if kind == "quarter_lattice":
            assert N[0] == N[1] == N[2]
            A = A * ((N[0] - 1) / N[0])
    elif kind == "out":
        t = torch.tensor([3.5, 0.1, -0.1], dtype=torch.float64)
    elif kind == "clip":
        A, t = _rot((0.0, 0.0, 1.0), 0.1 + 0.1 * r(1).item()), torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64) + (r(3) - 0.5) * 0.1
    else:
        raise KeyError(kind)
    return torch.cat([A, t[:, None]], dim=1)


def make_data(c):
    """Seeded float32 operands: vox, dout [n][D][H][W][C] (the kernels' channels-last layout) ~ N(0, 1), xf [n][12], mode, slot, prior [n][12]."""
    g = torch.Generator().manual_seed(1000 * c.seed + sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)))
    n = len(c.views)
    xf = torch.stack([transform(k, g, (c.W, c.H, c.D)) for k in c.views]).reshape(n, 12).float()
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"vox": rn(n, c.D, c.H, c.W, c.C), "dout": rn(n, c.D, c.H, c.W, c.C), "xf": xf,
            "mode": torch.tensor([0 if k == "copy" else 1 for k in c.views], dtype=torch.int32),
            "slot": None if c.slot is None else torch.tensor(c.slot, dtype=torch.int32), "prior": rn(n, 12)}


def evaluate(vox, xf, mode, slot=None, dtype=torch.float64):
    """The contract in plain torch. vox [n][C][D][H][W], xf [n][12], mode [n], slot [n] or None -> out [n][C][D][H][W] in `dtype`."""
    vox, xf = vox.to(dtype), xf.to(dtype)
    n, C, D, H, W = vox.shape
    gz, gy, gx = torch.meshgrid(torch.linspace(-1, 1, D, dtype=dtype), torch.linspace(-1, 1, H, dtype=dtype), torch.linspace(-1, 1, W, dtype=dtype), indexing="ij")
    G = torch.stack([gx, gy, gz, torch.ones_like(gx)], dim=-1)                             # [D][H][W][4]
    s = torch.einsum("nab,dhwb->ndhwa", xf.view(n, 3, 4), G)
    warped = F.grid_sample(vox, s, mode="bilinear", padding_mode="zeros", align_corners=False)
    out = torch.where((torch.as_tensor(mode) != 0).view(n, 1, 1, 1, 1), warped, vox)
    if slot is not None:
        out = torch.zeros_like(out).index_copy(0, torch.as_tensor(slot).long(), out)       # view i is stored at volume slot[i]
    return out


def gradients(c, d, dtype=torch.float64):
    """(out, dvox, dxf) of <out, dout> by autograd through evaluate(), channels-last like the kernels' operands: [n][D][H][W][C], [n][12]."""
    vox = d["vox"].to(dtype).permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    xf = d["xf"].to(dtype).clone().requires_grad_(True)
    out = evaluate(vox, xf, d["mode"], d["slot"], dtype)
    (out * d["dout"].to(dtype).permute(0, 4, 1, 2, 3)).sum().backward()
    return out.detach().permute(0, 2, 3, 4, 1).contiguous(), vox.grad.permute(0, 2, 3, 4, 1).contiguous(), xf.grad


def _box_keep(A, N, q, x, mut):
    """The gather's candidate box, restated from its comment: source voxel q receives from the integer points x of P^-1 (q - p0 + (-1, 1)^3).
    Returns whether x lies inside the box of q. q, x: [M][3] integer (x, y, z). mut: a WRONG box."""
    Nf = torch.tensor(N, dtype=torch.float64)
    P = A[:, :3] * (Nf[None, :] / (Nf[:, None] - 1) if mut == "swap_n" else Nf[:, None] / (Nf[None, :] - 1))
    p0 = ((A[:, 3] - A[:, :3].sum(1) + 1) * Nf - 1) * 0.5
    Inv = torch.linalg.inv(P)
    if mut == "lost_sign" and torch.linalg.det(P) < 0:
        Inv = -Inv                                            # the cofactors over |det|
    ctr = (q.double() - p0) @ Inv.T
    hh = Inv.abs().sum(1)[None, :] + 0.02 + 1e-5 * ctr.abs()
    lo = torch.maximum(ctr - hh, torch.tensor(-1.0, dtype=torch.float64)).ceil().clamp_min(0)
    hi = torch.minimum(torch.minimum(ctr + hh, Nf).floor(), Nf - 1)
    keep = ((x >= lo) & (x <= hi)).all(1)
    if mut == "drop_corner":
        keep = keep & ~(x == hi).all(1)
    return keep


def explicit(c, d, mut=None, box=False):
    """The contract and its adjoint by floor / 8-tap index arithmetic in float64: {"out", "dvox" [n][D][H][W][C], "dxf" [n][12], "pos": per warped view
    (voxel coordinates [M][3], has an in-range tap [M])}. box: the volume gradient only receives what the gather's candidate box lets through
    (restated from the kernel's comment: it must let everything through). mut: one of MUTATIONS - a deliberately WRONG reading."""
    assert mut is None or mut in MUTATIONS
    n, D, H, W, C = d["vox"].shape
    N = (W, H, D)
    Nl, Nf = torch.tensor(N), torch.tensor(N, dtype=torch.float64)
    M = D * H * W
    e = torch.arange(M)
    X = torch.stack([e % W, (e // W) % H, e // (W * H)], dim=1)                           # [M][3] (x, y, z), x fastest
    g = 2.0 * X.double() / (Nf if mut == "lin_mismatch" else Nf - 1) - 1.0
    vox, dout, xf = d["vox"].double().reshape(n, M, C), d["dout"].double().reshape(n, M, C), d["xf"].double().view(n, 3, 4)
    slot = list(range(n)) if d["slot"] is None else d["slot"].tolist()
    out, dvox, dxf, pos = torch.zeros(n, M, C, dtype=torch.float64), torch.zeros(n, M, C, dtype=torch.float64), torch.zeros(n, 3, 4, dtype=torch.float64), {}
    for i in range(n):
        src, dst = (slot[i], i) if mut == "slot_side" else (i, slot[i])
        v, gd = vox[src], dout[dst]
        if d["mode"][i] == 0:
            out[dst], dvox[src] = v, gd
            continue
        A = xf[i]
        p = ((g @ A[:, :3].T + A[:, 3] + 1.0) * Nf - 1.0) * 0.5
        i0 = p.floor().long()
        fr = p - i0.double()
        o, gp, anyok = torch.zeros(M, C, dtype=torch.float64), torch.zeros(M, 3, dtype=torch.float64), torch.zeros(M, dtype=torch.bool)
        for k in range(8):
            dd = torch.tensor([k & 1, (k >> 1) & 1, k >> 2])
            ii = i0 + dd
            ok = ((ii >= 0) & (ii < Nl)).all(1)
            anyok |= ok
            wa = torch.where(dd.bool()[None, :], fr, 1.0 - fr)
            w = wa.prod(1) * ok
            iic = torch.minimum(ii.clamp_min(0), Nl - 1)
            flat = (iic[:, 2] * H + iic[:, 1]) * W + iic[:, 0]
            tap = v[flat]
            o += w[:, None] * tap
            wk = w * _box_keep(A, N, iic, X, mut) if (box or mut in ("swap_n", "drop_corner", "lost_sign")) else w
            dvox[src].index_add_(0, flat, wk[:, None] * gd)
            dot = (tap * gd).sum(1) * ok
            sg = (2 * dd - 1).double()
            gp[:, 0] += sg[0] * wa[:, 1] * wa[:, 2] * dot
            gp[:, 1] += sg[1] * wa[:, 0] * wa[:, 2] * dot
            gp[:, 2] += sg[2] * wa[:, 0] * wa[:, 1] * dot
        out[dst] = o
        gs = gp * Nf * 0.5                                     # d voxel coordinate / d s = N / 2 (align_corners=False)
        dxf[i, :, :3], dxf[i, :, 3] = gs.T @ g, gs.sum(0)
        pos[i] = (p, anyok)
    sh = (n, D, H, W, C)
    return {"out": out.view(sh), "dvox": dvox.view(sh), "dxf": dxf.view(n, 12), "pos": pos}


def clearance(c, d):
    """(smallest margin, smallest distance): over every sample with an in-range tap and every axis a, the distance of its float64 voxel coordinate to
    the nearest integer, less 32 u (N_a + 2) - the position chain is about 8 fp32 roundings of a value of at most N_a + 2; this is 4x that."""
    need = 32 * U * (torch.tensor([c.W, c.H, c.D], dtype=torch.float64) + 2)
    margin, dist = float("inf"), float("inf")
    for p, anyok in explicit(c, d)["pos"].values():
        if anyok.any():
            dd = (p[anyok] - p[anyok].round()).abs()
            margin, dist = min(margin, (dd - need).min().item()), min(dist, dd.min().item())
    return margin, dist


def fwd_bound(c, ref):
    return max(2e-5, 3 * max(c.D, c.H, c.W) * 2.0 ** -23) * max(1.0, ref.abs().max().item())


def dvox_bound(c, ref):
    return 1e-4 * ref.abs().max().item()


def row_errors(got, ref):
    """Per transform row a: max |got - ref| over the four entries of row a of all views, relative to that row's maximum of |ref| (0 where the reference row
    is all zero: then the result must be exactly zero too)."""
    e, r = (got.double() - ref).abs().view(-1, 3, 4), ref.abs().view(-1, 3, 4)
    out = []
    for a in range(3):
        m = r[:, a].max().item()
        if m == 0:
            assert e[:, a].max().item() == 0, "a row of zeros in the reference is not exactly zero"
        out.append(e[:, a].max().item() / m if m else 0.0)
    return out


def yardstick_threads():
    """Context: torch on one CPU thread. The float32 yardstick's sums then round in one order on every host, whatever its core count."""
    import contextlib

    @contextlib.contextmanager
    def one():
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            yield
        finally:
            torch.set_num_threads(n)
    return one()


def dxf_bounds(yard_rows, noise=0.0):
    """The bound per row from the float32 yardstick's row errors."""
    return [min(DXF_CAP, max(DXF_FLOOR, SHARP * y)) + noise for y in yard_rows]


# ---- device buffers of the GPU matrices (this one and the ray-marcher's)
GUARD = 64            # floats of pattern on either side of every output (256 bytes: the body keeps its 16-byte alignment)


def guarded(shape, dev, fill=None):
    """A float32 tensor of `shape` inside a pattern-filled allocation. fill None: the body holds the pattern too."""
    numel = 1
    for s in shape:
        numel *= s
    raw = torch.full((2 * GUARD + numel,), CANARY, dtype=torch.int32, device=dev)
    body = raw[GUARD:GUARD + numel].view(torch.float32).view(shape)
    if fill is not None:
        body.copy_(fill if torch.is_tensor(fill) else torch.full(shape, float(fill)))
    return raw, body


def finish(raw, body, what):
    torch.cuda.synchronize()
    host = raw.cpu()
    n = body.numel()
    guard = torch.cat([host[:GUARD], host[GUARD + n:]])
    assert (guard == CANARY).all(), (what, "an element outside the buffer was written", int((guard != CANARY).sum()))
    got = host[GUARD:GUARD + n].view(torch.float32).view(body.shape).clone()
    assert torch.isfinite(got).all(), (what, "an element was not written (or is not finite)", int((~torch.isfinite(got)).sum()))
    return got
