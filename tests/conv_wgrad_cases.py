"""The dispatch-space matrix of forge_conv_wgrad / forge_conv_wgrad_det: the documented contract restated in plain torch, and the case table.

tests/test_gpu_conv_wgrad_matrix.py launches every case of CASES through the C entry points (through convops.conv_wgrad for the launcher cases)
and measures it against evaluate() in float64; tests/test_conv_wgrad_reference_cpu.py pins evaluate() to independent torch code, asks
forge_conv_wgrad_plan (host-only) whether every case reaches the kernel and parameters it is in the table for, and validates the wrong references
(MUTATIONS) before a GPU is spent on them. Both import this module, so the table cannot drift between them.

evaluate() is written from the contract in include/forge_hip.h (the block above forge_conv_wgrad and the deterministic-mode block), not from the
kernels:
    dw[t][co][ci] = sum_m dy[m][co] x[voxel(m) is + tap_t][ci],      x = x1 | x2 along the channels, zero outside in_grid
as one explicit gather + one matmul per tap in the dtype asked for. In float64 it is the reference; with mag=True it returns the magnitude sum
S[t][co][ci] = sum_m |dy[m][co]| |x[..][ci]|, the error scale of the element (mag="both": the pair, from one pass).

Error model (as wino_cases states it for `wgrad`), u = 2^-24:
  unconditional  |got - ref| <= gamma_k S, k = M + 2, gamma_k = k u / (1 - k u): M products summed in ANY order over ANY chunking commit at most M - 1
                 additions and one rounding per product (exact inside an fmaf or MFMA) to an element; the two spare roundings cover the slab sum of
                 the deterministic mode (float64, rounded once) and the single add onto a prior. No fp32 evaluation of the contract can miss it.
  sharp          q = max |got - ref| / (u S) and q_rms, compared with SHARP x the same figures of a float32 CPU evaluation of the contract (yardstick())
                 at a stated grain. An element with S = 0 (a tap wholly outside the grid) must be exactly zero and then counts as q = 0.
Onto a prior p the result is p + dw within the same bounds plus one ulp of p.
"""
from collections import namedtuple

import torch

import conv_igemm_cases as cc

U = cc.U
SHARP = cc.SHARP
CANARY = cc.CANARY
FAMILY = {1: "tiles", 2: "small", 3: "lines", 4: "lines16"}

T27, T9, T25, T1, T27_SHUFFLED = cc.T27, cc.T9, cc.T25, cc.T1, cc.T27_SHUFFLED
T9_SHUFFLED = [T9[(4 * i + 1) % 9] for i in range(9)]
T28_9L = T27 + [(0, 0, 2)]                                   # 28 taps on 9 (dz, dy) lines: the most the line kernels take
T28_10L = T27 + [(2, 0, 0)]                                  # 28 taps on 10 lines
T29_9L = T27 + [(0, 0, 2), (0, 0, -2)]                       # 29 taps on 9 lines
DX3 = [(0, 0, -3), (0, 1, 0), (0, 0, 3), (0, -1, 1)]         # |dx| = 3: still a line kernel; at W = 3 the taps dx = +-3 lie wholly outside the grid
DX4 = [(0, 0, -4), (0, 1, 0), (0, 0, 4), (0, -1, 1)]         # |dx| = 4: not
T36 = [(0, ky - 2, kx - 2) for ky in range(6) for kx in range(6)]          # ConvTranspose2d(k6, s2, p2): 36 taps on 6 lines, dx -2..3
T35_7L = [(0, ky - 3, kx - 2) for ky in range(7) for kx in range(5)]       # 35 taps on 7 lines
T64 = [(kz - 1, ky - 1, kx - 1) for kz in range(4) for ky in range(4) for kx in range(4)]   # ConvTranspose3d(k4, s2, p1): the heads' up-convolution
T5_FAR = [(0, 0, -4), (0, 0, 4), (1, 1, 0), (0, 0, 0), (-1, 0, 2)]
T8_VALID = [(dz, dy, dx) for dz in (0, 1) for dy in (0, 2) for dx in (0, 4)]                # a "valid" convolution: the input grid is larger than the row grid

_FIELDS = "name rows n D H W C1 C2 Cout taps istride in_grid ldy ld1 ld2 views1 views2 launcher plan muts note"
Case = namedtuple("Case", _FIELDS)


def mk(name, rows, n, D, H, W, C1, Cout, taps, plan, C2=0, istride=1, in_grid=None, ldy=None, ld1=None, ld2=None, views1=None, views2=None,
       launcher=None, muts="", note=""):
    """plan = (family, CIW | CIT, TG | IS, waves per workgroup): what forge_conv_wgrad_plan must answer, for the atomic and the deterministic path.
    views = (tv, ti): the operand is view ti of a [n][tv] stack (batch stride tv x the volume). launcher: None = the C entry points;
    'concat' / 'chunk' = convops.conv_wgrad's two paths (its operands are dense in the channels: it reads the strides off the tensors)."""
    if in_grid is None:
        in_grid = (D * istride if D > 1 else 1, H * istride, W * istride)
    return Case(name, frozenset(rows.split()), n, D, H, W, C1, C2, Cout, list(taps), istride, tuple(in_grid), ldy or Cout, ld1 or C1, ld2 or C2,
                views1, views2, launcher, tuple(plan), tuple(muts.split()), note)


# The rows of the coverage table; test_conv_wgrad_reference_cpu.test_coverage_rows asserts that every one is reached and holds what its name says.
# Every case runs the atomic AND the deterministic path, so a fam_* row stands for both twins of the kernel.
ROWS = ("fam_tiles128 fam_tiles64 fam_tiles32 fam_tiles32_tg4 fam_tiles64_tg2 fam_small fam_lines fam_lines16_c16 fam_lines16_c32 fam_lines16_s2 "
        "ldy ld1 ld2 bs1 bs2 cout132 cout260 cin36 cin68 cin132 two_128_36 two_128_132 two_256_64 m_lt_16 m_not_16 chunk_in_row w1 w2 w3 w5 "
        "lines9 lines10 dx3 dx4 taps28 taps29 s2_lines6 s2_lines7 cout16 cout20 cin16 cin20 w_even w_odd m131072 m_below_131072 "
        "walk_lines walk_lines16_c16 walk_lines16_c32 walk_lines16_s2 small_s2 small_in_grid outside_tiles outside_small outside_lines outside_lines16 "
        "line_order s2_64taps launcher_concat launcher_chunk_bs1").split()

TI = (1, 128, 1, 4)
CASES = [
    # ---- the 128-row tiles: ragged Cout / Cin / C2 tiles, padded operands, ragged M, rows shorter than a K-step (the carry chain)
    mk("t_two36", "fam_tiles128 two_128_36 cout132 ldy ld1 ld2 bs1 bs2 w5 m_not_16", 2, 3, 7, 5, 128, 132, T27, TI, C2=36, ldy=140, ld1=136,
       ld2=44, views1=(3, 1), views2=(2, 1), muts="neg_taps wrap_border drop_last shift_x2 swap_line",
       note="M = 210. Reading ld1 as C1 (or ldy as Cout, ld2 as C2, bs as the volume) sums NaN padding here; a C2 tile of 36 in a 128-wide tile; "
            "dropping tap_ok's bounds test is wrong reference wrap_border"),
    mk("t_two132", "fam_tiles128 two_128_132 cout260 w5 m_not_16 chunk_in_row", 1, 2, 101, 5, 128, 260, cc.T3Z, TI, C2=132, ld2=136,
       muts="shift_x2 drop_last", note="M = 1010 in 3 chunks of 352 voxels: the boundaries fall inside rows; the second input takes two Cin tiles, the last of 4 channels; three Cout tiles"),
    mk("t_two64", "fam_tiles128 two_256_64 w1", 1, 1, 2500, 1, 256, 64, [(0, -1, 0), (0, 0, 0), (0, 1, 0), (1, 0, 0)], TI, C2=64,
       muts="dup_chunk_row drop_last", note="W = 1: every K-step of 16 voxels wraps 16 rows; M = 2500 runs as several chunks whose first row is "
                                            "wrong reference dup_chunk_row; tap (1, 0, 0) lies wholly outside the D = 1 grid"),
    mk("t_cin132", "fam_tiles128 cin132 m_lt_16 outside_tiles w5", 1, 1, 1, 5, 132, 36, [(0, 0, -1), (0, 0, 0), (0, 0, 5), (0, 1, 0)], TI,
       muts="bf16 drop_last", note="M = 5 < one K-step; taps (0, 0, 5) and (0, 1, 0) lie wholly outside the 1 x 5 grid: exact zeros; the bf16 mutation is "
                                   "only beyond the unconditional bound at an M this small"),
    mk("t_cin68", "fam_tiles128 cin68 w2 m_not_16", 3, 1, 7, 2, 68, 40, T9, TI, ld1=72, views1=(2, 0), note="M = 42: W = 2, H = 7: a K-step wraps rows and batch elements"),
    mk("t_cin36", "fam_tiles64 cin36 w3 ld1 ldy", 2, 2, 5, 3, 36, 36, T27, (1, 64, 1, 4), ld1=40, ldy=44, muts="neg_taps wrap_border",
       note="M = 60; Cin 36 in the 64-wide tile"),
    mk("t_w_odd", "fam_tiles32 w_odd dx4", 2, 2, 6, 9, 20, 20, DX4, (1, 32, 1, 4), ld1=24, muts="neg_taps",
       note="M = 216; narrow channels, |dx| = 4 and W odd: neither a line kernel nor the small one"),
    mk("t_s2_7l", "fam_tiles32 s2_lines7 w_odd", 2, 1, 9, 7, 16, 16, T35_7L, (1, 32, 1, 4), istride=2, muts="stride_on_tap",
       note="stride 2 on 7 lines (the stride-2 line kernel takes 6), W odd"),
    # ---- tap-grouped tiles: from M = 131072 only
    mk("g_tg4", "fam_tiles32_tg4 m131072", 2, 1, 256, 256, 32, 64, T9, (1, 32, 4, 4), ld1=36, muts="neg_taps",
       note="9 taps in groups of 4: the last group holds one tap and three absent ones"),
    mk("g_below", "m_below_131072", 1, 1, 511, 256, 32, 64, T9, (1, 32, 1, 4), note="M = 130816: the same problem one row short of grouping"),
    mk("g_tg2", "fam_tiles64_tg2", 1, 2, 256, 256, 40, 36, cc.T3Z, (1, 64, 2, 4), ldy=40, muts="neg_taps",
       note="3 taps in groups of 2, Cin 40 of 64 columns per tap"),
    mk("g_s2_64", "s2_64taps", 1, 2, 256, 256, 32, 36, T64, (1, 32, 4, 4), istride=2,
       note="the heads' ConvTranspose3d(k4, s2, p1) weight gradient: 64 taps gathered on the 2x finer grid, the smallest M that is grouped"),
    # ---- the small kernel (independent waves)
    mk("s_far", "fam_small w_even dx4 ldy ld1 bs1 outside_small", 2, 3, 5, 4, 20, 12, DX4, (2, 32, 4, 4), ldy=16, ld1=28, views1=(2, 1),
       muts="neg_taps wrap_border", note="M = 120; at W = 4 the taps dx = +-4 lie wholly outside"),
    mk("s_w2", "fam_small w2 lines10 taps28 m_not_16", 1, 5, 7, 2, 32, 32, T28_10L, (2, 32, 4, 4), muts="swap_line",
       note="M = 70; 28 taps on 10 lines: one line too many for the line kernels; W = 2: a lane's walk of 2 voxels wraps a row every step"),
    mk("s_t29", "fam_small taps29", 1, 3, 5, 6, 16, 16, T29_9L, (2, 32, 4, 4), note="29 taps on 9 lines: one tap too many; 8 tap groups, the last with one tap"),
    mk("s_s2", "fam_small small_s2 s2_lines7", 2, 1, 9, 6, 16, 16, T35_7L, (2, 32, 4, 4), istride=2, ld1=20, muts="stride_on_tap neg_taps",
       note="stride 2 on 7 lines, W even"),
    mk("s_valid", "fam_small small_in_grid", 2, 2, 5, 6, 8, 8, T8_VALID, (2, 32, 4, 4), in_grid=(3, 7, 10), views1=(2, 1), muts="neg_taps",
       note="in_grid != grid at stride 1 (a 'valid' convolution): Hi, Wi, Di must index the operand, not H, W, D"),
    mk("s_chunks", "fam_small chunk_in_row", 1, 1, 250, 10, 8, 8, T5_FAR, (2, 32, 4, 4), muts="dup_chunk_row", note="M = 2500 in chunks of 256 voxels: boundaries inside rows"),
    # ---- the line kernels: 32 x 32 MFMA, and the 16 x 16 x 4 forms
    mk("l_9l", "fam_lines lines9 taps28 cout20 ldy ld1 bs1 w5", 2, 3, 6, 5, 20, 20, T28_9L, (3, 32, 1, 4), ldy=24, ld1=28, views1=(3, 2),
       muts="neg_taps wrap_border swap_line drop_last", note="28 taps on 9 lines; Cout = Cin = 20"),
    mk("l_dx3", "fam_lines dx3 w3 outside_lines walk_lines line_order", 1, 1, 520, 3, 32, 32, DX3, (3, 32, 1, 4), muts="swap_line wrap_border",
       note="520 segments on 512 persistent workgroups; at W = 3 taps dx = +-3 lie wholly outside; the taps are not in line order (tap[t][3] = 0, 1, 0, 2)"),
    mk("l_w70", "fam_lines line_order", 1, 2, 3, 70, 32, 24, T27_SHUFFLED, (3, 32, 1, 4), muts="swap_line", note="W = 70: three segments per row, the last of 6 voxels; shuffled taps"),
    mk("l16_c16", "fam_lines16_c16 cout16 cin16 w2 walk_lines16_c16 line_order", 1, 1, 1030, 2, 16, 16, T9_SHUFFLED + [(0, 2, 0)], (4, 16, 1, 4),
       ldy=20, ld1=20, muts="swap_line drop_last", note="1030 segments on 1024 persistent workgroups"),
    mk("l16_c20", "fam_lines16_c32 cin20 cout16 walk_lines16_c32 w1 outside_lines16", 1, 1, 520, 1, 20, 16, T9, (4, 32, 1, 8), ld1=24,
       muts="wrap_border", note="W = 1: every dx != 0 tap lies wholly outside; 520 segments on 512 workgroups of 8 waves"),
    mk("l16_c32", "fam_lines16_c32 lines9 ldy bs1", 2, 3, 4, 37, 32, 8, T27, (4, 32, 1, 8), ldy=12, views1=(2, 1), muts="neg_taps swap_line"),
    mk("l16_s2", "fam_lines16_s2 s2_lines6 walk_lines16_s2 w2 ld1", 1, 1, 775, 2, 16, 16, T36, (4, 16, 2, 4), istride=2, ld1=20,
       muts="stride_on_tap wrap_border swap_line", note="conv_rgb's ConvTranspose2d(k6, s2, p2): 775 segments on 768 persistent workgroups"),
    mk("l16_s2_w", "fam_lines16_s2 bs1", 2, 1, 5, 37, 12, 8, T36, (4, 16, 2, 4), istride=2, views1=(2, 0), muts="stride_on_tap", note="W = 37: two segments per row, the second of 5 voxels, gathered with a row stride of 2"),
    # ---- convops.conv_wgrad's own paths
    mk("p_concat", "launcher_concat", 2, 2, 5, 6, 64, 40, T27, (1, 128, 1, 4), C2=32, launcher="concat", muts="shift_x2",
       note="two inputs with C1 % 128 != 0: the launcher concatenates them (Cin = 96 in one 128-wide tile)"),
    mk("p_chunk", "launcher_chunk_bs1 bs1", 3, 2, 5, 6, 128, 40, T27, (1, 128, 1, 4), C2=32, views1=(2, 1), launcher="chunk", muts="drop_last",
       note="MAX_OPERAND_BYTES lowered to two batch elements: 3 run as 2 + 1, the second launch adds onto the first"),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

MUTATIONS = ("neg_taps", "wrap_border", "drop_last", "dup_chunk_row", "shift_x2", "stride_on_tap", "swap_line", "bf16")
MUTATION_CASES = [(c.name, c.muts) for c in CASES if c.muts]

# Boundary pairs: (row a, row b) must both be reached, by cases whose plans differ.
BOUNDARIES = (("lines9", "lines10"), ("dx3", "dx4"), ("taps28", "taps29"), ("s2_lines6", "s2_lines7"), ("cout16", "cout20"), ("cin16", "cin20"),
              ("w_even", "w_odd"), ("m131072", "m_below_131072"))
BOUNDARY_CASES = {"lines9": "l_9l", "lines10": "s_w2", "dx3": "l_dx3", "dx4": "t_w_odd", "taps28": "l_9l", "taps29": "s_t29", "s2_lines6": "l16_s2",
                  "s2_lines7": "s_s2", "cout16": "l16_c20", "cout20": "l_9l", "cin16": "l16_c16", "cin20": "l16_c20", "w_even": "s_far", "w_odd": "t_w_odd",
                  "m131072": "g_tg4", "m_below_131072": "g_below"}


def M_of(c):
    return c.n * c.D * c.H * c.W


def Cin_of(c):
    return c.C1 + c.C2


def gamma(c):
    k = (M_of(c) + 2) * U
    return k / (1 - k)


def is_big(c):
    return M_of(c) >= 100000


def chunk_limit(c):
    """MAX_OPERAND_BYTES of the 'chunk' launcher case: room for two batch elements of the widest operand."""
    vol = c.in_grid[0] * c.in_grid[1] * c.in_grid[2]
    bs1 = vol * (c.views1[0] if c.views1 else 1)
    return max((bs1 + vol) * c.ld1 * 4, 2 * c.D * c.H * c.W * c.ldy * 4, 2 * vol * max(c.ld2, 1) * 4)


def make_data(c):
    """Seeded float32 operands in their logical (dense) form: dy [n][D][H][W][Cout], x1 / x2 [n][Di][Hi][Wi][C] ~ N(0, 1), prior [ntaps][Cout][Cin]."""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)))
    Di, Hi, Wi = c.in_grid
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"dy": rn(c.n, c.D, c.H, c.W, c.Cout), "x1": rn(c.n, Di, Hi, Wi, c.C1), "x2": rn(c.n, Di, Hi, Wi, c.C2) if c.C2 else None,
            "prior": rn(len(c.taps), c.Cout, Cin_of(c))}


def gather(x, D, H, W, vmul, tap, wrap=False):
    """x [n][Di][Hi][Wi][C] -> [n D H W][C]: the row of voxel (z, y, x) is input voxel (z vmul + dz, y vmul + dy, x vmul + dx), zero outside the input
    grid. wrap (a WRONG reading): an x outside [0, Wi) is not refused but carried into the flat index of the batch element's volume."""
    n, Di, Hi, Wi, C = x.shape
    z = (torch.arange(D) * vmul + tap[0])[:, None, None]
    y = (torch.arange(H) * vmul + tap[1])[None, :, None]
    xx = (torch.arange(W) * vmul + tap[2])[None, None, :]
    ok = (z >= 0) & (z < Di) & (y >= 0) & (y < Hi)
    e = (z * Hi + y) * Wi + xx
    ok = ok & ((e >= 0) & (e < Di * Hi * Wi) if wrap else (xx >= 0) & (xx < Wi))
    rows = x.reshape(n, Di * Hi * Wi, C)[:, e.clamp(0, Di * Hi * Wi - 1).reshape(-1)]
    return torch.where(ok.reshape(1, -1, 1), rows, torch.zeros((), dtype=x.dtype)).reshape(n * D * H * W, C)


def swapped_lines(taps):
    """Tap 0 takes the (dz, dy) line of the last tap on another line and gives it its own; both keep their dx."""
    u = max(i for i, t in enumerate(taps) if t[:2] != taps[0][:2])
    out = list(taps)
    out[0], out[u] = taps[u][:2] + taps[0][2:], taps[0][:2] + taps[u][2:]
    return out


def evaluate(c, d, dtype=torch.float64, grain=None, mag=False, mut=None, mchunk=0, corner=None):
    """The contract evaluated in `dtype` on the CPU: dw [ntaps][Cout][Cin] (mag: the magnitude sums S).
    grain None: one matmul per tap over all M voxels. grain = g voxels (the float32 yardsticks): the voxels are cut into chunks of `mchunk` (0: one
    chunk) and each chunk into steps of g; a step's partial product is one matmul (g > 2) or, for g <= 2, exact products added to the running sum and
    rounded once (the fmaf chain, two voxels per MFMA); steps add to the chunk's sum in order, chunk sums to the result in chunk order.
    corner = (taps, co, ci): only that leading block of the elements. mut: one of MUTATIONS - a deliberately WRONG reading of the contract."""
    assert mut is None or mut in MUTATIONS
    T, Co, Ci = (min(a, b) for a, b in zip(corner or (1 << 30,) * 3, (len(c.taps), c.Cout, Cin_of(c))))
    M = M_of(c)
    cv = (lambda t: t.bfloat16().to(dtype)) if mut == "bf16" else (lambda t: t.to(dtype))
    dy = cv(d["dy"]).reshape(M, c.Cout)[:, :Co]
    x1, x2 = cv(d["x1"]), (cv(d["x2"]) if c.C2 else None)
    if mut == "shift_x2":
        x2 = x2.roll(1, dims=-1)
    if mut in ("drop_last", "dup_chunk_row"):
        r = M - 1 if mut == "drop_last" else (mchunk if 0 < mchunk < M else min(32, M // 2))
        dy = dy.clone()
        dy[r] *= 0 if mut == "drop_last" else 2
    taps = [tuple(-v for v in t) for t in c.taps] if mut == "neg_taps" else swapped_lines(c.taps) if mut == "swap_line" else c.taps
    if mag is True:
        dy = dy.abs()
    out = torch.zeros(T, Co, Ci, dtype=dtype)
    outS = torch.zeros(T, Co, Ci, dtype=dtype) if mag == "both" else None
    for t in range(T):
        tap = tuple(v * c.istride for v in taps[t]) if mut == "stride_on_tap" else taps[t]
        vmul = 1 if mut == "stride_on_tap" else c.istride
        X = gather(x1, c.D, c.H, c.W, vmul, tap, wrap=mut == "wrap_border")
        if x2 is not None:
            X = torch.cat([X, gather(x2, c.D, c.H, c.W, vmul, tap, wrap=mut == "wrap_border")], dim=1)
        X = X[:, :Ci]
        if mag is True:
            X = X.abs()
        if grain is None:
            out[t] = dy.t() @ X
            if mag == "both":
                outS[t] = dy.abs().t() @ X.abs()
            continue
        mc = mchunk if mchunk > 0 else M
        nch = (M + mc - 1) // mc
        pad = lambda r: torch.cat([r, r.new_zeros(nch * mc - M, r.shape[1])]).view(nch, mc, -1)      # zero rows add exact zeros: no rounding changes
        A, B = pad(dy).transpose(1, 2), pad(X)                     # all chunks side by side: they are independent until their sums are added
        acc = torch.zeros(nch, Co, Ci, dtype=dtype)
        for s0 in range(0, mc, grain):
            a, b = A[:, :, s0:s0 + grain], B[:, s0:s0 + grain]
            acc = (a.double() @ b.double() + acc.double()).to(dtype) if grain <= 2 else acc + a @ b
        for k in range(nch):
            out[t] += acc[k]
    return (out, outS) if mag == "both" else out


def reference(c, d):
    """(float64 dw, magnitude sums S), from one pass over the gathered rows."""
    return evaluate(c, d, mag="both")


def q_stats(c, ref, S, got, prior=None):
    """(q, q_rms, worst ratio to the unconditional bound, flat index of the worst element) of `got` against ref (+ prior), over EVERY element.
    An element with S = 0 must equal the prior exactly."""
    want = ref if prior is None else ref + prior.double()
    slack = 0 if prior is None else (torch.nextafter(prior.abs(), torch.full_like(prior, float("inf"))) - prior.abs()).double()    # one ulp of the prior
    e = ((got.double() - want).abs() - slack).clamp_min(0)
    zero = S == 0
    assert torch.isfinite(e).all(), (c.name, "non-finite error")
    assert (e[zero] == 0).all(), (c.name, "an element no product reaches is not exactly its prior", int((e[zero] != 0).sum()))
    r = torch.where(zero, torch.zeros_like(e), e / (U * S).masked_fill(zero, 1.0))
    return r.max().item(), r.square().mean().sqrt().item(), r.max().item() * U / gamma(c), int(r.argmax())


def poisoned(x, ld, views):
    """cc.poisoned with NaN everywhere the contract does not feed: padding columns [C, ld), the other views of the [n][tv] stack (batch gaps), guard rows."""
    return cc.poisoned(x, ld, 0, views, float("nan"))


def plan_shape(c):
    """(C1, C2) as the kernel sees them: the 'concat' launcher path joins the inputs first."""
    return (c.C1 + c.C2, 0) if c.launcher == "concat" else (c.C1, c.C2)


def query_plan(c, det, taps=None, n=None):
    """forge_conv_wgrad_plan (host-only) -> (rc, dict)."""
    import ctypes

    from forge_amd import _lib
    taps = c.taps if taps is None else taps
    ta = (ctypes.c_int * (3 * len(taps)))(*[v for t in taps for v in t])
    out = (ctypes.c_longlong * 8)()
    C1, C2 = plan_shape(c)
    rc = _lib.lib().forge_conv_wgrad_plan(C1, C2, n or c.n, c.D, c.H, c.W, c.istride, *c.in_grid, c.Cout, ta, len(taps), det, out)
    return rc, dict(zip("family p1 p2 nwv grid nchunk mchunk nlines".split(), out))


def plan_text(p):
    return "%s<%d,%d>x%d grid %d chunks %d mchunk %d lines %d" % (FAMILY[p["family"]], p["p1"], p["p2"], p["nwv"], p["grid"], p["nchunk"], p["mchunk"], p["nlines"])
