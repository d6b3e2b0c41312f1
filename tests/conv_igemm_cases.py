"""The launch-space matrix of forge_conv_igemm: its documented contract restated in plain torch, and the case table.

tests/test_gpu_conv_igemm_matrix.py launches every case x plan of CASES through convops.conv_igemm and measures it against evaluate() in
float64; tests/test_conv_igemm_reference_cpu.py pins evaluate() to independent torch code, checks that every case reaches the plan it is in
the table for, and validates the wrong references (MUTATIONS) before a GPU is spent on them. Both import this module, so the table cannot
drift between them.

evaluate() is written from the contract in include/forge_hip.h (the block above forge_conv_igemm), not from the kernel: a tap-by-tap
gather + matmul in the dtype asked for. In float64 it is the reference; in float32 (accumulating tap by tap, or per K-step and split-K
slice) it is the yardstick the kernel's rounding error is measured against. Besides the outputs it returns, per output element, the two
parts of an error scale sigma = sigma_S + sigma_A:
  sigma_S   the magnitude sum S[m][co] = |bias| + sum |x||w| of the pre-activation, carried through the epilogue with its Lipschitz constant
            (LeakyReLU max(1, |slope|), sigmoid 1/4, tanh 1) and the factors it is multiplied by (|scale|, |h|, |z|)
  sigma_A   the magnitudes of the operands the epilogue itself adds or rounds (|shift|, |residual|, |h (1 - z)|, the result of expf / tanhf)
Any fp32 evaluation of the sum satisfies |acc - ref| <= gamma S, gamma = (K + 2) u / (1 - (K + 2) u), u = 2^-24, K = ntaps (C1 + C2); the
epilogue's own operations add at most EPI_ULPS ulps of their operands' magnitudes, so
  unconditional bound = gamma sigma_S + EPI_ULPS 2 u sigma_A,           sharp statistic q = |got - ref| / (u (sigma_S + sigma_A)).
EPI_ULPS: the ROCm installation documents no ulp bounds for expf / tanhf; torch's CPU float32 exp / tanh / sigmoid measure <= 2 ulps against
float64 (test_conv_igemm_reference_cpu.test_epilogue_ulps); 4 ulps are granted to each of expf, tanhf, the division of the sigmoid and
every fmaf / add / multiply of an epilogue (at most 4 of them in a chain): EPI_ULPS = 16.
"""
from collections import namedtuple

import torch

U = 2.0 ** -24
EPI_ULPS = 16
SHARP = 4.0                     # the HIP result gets 4x the float32 CPU yardstick's q and q_rms (the margin of test_training_gradients_vs_float64_reference)
TILE_BM = {"A": 128, "B": 64, "C": 128, "D": 64, "E": 128}      # rows per workgroup tile, as the contract's `stats` paragraph states them
ALL_TILES = ("A", "B", "C", "D", "E")
CANARY = 0x7FC0BEEF             # a quiet NaN with a known payload: what every element the contract does not name must still hold after a launch

T27 = [(kz - 1, ky - 1, kx - 1) for kz in range(3) for ky in range(3) for kx in range(3)]
T9 = [(0, ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
T25 = [(0, ky - 2, kx - 2) for ky in range(5) for kx in range(5)]
T1 = [(0, 0, 0)]
T3Z = [(-1, 0, 0), (0, 0, 0), (1, 0, 0)]
T27_SHUFFLED = [T27[(7 * i + 3) % 27] for i in range(27)]           # the same 27 taps, not in x-line order


def phase_taps(k, pad, nd):
    """Tap lists of the 2^nd output phases of a stride-2 transposed convolution (kernel k, padding pad), phase p = pz*4 + py*2 + px: output
    o = 2 i - pad + kk, so phase ph takes every kk = ph + pad (mod 2) at input offset d = (ph + pad - kk) / 2. [(phase, taps, kernel indices)]."""
    ax = {ph: [((ph + pad - kk) // 2, kk) for kk in range(k) if (kk - ph - pad) % 2 == 0] for ph in (0, 1)}
    out = []
    for pz in ((0, 1) if nd == 3 else (0,)):
        for py in (0, 1):
            for px in (0, 1):
                taps, idx = [], []
                for dz, kz in (ax[pz] if nd == 3 else [(0, None)]):
                    for dy, ky in ax[py]:
                        for dx, kx in ax[px]:
                            taps.append((dz, dy, dx))
                            idx.append((kz, ky, kx))
                out.append(((pz, py, px), taps, idx))
    return out


PH3 = phase_taps(4, 1, 3)        # ConvTranspose3d(k4, s2, p1): 8 phases x 8 taps
PH2 = phase_taps(6, 2, 2)        # ConvTranspose2d(k6, s2, p2): 4 phases x 9 taps
MERGED8 = [t for _, tp, _ in PH3 for t in tp]
MERGED4 = [t for _, tp, _ in PH2 for t in tp]

_FIELDS = ("name rows n D H W C1 C2 Cout taps istride in_grid ostride phase out_grid epi slope bias residual out2 out3 lift "
           "ld1 off1 ld2 off2 views1 views2 ldo plans stats limit note")
Case = namedtuple("Case", _FIELDS)
_DEFAULTS = dict(C2=0, istride=1, in_grid=None, ostride=1, phase=(0, 0, 0), out_grid=None, epi=0, slope=1.0, bias=True, residual=False, out2=False,
                 out3=False, lift=0, ld1=None, off1=0, ld2=None, off2=0, views1=None, views2=None, ldo=None, plans=None, stats=False, limit=None, note="")


def _plans(tiles=ALL_TILES, splits=()):
    """Every tile un-split, then the given (tile, ksplit) pairs."""
    return tuple((t, 1) for t in tiles) + tuple(splits)


def mk(name, rows, n, D, H, W, C1, Cout, taps, **kw):
    d = dict(_DEFAULTS, **kw)
    if d["in_grid"] is None:
        d["in_grid"] = (D * d["istride"] if D > 1 else 1, H * d["istride"], W * d["istride"])
    if d["out_grid"] is None:
        d["out_grid"] = (D * d["ostride"] if D > 1 else D, H * d["ostride"], W * d["ostride"])
    if d["plans"] is None:
        d["plans"] = (("N", 1),) if Cout <= 16 else _plans()
    d["ld1"] = d["ld1"] or C1
    d["ld2"] = d["ld2"] or d["C2"]
    d["ldo"] = d["ldo"] or Cout
    return Case(name=name, rows=frozenset(rows.split()), n=n, D=D, H=H, W=W, C1=C1, Cout=Cout, taps=list(taps), **d)


# The rows of the coverage table; test_conv_igemm_reference_cpu.test_coverage_rows asserts that every one is reached and holds what its name says.
ROWS = ("tiles splitk splitk_epi0 splitk_epi1 splitk_residual splitk_strided splitk_phase splitk_lift splitk_one_step_per_slice "
        "kloop1 kloop2 kloop3 k27x256 ragged_m cout17 cout20 cout33 cout40 cout96 cout130 cout257 ncout1 ncout3 ncout8 ncout16 "
        "epi0 epi1_slope1 epi1_slope0 epi1_slope001 epi1_residual epi1_plain epi2_plain epi2_residual epi2_out3 epi3_plain epi3_out2 epi3_out3 "
        "epi3_residual map_plain map_s2_2d map_s2_3d map_phase map_merged8 map_merged4 map_merged4_narrow lift2 lift32 lift_residual "
        "ld1 ld2 bs1 bs2 ldo chunk_bs1 chunk_lift chunk_gru narrow_lines1 narrow_lines2 narrow_generic_shuffled narrow_generic_w_le_r "
        "narrow_strided narrow_w2 narrow_w3 narrow_w5 narrow_w70 narrow_epi1_residual large_grid stats").split()

_SPLITS_D = tuple(("D", k) for k in (2, 3, 4, 6, 8))
CASES = [
    # ---- K loop lengths and the tile x split-K product on a ragged M (168 rows: no multiple of 32 / 64 / 128 / 256)
    mk("plain27", "tiles splitk splitk_epi0 ragged_m cout96 epi0 map_plain", 1, 4, 6, 7, 64, 96, T27,
       plans=_plans(splits=_SPLITS_D + (("A", 2), ("A", 8), ("B", 3), ("C", 4), ("E", 6)))),
    mk("k1", "kloop1 cout40 ragged_m epi0", 2, 1, 9, 11, 32, 40, T1),
    mk("k2", "kloop2 cout33 epi1_slope0 epi1_plain", 2, 1, 9, 11, 32, 33, T1, C2=32, epi=1, slope=0.0, note="odd Cout: the plan refuses split-K"),
    mk("k3", "kloop3 cout20 splitk_one_step_per_slice splitk_epi0", 1, 5, 6, 7, 32, 20, T3Z, plans=_plans(splits=(("D", 2), ("D", 3), ("A", 3), ("B", 3)))),
    mk("k27x256", "k27x256 splitk_epi1 splitk_residual epi1_slope001 epi1_residual", 1, 3, 5, 6, 128, 64, T27, C2=128, epi=1, slope=0.01, residual=True,
       plans=_plans(splits=(("D", 8), ("A", 4), ("B", 6)))),
    mk("cout17", "cout17 ragged_m", 1, 1, 9, 15, 32, 17, T9),
    mk("cout130", "cout130 epi1_slope1", 1, 1, 9, 15, 32, 130, T9, epi=1, slope=1.0),
    mk("cout257", "cout257", 1, 1, 7, 11, 32, 257, T1, bias=False),
    mk("slope1_res", "epi1_slope1 epi1_residual", 1, 1, 9, 15, 32, 40, T9, epi=1, slope=1.0, residual=True),
    # ---- the direct GRU epilogues (Cout = 2 Ch for the gates)
    mk("gates", "epi2_plain", 2, 3, 5, 7, 32, 40, T27, C2=32, epi=2),
    mk("gates_res", "epi2_residual epi2_out3 chunk_gru", 2, 3, 5, 7, 32, 40, T27, C2=32, epi=2, residual=True, out3=True, limit="half"),
    mk("state", "epi3_plain", 2, 3, 5, 7, 32, 40, T27, C2=32, epi=3),
    mk("state_full", "epi3_out2 epi3_out3 epi3_residual", 2, 3, 5, 7, 32, 40, T27, C2=32, epi=3, residual=True, out2=True, out3=True, ldo=44),
    # ---- output mappings
    mk("s2_2d", "map_s2_2d splitk_strided", 2, 1, 5, 6, 64, 32, T9, istride=2, epi=1, slope=0.01, residual=True, plans=_plans(splits=(("D", 2), ("A", 4)))),
    mk("s2_3d", "map_s2_3d splitk_strided", 1, 3, 4, 5, 32, 36, T27, istride=2, plans=_plans(splits=(("D", 3), ("C", 2)))),
] + [
    mk("phase%d%d%d" % ph, "map_phase splitk_phase", 2, 3, 4, 5, 64, 32, tp, ostride=2, phase=ph, epi=1, slope=0.01, residual=True,
       plans=_plans(splits=(("D", 2), ("B", 4), ("A", 8))))
    for ph, tp, _ in PH3
] + [
    mk("merged8", "map_merged8", 2, 3, 4, 5, 64, 32, MERGED8, ostride=2, phase="merged", epi=1, slope=0.01, residual=True),
    mk("merged4", "map_merged4", 2, 1, 5, 7, 32, 24, MERGED4, ostride=2, phase="merged"),
    mk("merged4_n", "map_merged4_narrow ncout3", 2, 1, 5, 7, 16, 3, MERGED4, ostride=2, phase="merged", epi=1, slope=0.0),
    mk("lift2", "lift2 lift_residual", 2, 1, 6, 7, 64, 128, T1, epi=1, slope=0.0, residual=True, lift=2, plans=_plans(splits=(("D", 2),))),
    mk("lift32", "lift32 splitk_lift", 2, 1, 6, 7, 64, 96, T9, epi=1, slope=0.01, lift=32, plans=_plans(splits=(("D", 2), ("A", 6)))),
    # ---- operand addressing: channel slices of wider tensors, views of a [b][t] stack in place, padded output rows, batch chunking
    mk("slices", "ld1 ld2 ldo", 2, 2, 5, 6, 32, 40, T27, C2=64, ld1=44, off1=4, ld2=76, off2=8, ldo=48, epi=1, slope=0.01, residual=True,
       plans=_plans(splits=(("D", 2),))),
    mk("views", "bs1 bs2", 3, 2, 5, 6, 32, 36, T27, C2=32, views1=(3, 1), views2=(2, 1)),
    mk("chunk_bs1", "chunk_bs1", 3, 2, 5, 6, 32, 36, T27, views1=(3, 2), ld1=36, off1=4, ldo=40, epi=1, slope=0.0, residual=True, limit="two",
       plans=_plans(splits=(("D", 2),))),
    mk("chunk_lift", "chunk_lift", 3, 1, 6, 7, 64, 128, T9, epi=1, slope=0.01, residual=True, lift=2, limit="two", plans=_plans(splits=(("D", 3),))),
    # ---- the Cout <= 16 kernels: x-line forms R = 1 / 2, the generic one; rows crossing x-line ends inside a 256-row tile
    mk("n_l1_w2", "narrow_lines1 narrow_w2 ncout16", 1, 4, 37, 2, 16, 16, T27),
    mk("n_l1_w70", "narrow_lines1 narrow_w70 ncout8 narrow_epi1_residual", 1, 1, 6, 70, 32, 8, T9, epi=1, slope=0.01, residual=True),
    mk("n_l2_w3", "narrow_lines2 narrow_w3 ncout3", 1, 1, 90, 3, 16, 3, T25),
    mk("n_l2_w5", "narrow_lines2 narrow_w5 ncout1", 1, 1, 60, 5, 16, 1, T25, C2=16, epi=1, slope=0.0, residual=True, ldo=4),
    mk("n_gen_shuf", "narrow_generic_shuffled ncout3", 1, 3, 19, 5, 16, 3, T27_SHUFFLED),
    mk("n_gen_w2", "narrow_generic_w_le_r", 1, 1, 150, 2, 16, 8, T25),
    mk("n_s2", "narrow_strided", 2, 1, 13, 11, 16, 8, T9, istride=2),
    # ---- a product-shaped launch of 2048 workgroups on tile D (512 on tile A, 2048 on tile E): every XCD slot of the remap
    mk("grid2048", "large_grid", 2, 16, 32, 32, 64, 256, T27, C2=64),
    # ---- the statistics by-product on 273 rows: tiles of 128 rows leave blocks 9-11 wholly past M, tiles of 64 rows block 9
    mk("stats", "stats", 1, 3, 7, 13, 32, 40, T27, stats=True),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

MUTATIONS = ("drop_tap", "mirror_dx", "zero_last_kstep", "rot_in2", "no_bias", "res_after", "swap_z", "shift_block")
# (case, wrong references it must reject)
MUTATION_CASES = [
    ("plain27", ("drop_tap", "mirror_dx", "zero_last_kstep", "no_bias", "shift_block")),
    ("k27x256", ("drop_tap", "zero_last_kstep", "rot_in2", "res_after", "shift_block")),
    ("state_full", ("swap_z", "rot_in2", "mirror_dx")),
    ("n_l2_w5", ("drop_tap", "mirror_dx", "res_after", "no_bias")),
]


def narrow_form(case):
    """Which Cout <= 16 kernel the documented rule picks: R (1 or 2) when the launch is a stride-1 convolution on its own grid whose taps are
    complete x-lines [(dz, dy)] x [dx = -R .. R], dx fastest, and W > R; 0 = the generic kernel."""
    if case.Cout > 16 or case.istride != 1 or case.ostride != 1 or case.phase == "merged":
        return 0
    for r in (1, 2):
        nt = 2 * r + 1
        if len(case.taps) % nt == 0 and case.W > r and all(
                tp[2] == (t % nt) - r and tp[:2] == case.taps[t - t % nt][:2] for t, tp in enumerate(case.taps)):
            return r
    return 0


def chunks(case):
    """Batch elements per launch of convops.conv_igemm under operand_limit(case)."""
    if case.limit is None:
        return [case.n]
    nc = 2 if case.limit == "two" else 1
    return [min(nc, case.n - s) for s in range(0, case.n, nc)]


def kstep(case):
    return 16 if case.Cout <= 16 else 32


def K_of(case):
    return len(case.taps) * (case.C1 + case.C2)


def nphase(case):
    if case.phase != "merged":
        return 1
    return 8 if case.out_grid[0] == 2 * case.D else 4


def stats_blocks(M, tile):
    bm = TILE_BM[tile]
    return ((M + bm - 1) // bm) * (bm // 32)


def can_split(case):
    """The contract's conditions for split-K (epilogues 0 / 1, no merged phases, Cout and ldo multiples of 4)."""
    return case.Cout > 16 and nphase(case) == 1 and case.epi in (0, 1) and case.Cout % 4 == 0 and case.ldo % 4 == 0


def operand_limit(case):
    """MAX_OPERAND_BYTES for a chunked case: 'two' = room for two batch elements (3 run as 2 + 1), 'half' = for one (2 run as 1 + 1)."""
    if case.limit is None:
        return None
    rows = case.in_grid[0] * case.in_grid[1] * case.in_grid[2]
    keep = 2 if case.limit == "two" else 1
    worst = 0
    for ld, views in ((case.ld1, case.views1), (case.ld2, case.views2)):
        if ld:
            bs = rows * (views[0] if views else 1)
            worst = max(worst, ((keep - 1) * bs + rows) * ld * 4)
    return worst


def out_desc(case):
    """{output name: (rows, width, row stride)} of the tensors the launch writes."""
    Do, Ho, Wo = case.out_grid
    rows = case.n * Do * Ho * Wo
    if case.lift:
        return {"out": (case.n * case.lift * case.H * case.W, case.Cout // case.lift, case.Cout // case.lift)}
    if case.epi == 2:
        Ch = case.Cout // 2
        d = {"out": (rows, Ch, Ch), "out2": (rows, Ch, Ch)}
        if case.out3:
            d["out3"] = (rows, Ch, Ch)
        return d
    d = {"out": (rows, case.Cout, case.ldo)}
    if case.epi == 3:
        if case.out2:
            d["out2"] = (rows, case.Cout, case.ldo)
        if case.out3:
            d["out3"] = (rows, case.Cout, case.ldo)
    return d


def make_data(case):
    """Seeded float32 operands in their logical (dense) form: x1 / x2 [n][Di][Hi][Wi][C], wp [ntaps][Cout][Cin] ~ N(0, 1 / K) so that the
    pre-activations are O(1) around an O(1) bias, scale in [0.5, 1.5), shift / residual / h ~ N(0, 1), z in (0, 1)."""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)))
    Di, Hi, Wi = case.in_grid
    Cin = case.C1 + case.C2
    rn = lambda *s: torch.randn(*s, generator=g)
    d = {"x1": rn(case.n, Di, Hi, Wi, case.C1), "x2": rn(case.n, Di, Hi, Wi, case.C2) if case.C2 else None,
         "wp": rn(len(case.taps), case.Cout, Cin) / (K_of(case) / nphase(case)) ** 0.5,
         "bias": rn(case.Cout) if case.bias else None, "scale": None, "shift": None, "residual": None, "aux_h": None, "aux_z": None}
    rows = out_desc(case)["out"][0]
    if case.epi == 1 or (case.epi == 3 and case.out2):
        d["scale"], d["shift"] = torch.rand(case.Cout, generator=g) + 0.5, rn(case.Cout)
    if case.residual:
        d["residual"] = rn(case.n * case.D * case.H * case.W if case.lift else rows, case.Cout)
    if case.epi == 2:
        d["aux_h"] = rn(rows, case.Cout // 2)
    if case.epi == 3:
        d["aux_h"], d["aux_z"] = rn(rows, case.Cout), torch.rand(rows, case.Cout, generator=g) * 0.98 + 0.01
    return d


def gather(x, D, H, W, istride, tap):
    """x [n][Di][Hi][Wi][C] -> [n D H W][C]: row of GEMM-grid voxel (z, y, x) is input voxel (z is + dz, y is + dy, x is + dx), zero outside."""
    n, Di, Hi, Wi, C = x.shape
    idx, ok = [], []
    for size, lim, d in ((D, Di, tap[0]), (H, Hi, tap[1]), (W, Wi, tap[2])):
        i = torch.arange(size) * istride + d
        ok.append((i >= 0) & (i < lim))
        idx.append(i.clamp(0, lim - 1))
    g = x[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]]
    m = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
    return torch.where(m[None, :, :, :, None], g, torch.zeros((), dtype=x.dtype)).reshape(n * D * H * W, C)


def out_rows(case, ph):
    """Output row of every GEMM row for phase ph = (pz, py, px): voxel (z os + pz, y os + py, x os + px) of the (n, Do, Ho, Wo) grid."""
    Do, Ho, Wo = case.out_grid
    os_ = case.ostride
    n = torch.arange(case.n)[:, None, None, None]
    z = torch.arange(case.D)[None, :, None, None] * os_ + ph[0]
    y = torch.arange(case.H)[None, None, :, None] * os_ + ph[1]
    x = torch.arange(case.W)[None, None, None, :] * os_ + ph[2]
    assert int(z.max()) < Do and int(y.max()) < Ho and int(x.max()) < Wo
    return (((n * Do + z) * Ho + y) * Wo + x).reshape(-1)


def _accumulate(case, d, taps, wp, dtype, grain, ksplit, mut, want_S):
    """Pre-activation sums without bias [M][Cout] over `taps` (weights wp [len(taps)][Cout][Cin]) and their magnitude sums. grain 'tap': one
    matmul over all input channels per tap, added tap by tap; 'kstep': one per K-step (32 channels, 16 for Cout <= 16) in the order taps outer,
    channels inner, the steps dealt to ksplit slices [ks nsteps / ksplit, (ks + 1) nsteps / ksplit) and the slice sums added in slice order."""
    x1, x2 = d["x1"].to(dtype), (d["x2"].to(dtype) if d["x2"] is not None else None)
    M, Cin, kb = case.n * case.D * case.H * case.W, case.C1 + case.C2, kstep(case)
    kch = Cin // kb
    nsteps = len(taps) * kch
    slices = [torch.zeros(M, case.Cout, dtype=dtype) for _ in range(ksplit)]
    S = torch.zeros(M, case.Cout, dtype=dtype) if want_S else None
    for t, tap in enumerate(taps):
        if mut == "drop_tap" and t == len(taps) // 2:
            continue
        tp = (tap[0], tap[1], -tap[2]) if mut == "mirror_dx" else tap
        X = gather(x1, case.D, case.H, case.W, case.istride, tp)
        if x2 is not None:
            X2 = gather(x2, case.D, case.H, case.W, case.istride, tp)
            X = torch.cat([X, X2.roll(1, dims=1) if mut == "rot_in2" else X2], dim=1)
        w = wp[t].to(dtype)
        if mut == "zero_last_kstep" and t == len(taps) - 1:
            w = w.clone()
            w[:, Cin - kb:] = 0
        if grain == "tap" and ksplit == 1:
            slices[0] += X @ w.t()
        elif grain == "chain":                 # one fused multiply-add per k, in K order (float64 product + sum rounded once = fmaf)
            for k in range(Cin):
                ks = next(q for q in range(ksplit) if t * kch + k // kb < (q + 1) * nsteps // ksplit)
                slices[ks] = (X[:, k, None].double() * w[None, :, k].double() + slices[ks].double()).to(dtype)
        else:
            for kc in range(kch):
                s = t * kch + kc
                ks = next(k for k in range(ksplit) if s < (k + 1) * nsteps // ksplit)
                slices[ks] += X[:, kc * kb:(kc + 1) * kb] @ w[:, kc * kb:(kc + 1) * kb].t()
        if want_S:
            S += X.abs() @ w.abs().t()
    acc = slices[0]
    for s in slices[1:]:
        acc = acc + s
    return acc, S


def gru_tail(epi, v, S, rs, h, z, scale, shift, out2):
    """The GRU epilogues on the pre-activation v [M][Cout] (bias included, residual rs - nullable - not yet): what forge_conv_igemm and forge_wino_output
    both compute. epi 2: g = sigmoid(v + rs); out = g[:, :Ch], out2 = h g[:, Ch:], out3 = g[:, Ch:]. epi 3: cand = tanh(v + rs), out = h (1 - z) + cand z,
    out2 (if asked) = out scale + shift, out3 = cand. S: the magnitude sum of v (None: no sigmas). Returns ({outputs}, {sigma_S}, {sigma_A})."""
    o, oS, oA = {}, {}, {}
    want_S = S is not None
    if rs is not None:
        v = v + rs
    if epi == 2:
        Ch = v.shape[1] // 2
        g = torch.sigmoid(v)
        o["out"], o["out2"], o["out3"] = g[:, :Ch], h * g[:, Ch:], g[:, Ch:]
        if want_S:
            gS, gA = S / 4, (rs.abs() / 4 if rs is not None else 0) + g
            oS["out"], oA["out"] = gS[:, :Ch], gA[:, :Ch]
            oS["out2"], oA["out2"] = h.abs() * gS[:, Ch:], h.abs() * gA[:, Ch:]
            oS["out3"], oA["out3"] = gS[:, Ch:], gA[:, Ch:]
    else:
        cand = torch.tanh(v)
        hn = h * (1 - z) + cand * z
        o["out"], o["out3"] = hn, cand
        if out2:
            o["out2"] = hn * scale + shift
        if want_S:
            cS, cA = S, (rs.abs() if rs is not None else 0) + cand.abs()
            oS["out"], oA["out"] = z.abs() * cS, z.abs() * cA + (h * (1 - z)).abs() + (cand * z).abs()
            oS["out3"], oA["out3"] = cS, cA
            if out2:
                oS["out2"], oA["out2"] = scale.abs() * oS["out"], scale.abs() * oA["out"] + shift.abs()
    return o, oS, oA


def evaluate(case, d, dtype=torch.float64, grain="tap", ksplit=1, mut=None):
    """The contract evaluated in `dtype` on the CPU. Returns {"out" / "out2" / "out3": [rows][width] with NaN in rows the launch does not name,
    "named": bool [rows], "sig_S" / "sig_A": {output: [rows][width]} (float64 evaluation only), "pre": the pre-activations in GEMM-row order}."""
    want_S = dtype == torch.float64 and mut is None
    desc = out_desc(case)
    res = {k: torch.full((r, w), float("nan"), dtype=dtype) for k, (r, w, _) in desc.items()}
    sS = {k: torch.zeros(r, w, dtype=dtype) for k, (r, w, _) in desc.items()} if want_S else None
    sA = {k: torch.zeros(r, w, dtype=dtype) for k, (r, w, _) in desc.items()} if want_S else None
    named = torch.zeros(desc["out"][0], dtype=torch.bool)
    cv = lambda t: None if t is None else t.to(dtype)
    bias, scale, shift, residual, aux_h, aux_z = (cv(d[k]) for k in ("bias", "scale", "shift", "residual", "aux_h", "aux_z"))
    if mut == "no_bias":
        bias = None
    np_ = nphase(case)
    tpp = len(case.taps) // np_
    phases = [(p, ((p >> 2) & 1 if np_ == 8 else 0, (p >> 1) & 1, p & 1)) for p in range(np_)] if np_ > 1 else [(0, tuple(case.phase))]
    pres = []
    for p, ph in phases:
        acc, S = _accumulate(case, d, case.taps[p * tpp:(p + 1) * tpp], d["wp"][p * tpp:(p + 1) * tpp], dtype, grain, ksplit, mut, want_S)
        v = acc + bias if bias is not None else acc
        if want_S and bias is not None:
            S = S + bias.abs()
        pres.append(v)
        M = v.shape[0]
        if case.lift:                         # GEMM column j = z Cl + c of row (n, hw) -> out[n][z][hw][c]
            Cl, HW = case.Cout // case.lift, case.H * case.W
            orow = None
        else:
            orow = out_rows(case, ph)
            named[orow] = True
        rs = None if residual is None else (residual if case.lift else residual[orow])
        zero = torch.zeros((), dtype=dtype)
        o, oS, oA = {}, {}, {}
        if case.epi == 0:
            o["out"], oS["out"], oA["out"] = v, S, zero
        elif case.epi == 1:
            y = v * scale + shift
            L = max(1.0, abs(case.slope))
            if rs is not None and mut != "res_after":
                y = y + rs
            out = torch.where(y > 0, y, y * case.slope)
            if rs is not None and mut == "res_after":
                out = out + rs
            o["out"] = out
            if want_S:
                oS["out"] = L * scale.abs() * S
                oA["out"] = L * (shift.abs() + (rs.abs() if rs is not None else 0)) + torch.zeros_like(S)
        else:
            z = None if aux_z is None else (1 - aux_z[orow] if mut == "swap_z" else aux_z[orow])
            o, oS, oA = gru_tail(case.epi, v, S if want_S else None, rs, aux_h[orow], z, scale, shift, case.out2)
        for k in desc:
            val = o[k]
            if mut == "shift_block" and M > 65:                    # rows 32..63 take the values of rows 33..64
                val = val.clone()
                val[32:64] = o[k][33:65]
            if case.lift:
                n_, Z = case.n, case.lift
                res[k] = val.reshape(n_, HW, Z, Cl).permute(0, 2, 1, 3).reshape(n_ * Z * HW, Cl)
                if want_S:
                    sS[k] = oS[k].reshape(n_, HW, Z, Cl).permute(0, 2, 1, 3).reshape(n_ * Z * HW, Cl)
                    sA[k] = (oA[k] + torch.zeros_like(val)).reshape(n_, HW, Z, Cl).permute(0, 2, 1, 3).reshape(n_ * Z * HW, Cl)
            else:
                res[k][orow] = val
                if want_S:
                    sS[k][orow] = oS[k]
                    sA[k][orow] = oA[k] + torch.zeros_like(val)
    if case.lift:
        named[:] = True
    res.update(named=named, sig_S=sS, sig_A=sA, pre=pres)
    return res


def gamma(case):
    k = (K_of(case) // nphase(case) + 2) * U
    return k / (1 - k)


def unconditional_bound(case, ref, name):
    """Per element: gamma sigma_S + EPI_ULPS 2 u sigma_A (module docstring). Holds for every fp32 evaluation of the contract in any order."""
    return gamma(case) * ref["sig_S"][name] + EPI_ULPS * 2 * U * ref["sig_A"][name]


def q_stats(case, ref, got, name):
    """(q, q_rms, element index of the maximum) of one output against the float64 reference, over every named element - none is excluded."""
    nm = ref["named"]
    e = (got[nm].double() - ref[name][nm]).abs() / (U * (ref["sig_S"][name][nm] + ref["sig_A"][name][nm]))
    assert torch.isfinite(e).all(), (case.name, name, "non-finite error ratio")
    return e.max().item(), e.square().mean().sqrt().item(), int(e.argmax())


def stats_from_outputs(out, M, tile):
    """float64 [stats_blocks(M, tile)][2][Cout]: column sums and sums of squares of `out` [M][Cout] per 32-row block; blocks past M hold zeros.
    Also the absolute sums the comparison scales its 1e-12 bound with."""
    nb, C = stats_blocks(M, tile), out.shape[1]
    o = torch.zeros(nb * 32, C, dtype=torch.float64)
    o[:M] = out.double()
    o = o.reshape(nb, 32, C)
    return torch.stack([o.sum(1), o.square().sum(1)], dim=1), torch.stack([o.abs().sum(1), o.square().sum(1)], dim=1)


def poisoned(x, ld, off, views, poison, guard_rows=3):
    """The logical rows x [n][rows][C] inside a wider, longer, poison-filled float32 buffer: columns [off, off + C) of rows of ld floats, as view
    `ti` of a [n][tv] stack when views = (tv, ti). Returns (flat buffer, element offset of the first fed element, batch stride in rows or 0)."""
    n, rows, C = x.shape
    tv, ti = views if views else (1, 0)
    G = guard_rows * ld
    buf = torch.full((G + n * tv * rows * ld + G,), poison, dtype=torch.float32)
    body = buf[G:G + n * tv * rows * ld].view(n, tv, rows, ld)
    body[:, ti, :, off:off + C] = x
    return buf, G + ti * rows * ld + off, (tv * rows if views else 0)
