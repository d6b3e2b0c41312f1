"""The dispatch-space matrix of the direct convolutions (forge_amd/csrc/conv_direct.hip): the contract restated in plain torch, and the case table.

tests/test_gpu_conv_direct_matrix.py launches every case of CASES through the C entry points (forge_conv_direct_fwd / _dgrad / _wgrad / _wgrad_det) into
canary-guarded buffers and measures it against evaluate() / gradients() in float64; tests/test_conv_direct_reference_cpu.py pins those to an independent
restatement by index arithmetic (explicit()), checks that every coverage row is reached and validates the wrong readings (MUTATIONS) with the float32
yardstick standing in for the kernel - before a GPU is spent on them. Both import this module, so the table cannot drift between them.

The contract (the header of conv_direct.hip); rows are channels-last [M][ld], M = n D H W, taps are offsets inside the same (n, D, H, W) grid, zero outside:
    fwd    out[m][co] = lrelu(bias[co] + sum_t sum_ci w[t][co][ci] in[m + tap_t][ci], slope)         (slope 1 = none, 0 = ReLU; bias nullable)
    dgrad  dx[m][ci]  = sum_t sum_co w[t][co][ci] dy[m - tap_t][co]
    wgrad  dw[t][co][ci] += sum_m dy[m][co] x[m + tap_t][ci]              (atomic: onto dw; deterministic: accumulate = 0 stores, 1 adds onto dw)
evaluate() is the forward as shifted-slice sums; gradients() differentiates <linear part, dout> by autograd.

Bounds (u = 2^-24; nothing here is a new constant):
  fwd, dgrad   the form of conv_igemm_cases: per element sigma = L S, S = |bias| + sum |x||w| the magnitude sum, L = max(1, |slope|);
               unconditional |got - ref| <= gamma_K sigma, K = taps x channels summed; sharp q = max |got - ref| / (u sigma) and q_rms within
               SHARP x the same figures of the float32 CPU yardstick: the contract as ONE fused multiply-add per (tap, channel), taps outer - the
               order the kernel documents, and the grain ("chain") test_gpu_conv_igemm_matrix settled on. An element with S = 0 must be exactly zero.
  wgrad        the form of conv_wgrad_cases (its q_stats is used as it stands): unconditional gamma_(M+2) S, sharp q and q_rms within SHARP x the float32
               yardstick, which follows the kernel's documented order: one partial sum per workgroup (256 voxels, grid-stride over wgrad_grid()
               workgroups), the workgroup sums added in order. The atomic entry's run-to-run noise: two runs, and the atomic and the deterministic
               entry, agree within twice the sharp bound. A tap wholly outside the grid leaves an exactly zero dw slice.
"""
import ctypes
from collections import namedtuple

import torch

import conv_igemm_cases as cc
import conv_wgrad_cases as wc
from rotate_cases import GUARD, finish, guarded, yardstick_threads          # noqa: F401  (re-exported to the two tests)

U, SHARP, CANARY = cc.U, cc.SHARP, cc.CANARY
T27, T9, T25, T1, T27_SHUFFLED = cc.T27, cc.T9, cc.T25, cc.T1, cc.T27_SHUFFLED
T64A = [(kz - 2, ky - 2, kx - 2) for kz in range(4) for ky in range(4) for kx in range(4)]      # 64 taps, offsets -2..1 per axis: the tap limit
TDUP = [(0, 0, 0), (0, 1, -1), (0, 0, 0), (1, 0, 1)]                                            # offset (0, 0, 0) twice: two weight slices, one input
TFAR = [(0, 0, -1), (0, 9, 0), (0, 0, 0)]                                                       # dy = 9 on H <= 5: wholly outside, between two live taps
TW3 = [(0, 0, -2), (0, 0, 2), (0, 1, 0), (0, -1, 1), (0, 0, 0), (0, 0, 1)]                      # dx = +-2 on W = 3: one column of three reaches
TAPS = {"T27": T27, "T9": T9, "T25": T25, "T1": T1, "T27S": T27_SHUFFLED, "T64A": T64A, "TDUP": TDUP, "TFAR": TFAR, "TW3": TW3}

PAIRS = [(ci, co) for ci in (4, 8, 16) for co in (1, 2, 3, 4)]
GRID_CAP = 2048                  # workgroups of the weight gradient along x: above it the kernel walks grid-stride
DET_SLAB_BYTES = 64 << 20        # common.h


def wg_taps(ci, co):
    """Taps per workgroup row of the weight-gradient grid (conv_direct.hip: about 48 partial sums per thread, at most 4 taps, at least 1)."""
    q = 48 // (ci * co)
    return 4 if q > 4 else 1 if q < 1 else q


def wgrad_grid(M):
    return min((M + 255) // 256, GRID_CAP)


_FIELDS = "name rows n D H W Cin Cout tapname taps slope bias ldi ldo ops muts note"
Case = namedtuple("Case", _FIELDS)


def mk(name, rows, grid, Cin, Cout, tapname, slope=1.0, bias=True, ldi=None, ldo=None, ops="fwd dgrad wgrad", muts="", note=""):
    """ldi: row stride of the Cin-wide operands (fwd in, dgrad dx, wgrad x); ldo: of the Cout-wide ones (fwd out, dgrad dy, wgrad dy).
    wgrad always means the atomic AND the deterministic entry."""
    n, D, H, W = grid
    return Case(name, frozenset(rows.split()), n, D, H, W, Cin, Cout, tapname, list(TAPS[tapname]), slope, bias, ldi or Cin, ldo or Cout,
                tuple(ops.split()), tuple(muts.split()), note)


# The rows of the coverage table; test_conv_direct_reference_cpu.test_coverage_rows asserts that every one is reached and holds what its name says.
ROWS = (["pair_%d_%d" % p for p in PAIRS] + "m_lt_256 m_two_blocks T27 T9 T25 T1 T27S T64A TDUP TFAR TW3 slope1 slope0 slope001 bias nobias "
        "ld_in ld_in16_c8 ld_out lds_full above_grid_cap".split())

G2, G1, G3 = (2, 4, 5, 7), (2, 3, 5, 7), (1, 4, 5, 6)        # 280 voxels: two workgroups, the second of 24; 210 and 120: one ragged workgroup
P2, P1 = (2, 1, 9, 13), (1, 1, 17, 19)                       # D = 1: 234 and 323 voxels
CASES = [
    mk("c4_1_t27", "pair_4_1 m_two_blocks T27 slope1 bias", G2, 4, 1, "T27", muts="dgrad_pos wrap_w drop_last_group", note="27 taps in groups of 4: the last group holds 3"),
    mk("c4_1_t64", "pair_4_1 m_lt_256 T64A slope0 nobias ld_in ld_out", G3, 4, 1, "T64A", slope=0.0, bias=False, ldi=8, ldo=4,
       muts="dgrad_pos slope_pos drop_last_group", note="the 64-tap limit, 16 full groups"),
    mk("c4_2_t9", "pair_4_2 m_lt_256 T9 slope001 bias", P2, 4, 2, "T9", slope=0.01, muts="w_cico act_before_bias slope_pos wrap_w", note="9 taps in groups of 4: the last holds 1"),
    mk("c4_2_dup", "pair_4_2 m_two_blocks TDUP slope1 nobias ld_out", G2, 4, 2, "TDUP", bias=False, ldo=5, muts="w_cico dgrad_pos", note="one full group; odd ld_out"),
    mk("c4_3_t25", "pair_4_3 T25 slope0 bias", P1, 4, 3, "T25", slope=0.0, muts="act_before_bias w_cico drop_last_group", note="323 voxels; 25 taps in groups of 4"),
    mk("c4_3_w3", "pair_4_3 m_lt_256 TW3 slope1 bias ld_in", (2, 2, 7, 3), 4, 3, "TW3", ldi=12, muts="wrap_w dgrad_pos", note="84 voxels, W = 3; 6 taps in groups of 4"),
    mk("c4_3_dup", "pair_4_3 m_lt_256 TDUP slope001 nobias", G1, 4, 3, "TDUP", slope=0.01, bias=False, muts="slope_pos", note="one full group of 4"),
    mk("c4_4_t64", "pair_4_4 m_lt_256 T64A slope1 bias", G3, 4, 4, "T64A", muts="w_cico drop_last_group", note="64 taps in groups of 3: the last holds 1"),
    mk("c4_4_t27s", "pair_4_4 m_two_blocks T27S slope0 nobias ld_out ld_in", G2, 4, 4, "T27S", slope=0.0, bias=False, ldi=8, ldo=8, muts="dgrad_pos wrap_w slope_pos",
       note="9 full groups of 3, shuffled"),
    mk("c8_1_t27", "pair_8_1 m_two_blocks T27 slope1 nobias ld_in ld_in16_c8 ld_out", G2, 8, 1, "T27", bias=False, ldi=16, ldo=4, muts="dgrad_pos wrap_w drop_last_group",
       note="the density head's Conv3d(8, 1, 3) as the inference callers launch it: slices of wider rows"),
    mk("c8_1_dup", "pair_8_1 m_lt_256 TDUP slope001 bias", G1, 8, 1, "TDUP", slope=0.01, muts="act_before_bias slope_pos", note="one full group of 4"),
    mk("c8_2_t25", "pair_8_2 T25 slope0 bias ld_out", P1, 8, 2, "T25", slope=0.0, ldo=3, muts="w_cico act_before_bias drop_last_group", note="25 taps in groups of 3"),
    mk("c8_2_t9", "pair_8_2 m_lt_256 T9 slope1 bias", P2, 8, 2, "T9", muts="wrap_w", note="3 full groups of 3"),
    mk("c8_3_t25", "pair_8_3 m_lt_256 T25 slope001 bias ld_in ld_in16_c8 ld_out", P2, 8, 3, "T25", slope=0.01, ldi=16, ldo=4,
       muts="w_cico act_before_bias slope_pos wrap_w drop_last_group", note="conv_rgb's Conv2d(8, 3, 5): 25 taps in groups of 2"),
    mk("c8_3_t64", "pair_8_3 m_lt_256 T64A slope1 nobias", G3, 8, 3, "T64A", bias=False, muts="dgrad_pos", note="32 full groups of 2"),
    mk("c8_3_w3", "pair_8_3 m_lt_256 TW3 slope0 bias", (2, 2, 7, 3), 8, 3, "TW3", slope=0.0, muts="wrap_w", note="W = 3; 3 full groups of 2"),
    mk("c8_4_t27", "pair_8_4 m_two_blocks T27 slope1 bias", G2, 8, 4, "T27", muts="w_cico dgrad_pos drop_last_group", note="one tap per group"),
    mk("c8_4_t1", "pair_8_4 m_lt_256 T1 slope0 bias ld_in ld_out", G1, 8, 4, "T1", slope=0.0, ldi=12, ldo=6, muts="w_cico act_before_bias", note="a 1 x 1 x 1 convolution"),
    mk("c16_1_t1", "pair_16_1 m_lt_256 T1 slope001 bias ld_in", G1, 16, 1, "T1", slope=0.01, ldi=20, muts="slope_pos drop_last_group", note="1 tap in a group of 3"),
    mk("c16_1_far", "pair_16_1 m_lt_256 TFAR slope1 bias ld_out", G1, 16, 1, "TFAR", ldo=2, muts="wrap_w dgrad_pos",
       note="one full group of 3; tap (0, 9, 0) lies wholly outside the H = 5 grid: it adds exact zeros and its dw slice is exactly zero"),
    mk("c16_2_t9", "pair_16_2 m_lt_256 T9 slope0 nobias", P2, 16, 2, "T9", slope=0.0, bias=False, muts="w_cico slope_pos"),
    mk("c16_2_w3", "pair_16_2 m_lt_256 TW3 slope1 bias", (2, 2, 7, 3), 16, 2, "TW3", muts="wrap_w w_cico"),
    mk("c16_3_t27s", "pair_16_3 m_two_blocks T27S slope001 bias ld_in ld_out", G2, 16, 3, "T27S", slope=0.01, ldi=24, ldo=7, muts="act_before_bias dgrad_pos drop_last_group"),
    mk("c16_3_dup", "pair_16_3 m_lt_256 TDUP slope1 nobias", G1, 16, 3, "TDUP", bias=False, muts="w_cico dgrad_pos"),
    mk("c16_4_t25", "pair_16_4 T25 slope1 nobias", P1, 16, 4, "T25", bias=False, muts="w_cico wrap_w"),
    mk("c16_4_t64", "pair_16_4 m_lt_256 T64A slope0 bias lds_full", G3, 16, 4, "T64A", slope=0.0, muts="act_before_bias drop_last_group",
       note="64 x 4 x 16 weights: all of the forward kernel's LDS, and the largest slab of the deterministic twin"),
    mk("big", "pair_4_1 T27 above_grid_cap", (2, 66, 64, 64), 4, 1, "T27", ops="wgrad", muts="drop_last_group",
       note="540 672 voxels = 2112 x 256: above the cap of 2048 workgroups, so workgroups 0..63 walk a second block of voxels"),
]
# Measured on the MI355X: the line "conv_direct_matrix <case> ..." that tests/test_gpu_conv_direct_matrix.py prints under -s, as printed. Per entry point
# (wgrad: the atomic entry onto zeros, #2 again, +p onto a prior; det: the deterministic one) q and q_rms, in brackets their ratios to the float32 CPU
# yardstick's (the bound is SHARP = 4), and the ratio to the unconditional bound. The data gradient is 1.00x everywhere: the kernel rounds exactly
# like the yardstick's fmaf chain. The atomic figures of the large case change from run to run.
MEASURED = {
    "c4_1_t27": "M    280 | fwd q 2.21 q_rms 0.540 (0.76x 1.03x) uncond 2.0e-02 | dgrad q 2.13 q_rms 0.452 (1.00x 1.00x) uncond 7.3e-02 | wgrad q 0.62 q_rms 0.170 (0.36x 0.36x) uncond 2.2e-03 | wgrad#2 q 0.62 q_rms 0.170 (0.36x 0.36x) uncond 2.2e-03 | wgrad+p q 0.58 q_rms 0.164 (0.34x 0.35x) uncond 2.0e-03 | det q 0.62 q_rms 0.170 (0.36x 0.36x) uncond 2.2e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_1_t64": "M    120 | fwd q 1.36 q_rms 0.285 (0.98x 0.91x) uncond 5.3e-03 | dgrad q 2.09 q_rms 0.448 (1.00x 1.00x) uncond 3.2e-02 | wgrad q 0.67 q_rms 0.231 (0.31x 0.51x) uncond 5.5e-03 | wgrad#2 q 0.67 q_rms 0.231 (0.31x 0.51x) uncond 5.5e-03 | wgrad+p q 1.17 q_rms 0.221 (0.54x 0.49x) uncond 9.6e-03 | det q 0.67 q_rms 0.231 (0.31x 0.51x) uncond 5.5e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_2_t9": "M    234 | fwd q 1.10 q_rms 0.139 (1.24x 0.96x) uncond 2.9e-02 | dgrad q 2.07 q_rms 0.477 (1.00x 1.00x) uncond 1.0e-01 | wgrad q 0.51 q_rms 0.154 (0.44x 0.44x) uncond 2.2e-03 | wgrad#2 q 0.51 q_rms 0.154 (0.44x 0.44x) uncond 2.2e-03 | wgrad+p q 0.44 q_rms 0.143 (0.38x 0.41x) uncond 1.9e-03 | det q 0.51 q_rms 0.154 (0.44x 0.44x) uncond 2.2e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_2_dup": "M    280 | fwd q 2.38 q_rms 0.427 (1.00x 0.96x) uncond 1.3e-01 | dgrad q 2.01 q_rms 0.403 (1.00x 1.00x) uncond 2.0e-01 | wgrad q 0.34 q_rms 0.161 (0.22x 0.36x) uncond 1.2e-03 | wgrad#2 q 0.34 q_rms 0.161 (0.22x 0.36x) uncond 1.2e-03 | wgrad+p q 0.33 q_rms 0.157 (0.21x 0.35x) uncond 1.2e-03 | det q 0.34 q_rms 0.161 (0.22x 0.36x) uncond 1.2e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_3_t25": "M    323 | fwd q 2.54 q_rms 0.326 (1.15x 1.02x) uncond 2.5e-02 | dgrad q 2.42 q_rms 0.445 (1.00x 1.00x) uncond 3.1e-02 | wgrad q 0.46 q_rms 0.135 (0.32x 0.40x) uncond 1.4e-03 | wgrad#2 q 0.46 q_rms 0.135 (0.32x 0.40x) uncond 1.4e-03 | wgrad+p q 0.60 q_rms 0.134 (0.43x 0.40x) uncond 1.8e-03 | det q 0.46 q_rms 0.135 (0.32x 0.40x) uncond 1.4e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_3_w3": "M     84 | fwd q 3.12 q_rms 0.807 (1.00x 1.01x) uncond 1.2e-01 | dgrad q 1.58 q_rms 0.483 (1.00x 1.00x) uncond 7.9e-02 | wgrad q 0.96 q_rms 0.319 (0.80x 0.71x) uncond 1.1e-02 | wgrad#2 q 0.96 q_rms 0.319 (0.80x 0.71x) uncond 1.1e-02 | wgrad+p q 1.06 q_rms 0.303 (0.89x 0.68x) uncond 1.2e-02 | det q 0.96 q_rms 0.319 (0.80x 0.71x) uncond 1.1e-02 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_3_dup": "M    210 | fwd q 1.69 q_rms 0.294 (0.96x 1.00x) uncond 9.4e-02 | dgrad q 2.75 q_rms 0.427 (1.00x 1.00x) uncond 2.0e-01 | wgrad q 0.41 q_rms 0.144 (0.15x 0.29x) uncond 1.9e-03 | wgrad#2 q 0.41 q_rms 0.144 (0.15x 0.29x) uncond 1.9e-03 | wgrad+p q 0.43 q_rms 0.137 (0.16x 0.28x) uncond 2.0e-03 | det q 0.41 q_rms 0.144 (0.15x 0.29x) uncond 1.9e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_4_t64": "M    120 | fwd q 4.14 q_rms 0.998 (1.05x 0.99x) uncond 1.6e-02 | dgrad q 1.93 q_rms 0.424 (1.00x 1.00x) uncond 7.5e-03 | wgrad q 1.01 q_rms 0.264 (0.42x 0.54x) uncond 8.3e-03 | wgrad#2 q 1.01 q_rms 0.264 (0.42x 0.54x) uncond 8.3e-03 | wgrad+p q 1.12 q_rms 0.253 (0.46x 0.52x) uncond 9.2e-03 | det q 1.01 q_rms 0.264 (0.42x 0.54x) uncond 8.3e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c4_4_t27s": "M    280 | fwd q 2.73 q_rms 0.352 (1.01x 0.98x) uncond 2.5e-02 | dgrad q 2.54 q_rms 0.472 (1.00x 1.00x) uncond 2.3e-02 | wgrad q 0.58 q_rms 0.158 (0.18x 0.34x) uncond 2.1e-03 | wgrad#2 q 0.58 q_rms 0.158 (0.18x 0.34x) uncond 2.1e-03 | wgrad+p q 0.59 q_rms 0.156 (0.18x 0.34x) uncond 2.1e-03 | det q 0.58 q_rms 0.158 (0.18x 0.34x) uncond 2.1e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_1_t27": "M    280 | fwd q 2.39 q_rms 0.488 (1.00x 0.99x) uncond 1.1e-02 | dgrad q 2.94 q_rms 0.466 (1.00x 1.00x) uncond 1.0e-01 | wgrad q 0.64 q_rms 0.146 (0.28x 0.31x) uncond 2.3e-03 | wgrad#2 q 0.64 q_rms 0.146 (0.28x 0.31x) uncond 2.3e-03 | wgrad+p q 0.64 q_rms 0.152 (0.28x 0.32x) uncond 2.3e-03 | det q 0.64 q_rms 0.146 (0.28x 0.31x) uncond 2.3e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_1_dup": "M    210 | fwd q 0.16 q_rms 0.015 (1.00x 0.97x) uncond 4.7e-03 | dgrad q 1.74 q_rms 0.486 (1.00x 1.00x) uncond 2.9e-01 | wgrad q 0.31 q_rms 0.171 (0.19x 0.30x) uncond 1.5e-03 | wgrad#2 q 0.31 q_rms 0.171 (0.19x 0.30x) uncond 1.5e-03 | wgrad+p q 0.40 q_rms 0.178 (0.24x 0.31x) uncond 1.9e-03 | det q 0.31 q_rms 0.171 (0.19x 0.30x) uncond 1.5e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_2_t25": "M    323 | fwd q 2.71 q_rms 0.398 (1.17x 1.06x) uncond 1.3e-02 | dgrad q 3.00 q_rms 0.483 (1.00x 1.00x) uncond 5.8e-02 | wgrad q 0.47 q_rms 0.131 (0.21x 0.30x) uncond 1.4e-03 | wgrad#2 q 0.47 q_rms 0.131 (0.21x 0.30x) uncond 1.4e-03 | wgrad+p q 0.46 q_rms 0.132 (0.21x 0.31x) uncond 1.4e-03 | det q 0.47 q_rms 0.131 (0.21x 0.30x) uncond 1.4e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_2_t9": "M    234 | fwd q 3.57 q_rms 0.791 (1.00x 1.00x) uncond 4.8e-02 | dgrad q 2.46 q_rms 0.482 (1.00x 1.00x) uncond 1.2e-01 | wgrad q 0.47 q_rms 0.151 (0.16x 0.26x) uncond 2.0e-03 | wgrad#2 q 0.47 q_rms 0.151 (0.16x 0.26x) uncond 2.0e-03 | wgrad+p q 0.49 q_rms 0.154 (0.16x 0.27x) uncond 2.1e-03 | det q 0.47 q_rms 0.151 (0.16x 0.26x) uncond 2.0e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_3_t25": "M    234 | fwd q 2.36 q_rms 0.365 (1.08x 1.18x) uncond 1.2e-02 | dgrad q 3.06 q_rms 0.486 (1.00x 1.00x) uncond 4.0e-02 | wgrad q 0.49 q_rms 0.159 (0.22x 0.34x) uncond 2.1e-03 | wgrad#2 q 0.49 q_rms 0.159 (0.22x 0.34x) uncond 2.1e-03 | wgrad+p q 0.64 q_rms 0.158 (0.29x 0.34x) uncond 2.7e-03 | det q 0.49 q_rms 0.159 (0.22x 0.34x) uncond 2.1e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_3_t64": "M    120 | fwd q 2.66 q_rms 0.454 (1.17x 1.00x) uncond 5.2e-03 | dgrad q 2.38 q_rms 0.492 (1.00x 1.00x) uncond 1.2e-02 | wgrad q 1.31 q_rms 0.244 (0.31x 0.55x) uncond 1.1e-02 | wgrad#2 q 1.31 q_rms 0.244 (0.31x 0.55x) uncond 1.1e-02 | wgrad+p q 1.46 q_rms 0.237 (0.35x 0.54x) uncond 1.2e-02 | det q 1.31 q_rms 0.244 (0.31x 0.55x) uncond 1.1e-02 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_3_w3": "M     84 | fwd q 3.51 q_rms 0.762 (0.98x 0.99x) uncond 7.0e-02 | dgrad q 1.99 q_rms 0.473 (1.00x 1.00x) uncond 9.9e-02 | wgrad q 0.69 q_rms 0.264 (0.34x 0.54x) uncond 8.0e-03 | wgrad#2 q 0.69 q_rms 0.264 (0.34x 0.54x) uncond 8.0e-03 | wgrad+p q 0.84 q_rms 0.250 (0.41x 0.51x) uncond 9.7e-03 | det q 0.69 q_rms 0.264 (0.34x 0.54x) uncond 8.0e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_4_t27": "M    280 | fwd q 2.56 q_rms 0.679 (0.97x 0.99x) uncond 1.2e-02 | dgrad q 2.44 q_rms 0.447 (1.00x 1.00x) uncond 2.2e-02 | wgrad q 0.95 q_rms 0.163 (0.32x 0.38x) uncond 3.4e-03 | wgrad#2 q 0.95 q_rms 0.163 (0.32x 0.38x) uncond 3.4e-03 | wgrad+p q 1.02 q_rms 0.162 (0.35x 0.37x) uncond 3.6e-03 | det q 0.95 q_rms 0.163 (0.32x 0.38x) uncond 3.4e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c8_4_t1": "M    210 | fwd q 2.48 q_rms 0.568 (1.08x 1.09x) uncond 2.5e-01 | dgrad q 2.05 q_rms 0.468 (1.00x 1.00x) uncond 3.4e-01 | wgrad q 0.53 q_rms 0.175 (0.37x 0.31x) uncond 2.5e-03 | wgrad#2 q 0.53 q_rms 0.175 (0.37x 0.31x) uncond 2.5e-03 | wgrad+p q 0.52 q_rms 0.181 (0.36x 0.32x) uncond 2.4e-03 | det q 0.53 q_rms 0.175 (0.37x 0.31x) uncond 2.5e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_1_t1": "M    210 | fwd q 1.11 q_rms 0.146 (1.99x 1.28x) uncond 6.2e-02 | dgrad q 0.97 q_rms 0.425 (1.00x 1.00x) uncond 3.2e-01 | wgrad q 0.29 q_rms 0.137 (0.45x 0.45x) uncond 1.4e-03 | wgrad#2 q 0.29 q_rms 0.137 (0.45x 0.45x) uncond 1.4e-03 | wgrad+p q 0.23 q_rms 0.128 (0.36x 0.41x) uncond 1.1e-03 | det q 0.29 q_rms 0.137 (0.45x 0.45x) uncond 1.4e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_1_far": "M    210 | fwd q 1.63 q_rms 0.426 (0.81x 0.96x) uncond 3.3e-02 | dgrad q 1.70 q_rms 0.453 (1.00x 1.00x) uncond 3.4e-01 | wgrad q 0.47 q_rms 0.119 (0.50x 0.37x) uncond 2.2e-03 | wgrad#2 q 0.47 q_rms 0.119 (0.50x 0.37x) uncond 2.2e-03 | wgrad+p q 0.31 q_rms 0.105 (0.34x 0.33x) uncond 1.5e-03 | det q 0.47 q_rms 0.119 (0.50x 0.37x) uncond 2.2e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_2_t9": "M    234 | fwd q 2.31 q_rms 0.341 (1.21x 1.01x) uncond 1.6e-02 | dgrad q 2.87 q_rms 0.441 (1.00x 1.00x) uncond 1.4e-01 | wgrad q 0.49 q_rms 0.160 (0.15x 0.30x) uncond 2.1e-03 | wgrad#2 q 0.49 q_rms 0.160 (0.15x 0.30x) uncond 2.1e-03 | wgrad+p q 0.56 q_rms 0.161 (0.17x 0.30x) uncond 2.4e-03 | det q 0.49 q_rms 0.160 (0.15x 0.30x) uncond 2.1e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_2_w3": "M     84 | fwd q 4.03 q_rms 0.821 (1.42x 1.04x) uncond 4.1e-02 | dgrad q 1.78 q_rms 0.410 (1.00x 1.00x) uncond 1.3e-01 | wgrad q 1.16 q_rms 0.257 (0.69x 0.55x) uncond 1.3e-02 | wgrad#2 q 1.16 q_rms 0.257 (0.69x 0.55x) uncond 1.3e-02 | wgrad+p q 0.83 q_rms 0.244 (0.49x 0.53x) uncond 9.6e-03 | det q 1.16 q_rms 0.257 (0.69x 0.55x) uncond 1.3e-02 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_3_t27s": "M    280 | fwd q 3.15 q_rms 0.441 (0.91x 0.98x) uncond 7.3e-03 | dgrad q 3.50 q_rms 0.466 (1.00x 1.00x) uncond 4.2e-02 | wgrad q 0.74 q_rms 0.156 (0.40x 0.37x) uncond 2.6e-03 | wgrad#2 q 0.74 q_rms 0.156 (0.40x 0.37x) uncond 2.6e-03 | wgrad+p q 0.83 q_rms 0.153 (0.44x 0.36x) uncond 2.9e-03 | det q 0.74 q_rms 0.156 (0.40x 0.37x) uncond 2.6e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_3_dup": "M    210 | fwd q 1.72 q_rms 0.441 (0.71x 1.04x) uncond 2.6e-02 | dgrad q 2.36 q_rms 0.429 (1.00x 1.00x) uncond 1.7e-01 | wgrad q 0.67 q_rms 0.183 (0.32x 0.39x) uncond 3.1e-03 | wgrad#2 q 0.67 q_rms 0.183 (0.32x 0.39x) uncond 3.1e-03 | wgrad+p q 0.74 q_rms 0.188 (0.36x 0.40x) uncond 3.5e-03 | det q 0.67 q_rms 0.183 (0.32x 0.39x) uncond 3.1e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_4_t25": "M    323 | fwd q 3.22 q_rms 0.459 (1.24x 0.98x) uncond 8.0e-03 | dgrad q 4.47 q_rms 0.471 (1.00x 1.00x) uncond 4.4e-02 | wgrad q 0.61 q_rms 0.134 (0.36x 0.45x) uncond 1.9e-03 | wgrad#2 q 0.61 q_rms 0.134 (0.36x 0.45x) uncond 1.9e-03 | wgrad+p q 0.72 q_rms 0.132 (0.43x 0.44x) uncond 2.2e-03 | det q 0.61 q_rms 0.134 (0.36x 0.45x) uncond 1.9e-03 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "c16_4_t64": "M    120 | fwd q 4.04 q_rms 0.636 (1.01x 0.97x) uncond 3.9e-03 | dgrad q 2.64 q_rms 0.464 (1.00x 1.00x) uncond 1.0e-02 | wgrad q 1.60 q_rms 0.254 (0.58x 0.53x) uncond 1.3e-02 | wgrad#2 q 1.60 q_rms 0.254 (0.58x 0.53x) uncond 1.3e-02 | wgrad+p q 1.60 q_rms 0.247 (0.58x 0.51x) uncond 1.3e-02 | det q 1.60 q_rms 0.254 (0.58x 0.53x) uncond 1.3e-02 | atomic vs atomic 0.00 det vs atomic 0.00 of 2x sharp",
    "big": "M 540672 | wgrad q 0.14 q_rms 0.025 (1.50x 0.99x) uncond 2.4e-07 | wgrad#2 q 0.09 q_rms 0.027 (1.02x 1.08x) uncond 1.7e-07 | wgrad+p q 0.13 q_rms 0.029 (1.38x 1.17x) uncond 2.3e-07 | det q 0.01 q_rms 0.003 (0.11x 0.13x) uncond 1.8e-08 | atomic vs atomic 0.13 det vs atomic 0.19 of 2x sharp",
}
CASES = [c._replace(note=(c.note + "; " if c.note else "") + "MI355X: " + MEASURED[c.name]) if c.name in MEASURED else c for c in CASES]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

MUTATIONS = ("dgrad_pos", "wrap_w", "w_cico", "drop_last_group", "act_before_bias", "slope_pos")
MUTATION_CASES = [(c.name, c.muts) for c in CASES if c.muts]


def M_of(c):
    return c.n * c.D * c.H * c.W


def slope64(c):
    """The slope as the entry point receives it: a float."""
    return torch.tensor(c.slope, dtype=torch.float32).double().item()


def make_data(c):
    """Seeded float32 operands in their dense form: x [n][D][H][W][Cin], dout [n][D][H][W][Cout] ~ N(0, 1), w [ntaps][Cout][Cin] ~ N(0, 1 / K), bias,
    prior [ntaps][Cout][Cin] ~ N(0, 1)."""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)))
    rn = lambda *s: torch.randn(*s, generator=g)
    T = len(c.taps)
    return {"x": rn(c.n, c.D, c.H, c.W, c.Cin), "dout": rn(c.n, c.D, c.H, c.W, c.Cout), "w": rn(T, c.Cout, c.Cin) / (T * c.Cin) ** 0.5,
            "bias": rn(c.Cout) if c.bias else None, "prior": rn(T, c.Cout, c.Cin)}


def shifted(x, tap):
    """x [n][D][H][W][C] -> the same shape: voxel (z, y, x) holds voxel (z + dz, y + dy, x + dx), zero outside the grid."""
    out = torch.zeros_like(x)
    sl_o, sl_i = [slice(None)], [slice(None)]
    for size, d in zip(x.shape[1:4], tap):
        lo, hi = max(0, -d), min(size, size - d)
        if lo >= hi:
            return out
        sl_o.append(slice(lo, hi))
        sl_i.append(slice(lo + d, hi + d))
    out[tuple(sl_o)] = x[tuple(sl_i)]
    return out


def linear(x, w, taps):
    """sum_t shifted(x, tap_t) w[t]^T: [n][D][H][W][Cin] -> [n][D][H][W][Cout]."""
    out = 0
    for t, tap in enumerate(taps):
        out = out + shifted(x, tap) @ w[t].t()
    return out


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def evaluate(c, d, dtype=torch.float64):
    """The forward contract: [M][Cout]."""
    pre = linear(d["x"].to(dtype), d["w"].to(dtype), c.taps)
    if d["bias"] is not None:
        pre = pre + d["bias"].to(dtype)
    return lrelu(pre, slope64(c) if dtype == torch.float64 else c.slope).reshape(M_of(c), c.Cout)


def gradients(c, d, dtype=torch.float64):
    """(dx [M][Cin], dw [ntaps][Cout][Cin]) of <linear(x, w), dout> by autograd."""
    x, w = d["x"].to(dtype).clone().requires_grad_(True), d["w"].to(dtype).clone().requires_grad_(True)
    (linear(x, w, c.taps) * d["dout"].to(dtype)).sum().backward()
    return x.grad.reshape(M_of(c), c.Cin), w.grad


def magnitudes(c, d):
    """The magnitude sums of the three results in float64: S_fwd [M][Cout] (times L), S_dx [M][Cin], S_dw [ntaps][Cout][Cin]."""
    x, w, g = d["x"].double().abs(), d["w"].double().abs(), d["dout"].double().abs()
    S = linear(x, w, c.taps)
    if d["bias"] is not None:
        S = S + d["bias"].double().abs()
    neg = [tuple(-v for v in t) for t in c.taps]
    Sdx = linear(g, w.transpose(1, 2), neg)
    M = M_of(c)
    Sdw = torch.stack([g.reshape(M, -1).t() @ shifted(x, t).reshape(M, -1) for t in c.taps])
    return max(1.0, abs(c.slope)) * S.reshape(M, c.Cout), Sdx.reshape(M, c.Cin), Sdw


_REF = {}


def reference(c):
    """Per case, computed once and left unchanged: data, float64 results, magnitude sums."""
    if c.name not in _REF:
        d = make_data(c)
        dx, dw = gradients(c, d)
        Sf, Sdx, Sdw = magnitudes(c, d)
        r = {"d": d, "dx": dx, "dw": dw, "S_fwd": Sf, "S_dx": Sdx, "S_dw": Sdw}
        if "fwd" in c.ops:
            r["fwd"] = evaluate(c, d)
        _REF[c.name] = r
    return _REF[c.name]


# ---- the float32 yardsticks
def _fma(a, b, acc):
    """fl(a b + acc) elementwise in float32: the product of two floats is exact in float64."""
    return (a.double() * b.double() + acc.double()).float()


def yard_fwd(c, d):
    M = M_of(c)
    acc = (d["bias"] if d["bias"] is not None else torch.zeros(c.Cout)).float().expand(M, c.Cout).contiguous()
    for t, tap in enumerate(c.taps):
        xs = shifted(d["x"], tap).reshape(M, c.Cin)
        for ci in range(c.Cin):
            acc = _fma(xs[:, ci, None], d["w"][t, :, ci][None, :], acc)
    return lrelu(acc, torch.tensor(c.slope, dtype=torch.float32))


def yard_dgrad(c, d):
    M = M_of(c)
    acc = torch.zeros(M, c.Cin)
    for t, tap in enumerate(c.taps):
        gs = shifted(d["dout"], tuple(-v for v in tap)).reshape(M, c.Cout)
        for co in range(c.Cout):
            acc = _fma(gs[:, co, None], d["w"][t, co][None, :], acc)
    return acc


def yard_wgrad(c, d):
    """One float32 matmul per workgroup's voxels (workgroup b takes the 256-voxel blocks b, b + G, ...), the workgroup sums added in order."""
    M, G = M_of(c), wgrad_grid(M_of(c))
    nb = (M + 255) // 256
    J = (nb + G - 1) // G
    pad = lambda r: torch.cat([r, r.new_zeros(J * G * 256 - M, r.shape[1])]).view(J, G, 256, -1).permute(1, 0, 2, 3).reshape(G, J * 256, -1)
    dy = pad(d["dout"].reshape(M, c.Cout)).transpose(1, 2)                          # [G][Cout][J 256]
    part = torch.stack([dy @ pad(shifted(d["x"], t).reshape(M, c.Cin)) for t in c.taps], dim=1)      # [G][T][Cout][Cin]
    out = torch.zeros_like(part[0])
    for b in range(G):
        out += part[b]
    return out


def q_elem(got, ref, S):
    """(q, q_rms) of |got - ref| / (u S) over every element; an element with S = 0 must be exactly equal."""
    e = (got.double() - ref).abs()
    zero = S == 0
    assert torch.isfinite(e).all(), "non-finite error"
    assert (e[zero] == 0).all(), ("an element no product reaches is not exact", int((e[zero] != 0).sum()))
    r = torch.where(zero, torch.zeros_like(e), e / (U * S).masked_fill(zero, 1.0))
    return r.max().item(), r.square().mean().sqrt().item()


def gamma(k):
    return (k + 2) * U / (1 - (k + 2) * U)


def K_of(c, op):
    return len(c.taps) * (c.Cin if op == "fwd" else c.Cout)


_YARD = {}


def yardstick(c):
    """{op: (q, q_rms)} of the float32 CPU yardsticks on one thread, computed once per case."""
    if c.name not in _YARD:
        r = reference(c)
        y = {}
        with yardstick_threads():
            if "fwd" in c.ops:
                y["fwd"] = q_elem(yard_fwd(c, r["d"]), r["fwd"], r["S_fwd"])
            if "dgrad" in c.ops:
                y["dgrad"] = q_elem(yard_dgrad(c, r["d"]), r["dx"], r["S_dx"])
            y["wgrad"] = wc.q_stats(c, r["dw"], r["S_dw"], yard_wgrad(c, r["d"]))[:2]
        _YARD[c.name] = y
    return _YARD[c.name]


def violations(c, op, got, ref=None, prior=None):
    """(q, q_rms, ratio to the unconditional bound, [the bounds `got` misses]) for op in fwd / dgrad / wgrad against the float64 reference (or `ref`)."""
    r, (yq, yr) = reference(c), yardstick(c)[op]
    if op == "wgrad":
        q, qr, ub, _ = wc.q_stats(c, r["dw"] if ref is None else ref, r["S_dw"], got, prior)
    else:
        q, qr = q_elem(got, r["fwd" if op == "fwd" else "dx"] if ref is None else ref, r["S_fwd" if op == "fwd" else "S_dx"])
        ub = q * U / gamma(K_of(c, op))
    fails = []
    if ub > 1:
        fails.append("unconditional bound exceeded %.3g times" % ub)
    if q > SHARP * yq or qr > SHARP * yr:
        fails.append("sharp bound: q %.2f (yardstick %.2f) q_rms %.3f (yardstick %.3f)" % (q, yq, qr, yr))
    return q, qr, ub, fails


# ---- the independent restatement: flat index arithmetic, and the wrong readings
def explicit(c, d, mut=None):
    """{"fwd" [M][Cout], "dx" [M][Cin], "dw" [ntaps][Cout][Cin]} in float64 by coordinates, bound tests and flat row indices - no slices, no autograd.
    mut: one of MUTATIONS - a deliberately WRONG reading."""
    assert mut is None or mut in MUTATIONS
    M, T = M_of(c), len(c.taps)
    x, g, w = d["x"].double().reshape(M, c.Cin), d["dout"].double().reshape(M, c.Cout), d["w"].double()
    if mut == "w_cico":
        w = w.reshape(-1).view(T, c.Cin, c.Cout).transpose(1, 2)
    e = torch.arange(M)
    X, Y, Z = e % c.W, (e // c.W) % c.H, (e // (c.W * c.H)) % c.D

    def rows(tap, sign):
        dz, dy, dx = (sign * v for v in tap)
        flat = e + (dz * c.H + dy) * c.W + dx
        ok = (Z + dz >= 0) & (Z + dz < c.D) & (Y + dy >= 0) & (Y + dy < c.H)
        ok = ok & ((flat >= 0) & (flat < M) if mut == "wrap_w" else (X + dx >= 0) & (X + dx < c.W))
        return flat.clamp(0, M - 1), ok.double()[:, None]

    pre, dxo, dw = torch.zeros(M, c.Cout, dtype=torch.float64), torch.zeros(M, c.Cin, dtype=torch.float64), torch.zeros(T, c.Cout, c.Cin, dtype=torch.float64)
    tg = wg_taps(c.Cin, c.Cout)
    for t, tap in enumerate(c.taps):
        src, ok = rows(tap, 1)
        xs = x[src] * ok
        for co in range(c.Cout):
            pre[:, co] += (xs * w[t, co][None, :]).sum(1)
            if not (mut == "drop_last_group" and t >= (T - 1) // tg * tg):
                dw[t, co] = (g[:, co, None] * xs).sum(0)
        src, ok = rows(tap, 1 if mut == "dgrad_pos" else -1)
        gs = g[src] * ok
        for co in range(c.Cout):
            dxo += gs[:, co, None] * w[t, co][None, :]
    b = d["bias"].double() if d["bias"] is not None else torch.zeros(c.Cout, dtype=torch.float64)
    s = slope64(c)
    if mut == "act_before_bias":
        out = lrelu(pre, s) + b
    elif mut == "slope_pos":
        out = torch.where(pre + b > 0, (pre + b) * s, pre + b)
    else:
        out = lrelu(pre + b, s)
    return {"fwd": out, "dx": dxo, "dw": dw}


# ---- what the entry points refuse before launching anything: (what, changed arguments, error code)
REFUSALS = [
    ("Cin 12", dict(Cin=12, ldi=12), -2), ("Cout 5", dict(Cout=5, ldo=5), -2),
    ("ld_in % 4 != 0", dict(ldi=10), -2), ("ld_in < Cin", dict(ldi=4), -2), ("ld_out < Cout", dict(ldo=2), -2),
    ("ntaps 0", dict(ntaps=0), -1), ("ntaps 65", dict(ntaps=65), -1), ("a tap component of 128", dict(tap128=True), -1),
    ("a NULL operand", dict(null=True), -1),
]
REFUSAL_BASE = dict(Cin=8, Cout=3, ldi=8, ldo=3, ntaps=9, n=1, D=1, H=4, W=5)


def refusal_calls(L, ptrs, ws_ok=1 << 20):
    """Every refusal of REFUSALS on each entry point it applies to, and the deterministic entry's own: [(what, rc, wanted code)].
    ptrs = (in, w, bias, out, x, ws): never dereferenced by a call that is refused."""
    pin, pw, pb, pout, px, pws = ptrs
    res = []
    for what, kw, code in REFUSALS:
        a = dict(REFUSAL_BASE, **{k: v for k, v in kw.items() if k in REFUSAL_BASE})
        nt = a["ntaps"]
        taps = [(0, 0, i % 3 - 1) for i in range(max(nt, 1))]
        if kw.get("tap128"):
            taps[-1] = (0, 128, 0)
        ta = (ctypes.c_int * (3 * len(taps)))(*[v for t in taps for v in t])
        dims = (a["n"], a["D"], a["H"], a["W"], a["Cin"], a["Cout"], ta, nt)
        null = kw.get("null")
        res.append((what + " (fwd)", L.forge_conv_direct_fwd(pin, a["ldi"], None if null else pw, pb, 0.0, pout, a["ldo"], *dims, None), code))
        res.append((what + " (dgrad)", L.forge_conv_direct_dgrad(pin, a["ldo"], pw, None if null else px, a["ldi"], *dims, None), code))
        res.append((what + " (wgrad)", L.forge_conv_direct_wgrad(pin, a["ldo"], None if null else px, a["ldi"], pout, *dims, None), code))
        res.append((what + " (wgrad det)", L.forge_conv_direct_wgrad_det(pin, a["ldo"], px, a["ldi"], None if null else pout, *dims, 0, pws, ws_ok, None), code))
    a = REFUSAL_BASE
    ta = (ctypes.c_int * 27)(*[v for t in T9 for v in t])
    dims = (a["n"], a["D"], a["H"], a["W"], a["Cin"], a["Cout"], ta, 9)
    need = L.forge_conv_direct_wgrad_det_ws_bytes(*dims[:6], 9)
    det = lambda acc, ws, nbytes: L.forge_conv_direct_wgrad_det(pin, a["ldo"], px, a["ldi"], pout, *dims, acc, ws, nbytes, None)
    res.append(("workspace one byte short", det(0, pws, need - 1), -1))
    res.append(("workspace misaligned", det(0, ctypes.c_void_p(pws.value + 4), need + 4), -1))
    res.append(("workspace NULL", det(0, None, need), -1))
    res.append(("accumulate = 2", det(2, pws, need), -1))
    return res


# ---- device buffers with row gaps
def guarded_rows(x, ld, dev):
    """An input [M][C] as columns [0, C) of rows of ld floats; gap columns and guard rows are NaN. Returns the view whose pointer the kernel gets."""
    buf, start, _ = cc.poisoned(x[None], ld, 0, None, float("nan"))
    return buf.to(dev)[start:]


def finish_rows(raw, body, width, what):
    """finish() for an output [M][ld] of which columns [0, width) are named: every other float of the allocation still holds the pattern."""
    torch.cuda.synchronize()
    host = raw.cpu()
    M, ld = body.shape
    named = torch.zeros(host.numel(), dtype=torch.bool)
    named[GUARD:GUARD + M * ld].view(M, ld)[:, :width] = True
    assert (host[~named] == CANARY).all(), (what, "an element the contract does not name was written", int((host[~named] != CANARY).sum()))
    got = host[GUARD:GUARD + M * ld].view(torch.float32).view(M, ld)[:, :width].clone()
    assert torch.isfinite(got).all(), (what, "an element was not written (or is not finite)", int((~torch.isfinite(got)).sum()))
    return got
