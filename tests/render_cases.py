"""The dispatch-space matrix of the ray-marcher (forge_amd/csrc/render.hip): the contract restated in plain torch, and the case table.

tests/test_gpu_render_matrix.py launches every case of CASES through forge_render_fwd / forge_render_bwd and measures it against evaluate() in float64;
tests/test_render_reference_cpu.py pins evaluate() to independent index arithmetic (explicit()), to the oracle and to finite differences, checks
that every coverage row is reached, that the voxel gather takes each of its three axis pairs, that every camera-gradient case clears the lattice,
and validates the wrong references (MUTATIONS) before a GPU is spent on them. Both import this module, so the table cannot drift between them.

The contract (models/volume_render.py:53-63 of the reference): pinhole rays of the packed camera [R9 | T3 | fx fy cx cy] with half-pixel centres,
o = -R^T T, dir = R^T ((w + .5 - cx) / fx, (h + .5 - cy) / fy, 1); samples at camera depths z = linspace(zmin, zmax, S); the volumes sampled at
p / (hx, hy, hz) by grid_sample(trilinear, zeros, align_corners=True); emission-absorption compositing w_s = d_s prod_{j<s} (1 - d_j): features
sum w f, opacity 1 - prod (1 - d), depth sum w z. evaluate() is that sentence in torch with independent hx, hy, hz and D != H != W; gradients()
differentiates <feat, g_feat> + <opac, g_opac> + <depth, g_depth> by autograd for the volumes and the cameras. explicit() is the same contract by
floor / 8-tap index arithmetic with the Q recurrence written out by hand; it carries the wrong readings of the backward (MUTATIONS).

Bounds (the ones the project already states for this kernel; u = 2^-24):
  forward        2e-5 max(1, |ref|_max) on features, opacity and depth
  dfeat, ddens   5e-5 of the gradient's maximum
  dcam           per camera-entry group (R, T, f, c; over all views), relative to that group's maximum: SHARP x the float32 CPU evaluation of evaluate()
                 (the yardstick), at least 64 u, never more than 2e-3. Compared on cases that clear the lattice only (clearance()).
  exact          a frustum that misses the volume, an all-zero density, a volume no view reads: zeros.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_igemm_cases as cc

U = cc.U
SHARP = cc.SHARP
CANARY = cc.CANARY
DCAM_CAP = 2e-3
DCAM_FLOOR = 64 * U
GROUPS = (("R", 0, 9), ("T", 9, 12), ("f", 12, 14), ("c", 14, 16))
LDS_LIMIT = 160 * 1024 - 2048

_FIELDS = "name rows C D H W half Hr Wr S zmin zmax nvol v2v cams dens seed cam nodepth muts note"
Case = namedtuple("Case", _FIELDS)

GRID_A, HALF_A = (6, 10, 14), (0.2, 0.35, 0.5)        # (D, H, W), (hx, hy, hz): pitches 0.031, 0.078, 0.2 - anisotropic 6.5 : 1
GRID_B, HALF_B = (12, 7, 5), (0.5, 0.3, 0.2)          # pitches 0.25, 0.1, 0.036
GRID_8, HALF_8 = (8, 8, 8), (0.45, 0.45, 0.45)


def mk(name, rows, C, grid, half, img, S, cams, z=(0.7, 2.3), nvol=1, v2v=None, dens="rand", seed=0, cam=True, nodepth=False, muts="", note=""):
    """cams: one camera kind per view (KINDS). v2v: the volume of each view (default 0). dens: the density volume's kind (make_data). cam: the camera
    gradient is compared (the case must then clear the lattice: test_render_reference_cpu asserts it). nodepth: the case also runs the backward
    with g_depth == NULL."""
    cams = tuple(cams.split()) if isinstance(cams, str) else tuple(cams)
    return Case(name, frozenset(rows.split()), C, grid[0], grid[1], grid[2], tuple(half), img[0], img[1], S, z[0], z[1], nvol,
                tuple(v2v) if v2v else (0,) * len(cams), cams, dens, seed, cam, nodepth, tuple(muts.split()), note)


KINDS = ("tilt", "diag", "ax", "ay", "az", "miss", "inside")

# The rows of the coverage table; test_render_reference_cpu.test_coverage_rows asserts that every one is reached and holds what its name says.
# Every case runs the forward with and without depth, the backward without dcam and the backward with dcam.
ROWS = ("c4 c8 c16 c32 partial_tiles aniso_pitch noncubic det01 det02 det12 pitch_decides beta0 views70 unused_volume "
        "band4 band8 band16 band32 band_partial4 band_partial8 band_partial16 band_partial32 launch4 launch8 launch16 launch32 s2 s_odd s_lds_limit miss inside partial_z ones over zero intrinsics nodepth "
        "cam4 cam8 cam16 cam32").split()

V70 = tuple(1 if i in (10, 33, 66) else 0 for i in range(70))
CASES = [
    # ---- the instantiations, on anisotropic non-cubic grids and images whose last tile row and column are partial for every tile height
    mk("r4", "c4 partial_tiles aniso_pitch noncubic intrinsics nodepth", 4, GRID_A, HALF_A, (17, 10), 16, "tilt tilt", nodepth=True, muts="swap_h small_w",
       note="C4 = 1: no shuffle round, an 8 x 32 tile: one partial tile row", seed=1),
    mk("r8", "c8 partial_tiles aniso_pitch noncubic pitch_decides intrinsics", 8, GRID_B, HALF_B, (9, 13), 16, "tilt diag", muts="ac_false fx_both drop_pixel",
       note="8 x 16 tiles; the camera along (1, 1, 1) sees all three pairs equally: the pitch picks the pair"),
    mk("r16", "c16 partial_tiles aniso_pitch noncubic intrinsics nodepth", 16, GRID_A, HALF_A, (9, 13), 16, "tilt tilt tilt", nvol=2, v2v=(0, 1, 0), nodepth=True,
       muts="swap_h", note="8 x 8 tiles, two volumes"),
    mk("r32", "c32 partial_tiles aniso_pitch noncubic intrinsics", 32, GRID_B, HALF_B, (17, 10), 16, "tilt tilt", muts="fx_both small_w", note="8 x 4 tiles: five tile rows"),
    # ---- the gather's three axis pairs, and rays with a direction component of exactly zero
    mk("axes", "c8 det01 det02 det12 beta0 aniso_pitch", 8, GRID_A, HALF_A, (9, 13), 16, "ax ay az", cam=False, muts="drop_pixel swap_h",
       note="cameras along world x, y, z with the principal point on a pixel centre: its row and column of rays have a zero direction component, "
            "and their samples sit on lattice planes (no dcam comparison)"),
    mk("axes16", "c16 det01 det02 det12 beta0 noncubic", 16, GRID_B, HALF_B, (9, 13), 12, "az ay ax", cam=False, note="the same on the other grid"),
    # ---- view lists, unused volumes
    mk("v70", "views70 c8", 8, GRID_8, HALF_8, (8, 8), 8, ("tilt",) * 70, nvol=2, v2v=V70, muts="skip_view",
       note="67 views of volume 0 interleaved with 3 of volume 1: a second round of the 64-entry view list, partially filled"),
    mk("unused", "unused_volume c16", 16, GRID_8, HALF_8, (9, 13), 8, "tilt tilt tilt", nvol=3, v2v=(0, 2, 0), note="no view reads volume 1: its gradients are written as zeros"),
    # ---- workgroup placement: 8 tile rows deal evenly to the 8 XCDs (band order); one image row fewer is still 8 tile rows, the last a partial one;
    #      one image row more is 9 tile rows: launch order
    mk("b4", "band4 c4", 4, GRID_8, HALF_8, (256, 8), 8, "tilt tilt", note="8 tile rows of 32", seed=4),
    mk("b4n", "band_partial4 c4", 4, GRID_8, HALF_8, (255, 8), 8, "tilt tilt", seed=4),
    mk("b4p", "launch4 c4", 4, GRID_8, HALF_8, (257, 8), 8, "tilt tilt", seed=7),
    mk("b8", "band8 c8", 8, GRID_8, HALF_8, (128, 8), 8, "tilt tilt", note="8 tile rows of 16"),
    mk("b8n", "band_partial8 c8", 8, GRID_8, HALF_8, (127, 8), 8, "tilt tilt"),
    mk("b8p", "launch8 c8", 8, GRID_8, HALF_8, (129, 8), 8, "tilt tilt"),
    mk("b16", "band16 c16", 16, GRID_8, HALF_8, (64, 8), 7, "tilt tilt", note="8 tile rows of 8", seed=1),
    mk("b16n", "band_partial16 c16", 16, GRID_8, HALF_8, (63, 8), 7, "tilt tilt"),
    mk("b16p", "launch16 c16", 16, GRID_8, HALF_8, (65, 8), 7, "tilt tilt"),
    mk("b32", "band32 c32", 32, GRID_8, HALF_8, (32, 8), 6, "tilt tilt", note="8 tile rows of 4"),
    mk("b32n", "band_partial32 c32", 32, GRID_8, HALF_8, (31, 8), 6, "tilt tilt"),
    mk("b32p", "launch32 c32", 32, GRID_8, HALF_8, (33, 8), 6, "tilt tilt"),
    # ---- samples
    mk("s2", "s2 c8 nodepth", 8, GRID_A, HALF_A, (9, 13), 2, "tilt tilt", z=(1.35, 1.65), nodepth=True, muts="last_plane", note="both planes inside the volume", seed=1),
    mk("s7", "s_odd c16 partial_z", 16, GRID_B, HALF_B, (9, 13), 7, "tilt tilt", z=(1.35, 1.65), muts="last_plane",
       note="S odd: the middle sample is the first of sample_depth's upper half; the volume starts before zmin and ends past zmax"),
    mk("s78", "s_lds_limit c4", 4, GRID_8, HALF_8, (8, 8), 78, "tilt", note="2 x 256 x 79 x 4 B = 161792 B of LDS: the most C = 4 takes"),
    # ---- intervals
    mk("miss", "miss c16", 16, GRID_8, HALF_8, (9, 13), 8, "miss tilt", nvol=2, v2v=(0, 1), note="view 0 looks away from its volume: exact zeros in its outputs, in dcam and in volume 0's gradients"),
    mk("inside", "inside c8", 8, GRID_A, HALF_A, (9, 13), 12, "inside inside", z=(0.01, 0.8), note="cameras inside the grid, zmin near 0", seed=1),
    # ---- densities
    mk("ones", "ones c16", 16, GRID_8, HALF_8, (9, 13), 12, "tilt tilt", dens="ones", muts="stop_t0",
       note="densities exactly 1: the forward stops at T == 0, the backward's Q recurrence must not"),
    mk("over", "over c8", 8, GRID_8, HALF_8, (9, 13), 12, "tilt tilt", dens="over", note="densities up to 1.6: negative transmittance", seed=1),
    mk("zero", "zero c4", 4, GRID_8, HALF_8, (9, 13), 12, "tilt tilt", dens="zero", note="all-zero density: zero outputs and dfeat, ddens = T (a - Q) with T = 1"),
]
# Measured on the MI355X, per case (forward: worst of features / opacity / depth over max(1, |ref|); dfeat, ddens: of the maximum; dcam: R T f c groups). A ratio is the worst group's error over the float32 CPU yardstick's (at least 64 u / SHARP); the bound is SHARP = 4.
MEASURED = {
    "r4": "fwd 1.7e-06 dfeat 3.9e-06 ddens 3.3e-06 dcam [5.6e-06 1.9e-06 2.3e-06 2.0e-06] of yardstick [4.2e-06 1.2e-06 6.6e-06 1.3e-06]: 1.64x",
    "r8": "fwd 2.7e-06 dfeat 4.1e-06 ddens 6.7e-06 dcam [3.9e-06 2.8e-06 3.0e-06 1.5e-06] of yardstick [3.3e-06 1.6e-06 2.9e-06 2.4e-06]: 1.76x",
    "r16": "fwd 3.2e-06 dfeat 4.7e-06 ddens 7.2e-06 dcam [3.2e-06 1.2e-06 5.0e-06 9.4e-07] of yardstick [4.3e-06 3.1e-06 2.2e-06 3.2e-06]: 2.24x",
    "r32": "fwd 3.4e-06 dfeat 3.7e-06 ddens 5.2e-06 dcam [2.5e-06 3.3e-07 1.9e-06 3.2e-07] of yardstick [5.2e-06 5.1e-07 2.1e-06 3.4e-07]: 0.88x",
    "axes": "fwd 2.3e-06 dfeat 3.3e-06 ddens 5.4e-06 dcam not compared",
    "axes16": "fwd 1.4e-06 dfeat 1.4e-06 ddens 3.5e-06 dcam not compared",
    "v70": "fwd 1.2e-06 dfeat 1.6e-06 ddens 1.0e-06 dcam [1.1e-06 1.0e-06 9.6e-07 8.3e-07] of yardstick [1.1e-06 1.5e-06 1.2e-06 1.4e-06]: 0.95x",
    "unused": "fwd 1.2e-06 dfeat 2.2e-06 ddens 1.3e-06 dcam [7.4e-07 9.4e-07 1.2e-06 1.3e-06] of yardstick [9.3e-07 1.5e-06 1.4e-06 1.8e-06]: 0.86x",
    "b4": "fwd 1.4e-06 dfeat 1.7e-06 ddens 1.3e-06 dcam [1.9e-06 1.1e-06 1.7e-06 1.7e-06] of yardstick [2.4e-06 1.1e-06 1.5e-06 1.3e-06]: 1.26x",
    "b4n": "fwd 1.2e-06 dfeat 1.4e-06 ddens 1.8e-06 dcam [1.3e-06 1.5e-06 6.2e-07 1.7e-06] of yardstick [1.8e-06 1.8e-06 7.4e-07 1.3e-06]: 1.23x",
    "b4p": "fwd 9.4e-07 dfeat 1.1e-06 ddens 1.6e-06 dcam [8.0e-07 5.3e-07 1.0e-06 2.2e-07] of yardstick [5.5e-06 1.3e-06 1.4e-06 5.9e-07]: 0.76x",
    "b8": "fwd 1.2e-06 dfeat 8.2e-07 ddens 1.9e-06 dcam [8.9e-07 6.4e-07 1.5e-06 5.8e-07] of yardstick [2.1e-06 7.8e-07 2.3e-06 7.7e-07]: 0.68x",
    "b8n": "fwd 1.0e-06 dfeat 1.4e-06 ddens 2.4e-06 dcam [9.2e-07 1.0e-06 8.2e-07 8.0e-07] of yardstick [4.8e-06 5.5e-07 8.8e-07 4.6e-07]: 1.08x",
    "b8p": "fwd 1.1e-06 dfeat 7.0e-07 ddens 2.5e-06 dcam [6.5e-07 1.1e-06 8.8e-07 1.4e-06] of yardstick [1.9e-06 1.2e-06 1.3e-06 1.7e-06]: 0.90x",
    "b16": "fwd 1.0e-06 dfeat 1.1e-06 ddens 1.3e-06 dcam [1.5e-06 1.8e-06 8.5e-07 7.8e-07] of yardstick [2.3e-06 1.7e-06 1.2e-06 2.0e-06]: 1.01x",
    "b16n": "fwd 1.2e-06 dfeat 1.5e-06 ddens 2.5e-06 dcam [7.8e-07 1.0e-06 1.1e-06 5.8e-07] of yardstick [1.1e-06 9.1e-07 1.1e-06 2.6e-07]: 1.08x",
    "b16p": "fwd 1.4e-06 dfeat 1.0e-06 ddens 1.4e-06 dcam [2.1e-06 5.6e-07 9.6e-06 9.0e-07] of yardstick [3.9e-06 1.5e-06 1.4e-05 9.0e-07]: 0.95x",
    "b32": "fwd 1.6e-06 dfeat 1.1e-06 ddens 2.2e-06 dcam [1.4e-06 1.3e-06 8.3e-07 8.0e-07] of yardstick [1.6e-06 1.5e-06 2.2e-06 1.2e-06]: 0.88x",
    "b32n": "fwd 1.3e-06 dfeat 2.0e-06 ddens 1.9e-06 dcam [6.2e-07 1.6e-06 1.0e-06 5.5e-07] of yardstick [1.6e-06 1.5e-06 6.3e-07 1.4e-07]: 1.07x",
    "b32p": "fwd 1.4e-06 dfeat 1.4e-06 ddens 1.1e-06 dcam [9.7e-07 9.8e-07 4.5e-06 1.5e-06] of yardstick [1.5e-06 1.1e-06 6.8e-06 3.0e-06]: 0.86x",
    "s2": "fwd 2.2e-06 dfeat 3.3e-06 ddens 3.3e-06 dcam [3.4e-06 4.1e-06 2.0e-06 4.1e-06] of yardstick [3.2e-06 3.0e-06 2.8e-06 1.6e-06]: 2.63x",
    "s7": "fwd 1.8e-06 dfeat 2.1e-06 ddens 1.2e-06 dcam [3.1e-06 8.5e-07 1.8e-06 2.4e-07] of yardstick [1.9e-06 2.3e-06 6.2e-07 1.5e-06]: 1.91x",
    "s78": "fwd 8.7e-07 dfeat 5.8e-07 ddens 8.0e-07 dcam [7.4e-07 7.4e-07 5.0e-07 3.4e-07] of yardstick [5.9e-07 8.3e-07 6.2e-07 1.1e-06]: 0.78x",
    "miss": "fwd 1.2e-06 dfeat 2.3e-06 ddens 1.4e-06 dcam [6.7e-07 1.2e-06 3.9e-07 1.9e-06] of yardstick [1.2e-06 2.2e-06 4.0e-07 3.8e-06]: 0.54x",
    "inside": "fwd 5.7e-07 dfeat 4.1e-07 ddens 8.3e-07 dcam [1.1e-06 1.0e-06 1.1e-06 1.2e-06] of yardstick [8.1e-07 7.6e-07 1.4e-06 9.6e-07]: 1.29x",
    "ones": "fwd 1.4e-06 dfeat 1.5e-06 ddens 1.7e-06 dcam [5.0e-07 5.6e-07 4.0e-07 5.5e-07] of yardstick [1.1e-06 1.1e-06 6.5e-07 1.1e-06]: 0.50x",
    "over": "fwd 1.2e-06 dfeat 1.1e-06 ddens 9.8e-07 dcam [1.4e-06 7.2e-07 1.8e-06 8.8e-07] of yardstick [3.6e-06 2.0e-06 1.4e-06 1.9e-06]: 1.27x",
    "zero": "fwd 0.0e+00 dfeat 0.0e+00 ddens 1.6e-06 dcam [0.0e+00 0.0e+00 0.0e+00 0.0e+00] of yardstick [0.0e+00 0.0e+00 0.0e+00 0.0e+00]: 0.00x",
}
CASES = [c._replace(note=(c.note + "; " if c.note else "") + "MI355X: " + MEASURED[c.name]) for c in CASES]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

MUTATIONS = ("drop_pixel", "small_w", "last_plane", "swap_h", "ac_false", "stop_t0", "skip_view", "fx_both")
AUTOGRAD_MUTATIONS = ("swap_h", "ac_false", "fx_both")       # wrong readings of the geometry: through evaluate(); the others through explicit()
MUTATION_CASES = [(c.name, c.muts) for c in CASES if c.muts]


def tile_rows(C, Hr):
    TH = (256 // (C // 4)) // 8
    return (Hr + TH - 1) // TH


def band_order(c):
    return tile_rows(c.C, c.Hr) % 8 == 0


def lds_bytes(C, S):
    return 2 * (256 // (C // 4)) * (S + 1) * 4


def max_samples(C):
    """the largest S the backward takes at C channels"""
    return LDS_LIMIT // (2 * (256 // (C // 4)) * 4) - 1


def ws_bytes(c, want_cam):
    """forge_render_bwd's workspace, from the comment above render_bwd_ws_layout: G [V][S][Hr][Wr] float2, then with camera gradients 16 floats per
    workgroup (rounded up to 16 bytes) and six floats per sample."""
    V, TH = len(c.cams), (256 // (c.C // 4)) // 8
    g = V * c.Hr * c.Wr * c.S * 8
    if not want_cam:
        return g
    nblk = ((c.Wr + 7) // 8) * ((c.Hr + TH - 1) // TH)
    return g + (V * nblk * 64 + 15) // 16 * 16 + V * c.Hr * c.Wr * c.S * 24


def _unit(v):
    return v / v.norm()


def camera(kind, g, c):
    """One packed camera (float64; make_data rounds it to float32). g: the case's generator."""
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)
    dist = 1.5
    if kind in ("ax", "ay", "az", "miss"):
        a = {"ax": 0, "ay": 1, "az": 2, "miss": 0}[kind]
        e = torch.eye(3, dtype=torch.float64)
        eye, zc, xc = dist * e[a], (e[a] if kind == "miss" else -e[a]), e[(a + 1) % 3]
        Rm = torch.stack([xc, torch.linalg.cross(zc, xc), zc])
        K = f64(1.1 * c.Wr, 1.3 * c.Hr, c.Wr // 2 + 0.5, c.Hr // 2 + 0.5)               # the principal point on a pixel centre
    else:
        if kind == "inside":
            eye, target = (r(3) - 0.5) * 0.1, _unit(r(3) - 0.5)
        elif kind == "diag":
            eye, target = dist * _unit(f64(1.0, 1.0, 1.0) + 0.02 * (r(3) - 0.5)), torch.zeros(3, dtype=torch.float64)
        else:
            eye, target = dist * _unit((r(3) - 0.5) + 0.25 * torch.sign(r(3) - 0.5)), (r(3) - 0.5) * 0.1
        zc = _unit(target - eye)
        up = f64(0.0, 0.0, 1.0) if abs(zc[2]) < 0.9 else f64(0.0, 1.0, 0.0)
        xc = _unit(torch.linalg.cross(up, zc))
        yc = torch.linalg.cross(zc, xc)
        roll = (r(1).item() - 0.5) * 1.2
        xc, yc = math.cos(roll) * xc + math.sin(roll) * yc, -math.sin(roll) * xc + math.cos(roll) * yc
        Rm = torch.stack([xc, yc, zc])
        foc = 0.55 if kind == "inside" else 1.1
        K = f64(foc * c.Wr * (1 + 0.1 * r(1).item()), 0.9 * foc * c.Hr * (1 + 0.1 * r(1).item()), c.Wr / 2 + (r(1).item() - 0.5) * 1.7 + 0.013,
                c.Hr / 2 + (r(1).item() - 0.5) * 1.7 + 0.017)                              # fx != fy, the principal point off-centre by a non-integer
    return torch.cat([Rm.reshape(9), -(Rm @ eye), K])


def make_data(c):
    """Seeded float32 operands in the kernels' layout: feat [nvol][D][H][W][C] ~ N(0, 1), dens [nvol][D][H][W], cam [V][16], v2v [V] int32,
    upstream gradients g_feat [V][Hr][Wr][C], g_opac, g_depth [V][Hr][Wr]."""
    g = torch.Generator().manual_seed(1000 * c.seed + sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)))
    V = len(c.cams)
    cam = torch.stack([camera(k, g, c) for k in c.cams]).float()
    rn = lambda *s: torch.randn(*s, generator=g)
    u = torch.rand(c.nvol, c.D, c.H, c.W, generator=g)
    dens = {"rand": 0.35 * u, "ones": torch.ones_like(u), "over": 1.6 * u, "zero": torch.zeros_like(u)}[c.dens]
    return {"feat": rn(c.nvol, c.D, c.H, c.W, c.C), "dens": dens, "cam": cam, "v2v": torch.tensor(c.v2v, dtype=torch.int32),
            "g_feat": rn(V, c.Hr, c.Wr, c.C), "g_opac": rn(V, c.Hr, c.Wr), "g_depth": rn(V, c.Hr, c.Wr)}


def _positions(cam, Hr, Wr, S, zmin, zmax, dtype, fx_both=False):
    """World positions [V][Hr][Wr][S][3] of every sample, and z [S]."""
    V = cam.shape[0]
    Rm, T = cam[:, :9].view(V, 3, 3), cam[:, 9:12]
    fx, fy, cx, cy = cam[:, 12], (cam[:, 12] if fx_both else cam[:, 13]), cam[:, 14], cam[:, 15]
    ws, hs = torch.arange(Wr, dtype=dtype) + 0.5, torch.arange(Hr, dtype=dtype) + 0.5
    dxc = ((ws[None, :] - cx[:, None]) / fx[:, None])[:, None, :].expand(V, Hr, Wr)
    dyc = ((hs[None, :] - cy[:, None]) / fy[:, None])[:, :, None].expand(V, Hr, Wr)
    dc = torch.stack([dxc, dyc, torch.ones_like(dxc)], dim=-1)
    dw = torch.einsum("vji,vhwj->vhwi", Rm, dc)                                            # R^T d
    o = -torch.einsum("vji,vj->vi", Rm, T)
    z = torch.linspace(zmin, zmax, S, dtype=dtype)
    return o[:, None, None, None, :] + dw[:, :, :, None, :] * z[None, None, None, :, None], z


def evaluate(feat, dens, cam16, view2vol, Hr, Wr, S, zmin, zmax, half, dtype=torch.float64, mut=None):
    """The contract in plain torch. feat [nvol][C][D][H][W], dens [nvol][1][D][H][W], cam16 [V][16], view2vol [V] ->
    (features [V][C][Hr][Wr], opacity [V][Hr][Wr], depth [V][Hr][Wr]) in `dtype`. mut: one of AUTOGRAD_MUTATIONS - a deliberately WRONG reading."""
    assert mut is None or mut in AUTOGRAD_MUTATIONS
    feat, dens, cam = feat.to(dtype), dens.to(dtype), cam16.to(dtype)
    pts, z = _positions(cam, Hr, Wr, S, zmin, zmax, dtype, fx_both=mut == "fx_both")
    hh = torch.tensor([half[1], half[0], half[2]] if mut == "swap_h" else list(half), dtype=dtype)
    grid = pts / hh                                                                        # [V][Hr][Wr][S][3]: an output "volume" of Hr x Wr x S points
    idx = torch.as_tensor(view2vol).long()
    ac = mut != "ac_false"
    d = F.grid_sample(dens[idx], grid, mode="bilinear", padding_mode="zeros", align_corners=ac)[:, 0]          # [V][Hr][Wr][S]
    f = F.grid_sample(feat[idx], grid, mode="bilinear", padding_mode="zeros", align_corners=ac)                # [V][C][Hr][Wr][S]
    cp = torch.cumprod(1.0 - d, dim=-1)
    trans = torch.cat([torch.ones_like(cp[..., :1]), cp[..., :-1]], dim=-1)
    w = d * trans
    return (w[:, None] * f).sum(-1), 1.0 - torch.prod(1.0 - d, dim=-1), (w * z).sum(-1)


def gradients(c, d, dtype=torch.float64, depth=True, mut=None):
    """Forward and gradients of <feat, g_feat> + <opac, g_opac> (+ <depth, g_depth>) through evaluate(), in the kernels' layouts:
    {"feat" [V][Hr][Wr][C], "opac", "depth" [V][Hr][Wr], "dfeat" [nvol][D][H][W][C], "ddens" [nvol][D][H][W], "dcam" [V][16]}."""
    feat = d["feat"].to(dtype).permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    dens = d["dens"].to(dtype)[:, None].clone().requires_grad_(True)
    cam = d["cam"].to(dtype).clone().requires_grad_(True)
    of, oo, od = evaluate(feat, dens, cam, d["v2v"], c.Hr, c.Wr, c.S, c.zmin, c.zmax, c.half, dtype, mut)
    loss = (of * d["g_feat"].to(dtype).permute(0, 3, 1, 2)).sum() + (oo * d["g_opac"].to(dtype)).sum()
    if depth:
        loss = loss + (od * d["g_depth"].to(dtype)).sum()
    loss.backward()
    return {"feat": of.detach().permute(0, 2, 3, 1).contiguous(), "opac": oo.detach(), "depth": od.detach(),
            "dfeat": feat.grad.permute(0, 2, 3, 4, 1).contiguous(), "ddens": dens.grad[:, 0].contiguous(), "dcam": cam.grad}


def voxel_coords(c, d):
    """float64 voxel coordinates [V][Hr][Wr][S][3] (x, y, z) of every sample: ((p / h + 1) / 2) (N - 1), and z [S]."""
    pts, z = _positions(d["cam"].double(), c.Hr, c.Wr, c.S, c.zmin, c.zmax, torch.float64)
    N1 = torch.tensor([c.W - 1, c.H - 1, c.D - 1], dtype=torch.float64)
    return (pts / torch.tensor(c.half, dtype=torch.float64) + 1.0) * 0.5 * N1, z


def window(c, d, v, s, px, py, q, mut=None):
    """The voxel gather's window, restated from its comment in float64: whether voxel q [M][3] looks at sample s [M] of pixel (px, py) [M] of view v [M]
    - the depth planes with |z_s - z_q| < sum_a |R_2a| pitch_a, and on the plane the pixel rectangle of the 2x2 solve on the best-conditioned pair of
    axes. Returns (keep [M], pair [M]: 0 = det01, 1 = det02, 2 = det12, the determinants [M][3])."""
    f8 = torch.float64
    cam = d["cam"].double()[v]
    hh, N1 = torch.tensor(c.half, dtype=f8), torch.tensor([c.W - 1, c.H - 1, c.D - 1], dtype=f8)
    step = (c.zmax - c.zmin) / (c.S - 1)
    qf = q.double()
    world, pitch, k = (2.0 * qf / N1 - 1.0) * hh, 2.0 * hh / N1, 0.5 * N1 / hh
    zq = (cam[:, 6:9] * world).sum(1) + cam[:, 11]
    dzq = (cam[:, 6:9].abs() * pitch).sum(1) * 1.001 + 1e-6
    fs_lo, fs_hi = (zq - dzq - c.zmin) / step, (zq + dzq - c.zmin) / step
    s_lo, s_hi = (fs_lo - 0.02).ceil().clamp_min(0), (fs_hi + 0.02).floor().clamp_max(c.S - 1)
    if mut == "last_plane":
        s_hi = s_hi.clamp_max(c.S - 2)
    keep = (fs_hi >= -0.02) & (fs_lo <= c.S - 1 + 0.02) & (s >= s_lo) & (s <= s_hi)
    z = torch.linspace(c.zmin, c.zmax, c.S, dtype=f8)[s]
    Rm = cam[:, :9].view(-1, 3, 3)
    d00 = torch.stack([(0.5 - cam[:, 14]) / cam[:, 12], (0.5 - cam[:, 15]) / cam[:, 13], torch.ones_like(z)], dim=1)
    dir00, o = torch.einsum("mji,mj->mi", Rm, d00), -torch.einsum("mji,mj->mi", Rm, cam[:, 9:12])
    E0 = (dir00 * z[:, None] + o) * k + 0.5 * N1 - qf
    Uv, Vv = z[:, None] * Rm[:, 0] / cam[:, 12:13] * k, z[:, None] * Rm[:, 1] / cam[:, 13:14] * k
    dets = torch.stack([Uv[:, 0] * Vv[:, 1] - Uv[:, 1] * Vv[:, 0], Uv[:, 0] * Vv[:, 2] - Uv[:, 2] * Vv[:, 0], Uv[:, 1] * Vv[:, 2] - Uv[:, 2] * Vv[:, 1]], dim=1)
    pair = torch.zeros_like(s)
    pair[dets[:, 1].abs() > dets[:, 0].abs()] = 1
    best = torch.where(pair == 1, dets[:, 1], dets[:, 0])
    pair[dets[:, 2].abs() > best.abs()] = 2
    ia, ib = torch.tensor([0, 0, 1])[pair], torch.tensor([1, 2, 2])[pair]
    pick = lambda t, i: t.gather(1, i[:, None])[:, 0]
    Ua, Va, ra, Ub, Vb, rb, det = pick(Uv, ia), pick(Vv, ia), -pick(E0, ia), pick(Uv, ib), pick(Vv, ib), -pick(E0, ib), pick(dets, pair)
    cxp, cyp = (Vb * ra - Va * rb) / det, (Ua * rb - Ub * ra) / det
    ex, ey = (Vb.abs() + Va.abs()) / det.abs() + 0.05, (Ub.abs() + Ua.abs()) / det.abs() + 0.05
    x0, x1 = (cxp - ex).ceil().clamp_min(0), (cxp + ex).floor().clamp_max(c.Wr - 1)
    y0, y1 = (cyp - ey).ceil().clamp_min(0), (cyp + ey).floor().clamp_max(c.Hr - 1)
    solved = det.abs() > 1e-12
    keep = keep & (~solved | ((px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)))
    aff = E0 + px.double()[:, None] * Uv + py.double()[:, None] * Vv
    keep = keep & (aff.abs() < 1.001).all(1)
    if mut == "drop_pixel":
        keep = keep & ~(solved & (px == x1) & (py == y1))
    return keep, pair, dets


def explicit(c, d, mut=None, depth=True, gather=False):
    """The contract by floor / 8-tap index arithmetic in float64, the backward by the recurrence dL/dd_s = T_s (a_s - Q_s), Q_{s-1} = a_s d_s +
    (1 - d_s) Q_s, Q_{S-1} = -g_opacity, a_s = <g, f_s> + g_depth z_s, scattered to the taps: {"feat", "opac", "depth", "dfeat", "ddens", "pos"
    [V][Hr][Wr][S][3], "any" [V][Hr][Wr][S], "pairs": how often the gather's window takes each axis pair}. gather: the volume gradients only
    receive what the voxel gather's window (window()) lets through - it must let everything through. mut: a deliberately WRONG reading."""
    assert mut is None or (mut in MUTATIONS and mut not in AUTOGRAD_MUTATIONS)
    f8 = torch.float64
    V, Hr, Wr, S, C = len(c.cams), c.Hr, c.Wr, c.S, c.C
    M = c.D * c.H * c.W
    p, z = voxel_coords(c, d)
    Nl = torch.tensor([c.W, c.H, c.D])
    feat, dens = d["feat"].double().reshape(c.nvol * M, C), d["dens"].double().reshape(c.nvol * M)
    base = (d["v2v"].long() * M)[:, None, None, None]
    i0 = p.floor().long()
    fr = p - i0.double()
    ds, fs, anyok, taps = torch.zeros(V, Hr, Wr, S, dtype=f8), torch.zeros(V, Hr, Wr, S, C, dtype=f8), torch.zeros(V, Hr, Wr, S, dtype=torch.bool), []
    for k in range(8):
        dd = torch.tensor([k & 1, (k >> 1) & 1, k >> 2])
        ii = i0 + dd
        ok = ((ii >= 0) & (ii < Nl)).all(-1)
        anyok |= ok
        w = torch.where(dd.bool(), fr, 1.0 - fr).prod(-1) * ok
        iic = torch.minimum(ii.clamp_min(0), Nl - 1)
        flat = base + (iic[..., 2] * c.H + iic[..., 1]) * c.W + iic[..., 0]
        ds += w * dens[flat]
        fs += w[..., None] * feat[flat]
        taps.append((w, flat, iic))
    g_feat, g_opac = d["g_feat"].double(), d["g_opac"].double()
    g_dep = d["g_depth"].double() if depth else torch.zeros(V, Hr, Wr, dtype=f8)
    T = torch.ones(V, Hr, Wr, dtype=f8)
    Ts, of, od = [], torch.zeros(V, Hr, Wr, C, dtype=f8), torch.zeros(V, Hr, Wr, dtype=f8)
    for s in range(S):
        Ts.append(T)
        wgt = ds[..., s] * T
        of, od, T = of + wgt[..., None] * fs[..., s, :], od + wgt * z[s], T * (1.0 - ds[..., s])
    Ts = torch.stack(Ts, dim=-1)
    a = (fs * g_feat[:, :, :, None, :]).sum(-1) + g_dep[..., None] * z
    db, ab = ds, a
    if mut == "stop_t0":                                     # the backward stops where the forward does: the tail's (d, a) never enter Q
        live = torch.cat([torch.ones_like(Ts[..., :1]), (Ts[..., 1:].abs() > 1e-9).double()], dim=-1)
        db, ab = ds * live, a * live
    Q, X = -g_opac, torch.zeros(V, Hr, Wr, S, dtype=f8)
    for s in range(S - 1, -1, -1):
        X[..., s] = ab[..., s] - Q
        Q = ab[..., s] * db[..., s] + (1.0 - db[..., s]) * Q
    dLdd, wg = Ts * X, Ts * ds
    dfeat, ddens = torch.zeros(c.nvol * M, C, dtype=f8), torch.zeros(c.nvol * M, dtype=f8)
    vi, hi, wi, si = torch.meshgrid(torch.arange(V), torch.arange(Hr), torch.arange(Wr), torch.arange(S), indexing="ij")
    pairs = torch.zeros(3, dtype=torch.long)
    skip = None
    if mut == "skip_view":                                   # the 65th view of the fullest volume: the first of the view list's second round
        vol = max(set(c.v2v), key=c.v2v.count)
        skip = [i for i, n in enumerate(c.v2v) if n == vol][64]
    for w, flat, iic in taps:
        wk = w
        if mut == "small_w":
            wk = wk * (w >= 1e-3)
        if gather or mut in ("drop_pixel", "last_plane"):
            keep, pair, _ = window(c, d, vi.reshape(-1), si.reshape(-1), wi.reshape(-1), hi.reshape(-1), iic.reshape(-1, 3), mut)
            wk = wk * keep.view(V, Hr, Wr, S)
            pairs += torch.bincount(pair[(w.reshape(-1) > 0)], minlength=3)
        if skip is not None:
            wk = wk * (vi != skip)
        ddens.index_add_(0, flat.reshape(-1), (wk * dLdd).reshape(-1))
        dfeat.index_add_(0, flat.reshape(-1), ((wk * wg)[..., None] * g_feat[:, :, :, None, :]).reshape(-1, C))
    return {"feat": of, "opac": 1.0 - T, "depth": od, "dfeat": dfeat.view(c.nvol, c.D, c.H, c.W, C), "ddens": ddens.view(c.nvol, c.D, c.H, c.W),
            "pos": p, "any": anyok, "pairs": pairs}


def clearance(c, d):
    """(smallest margin, smallest distance): over every sample with an in-range tap and every axis a, the distance of its float64 voxel coordinate to
    the nearest integer, less 32 u (N_a + 2) - the position chain is about 8 fp32 roundings of a value of at most N_a + 2; this is 4x that."""
    p, _ = voxel_coords(c, d)
    Nl = torch.tensor([c.W, c.H, c.D], dtype=torch.float64)
    anyok = ((p > -1) & (p < Nl)).all(-1)
    if not anyok.any():
        return float("inf"), float("inf")
    dd = (p[anyok] - p[anyok].round()).abs()
    return (dd - 32 * U * (Nl + 2)).min().item(), dd.min().item()


def certainly_outside(c, d):
    """[V][S][Hr][Wr] bool: samples that lie at least two sample steps outside the stretch of their ray that can have a tap (voxel coordinates in
    (-1.001, N + 0.001) on all three axes), rays that miss the volume altogether included: the ray-parallel pass must leave exact zeros there."""
    p, z = voxel_coords(c, d)
    Nl = torch.tensor([c.W, c.H, c.D], dtype=torch.float64)
    lo, hi = torch.full(p.shape[:3], -float("inf"), dtype=torch.float64), torch.full(p.shape[:3], float("inf"), dtype=torch.float64)
    beta = (p[:, :, :, -1] - p[:, :, :, 0]) / (c.zmax - c.zmin)                              # voxel coordinates are affine in z
    alpha = p[:, :, :, 0] - beta * c.zmin
    never = torch.zeros(p.shape[:3], dtype=torch.bool)
    for a in range(3):
        al, be = alpha[..., a], beta[..., a]
        flat = be.abs() < 1e-9
        never |= flat & ~((al > -1.01) & (al < Nl[a] + 0.01))
        bs = torch.where(flat, torch.ones_like(be), be)
        t1, t2 = (-1.01 - al) / bs, (Nl[a] + 0.01 - al) / bs
        lo = torch.where(flat, lo, torch.maximum(lo, torch.minimum(t1, t2)))
        hi = torch.where(flat, hi, torch.minimum(hi, torch.maximum(t1, t2)))
    never |= lo > hi
    step = (c.zmax - c.zmin) / (c.S - 1)
    zs = z[None, None, None, :]
    out = never[..., None] | (zs < lo[..., None] - 3 * step) | (zs > hi[..., None] + 3 * step)
    return out.permute(0, 3, 1, 2).contiguous()


def fwd_bound(ref):
    return 2e-5 * max(1.0, ref.abs().max().item())


def grad_bound(ref):
    return 5e-5 * ref.abs().max().item()


def group_errors(got, ref):
    """Per camera-entry group (R, T, f, c): max |got - ref| over the group's entries of all views, relative to the group's maximum of |ref| (a group that
    is all zero in the reference must be exactly zero)."""
    out = []
    for _, a, b in GROUPS:
        e, m = (got.double() - ref)[:, a:b].abs().max().item(), ref[:, a:b].abs().max().item()
        if m == 0:
            assert e == 0, "a camera-entry group of zeros in the reference is not exactly zero"
        out.append(e / m if m else 0.0)
    return out


def dcam_bounds(yard):
    return [min(DCAM_CAP, max(DCAM_FLOOR, SHARP * y)) for y in yard]
