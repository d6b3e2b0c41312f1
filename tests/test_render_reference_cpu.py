"""CPU: the float64 restatement of the ray-marcher's contract (tests/render_cases.py) against independent index arithmetic, the oracle and finite
differences; the case table against the dispatch it is meant to reach (instantiations, tile heights, workgroup placement, the voxel gather's three
axis pairs, view-list rounds, the LDS limit); the lattice clearance of every camera-gradient case; the wrong references against the bounds; and the
host-side refusals (nothing is launched) - before tests/test_gpu_render_matrix.py spends a GPU on any of it."""
import pytest
import torch

import forge_oracle as fo
import render_cases as rc
from forge_amd import _lib

NAMES = [c.name for c in rc.CASES]
_REF = {}


def ref(name):
    if name not in _REF:
        c = rc.CASE[name]
        d = rc.make_data(c)
        _REF[name] = (c, d, rc.gradients(c, d))
    return _REF[name]


@pytest.fixture(scope="module")
def L(built_lib):
    return _lib.lib()


def _close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("name", NAMES)
def test_evaluate_vs_index_arithmetic(name):
    """grid_sample + cumprod + autograd against floor / 8 taps / the Q recurrence / index_add: 1e-12 on outputs and volume gradients - and the same
    with the volume gradients passed through the voxel gather's window as its comment states it: the window must let every contribution through."""
    c, d, r = ref(name)
    ex = rc.explicit(c, d, gather=True)
    for k in ("feat", "opac", "depth", "dfeat", "ddens"):
        assert _close(ex[k], r[k]), (name, k)
    if c.nodepth:
        r0, e0 = rc.gradients(c, d, depth=False), rc.explicit(c, d, depth=False)
        assert _close(e0["dfeat"], r0["dfeat"]) and _close(e0["ddens"], r0["ddens"]), name
        assert not _close(r0["ddens"], r["ddens"], 1e-3), (name, "g_depth does not matter here")


def test_evaluate_vs_oracle():
    """forge_oracle.render_rays (cubic grid, isotropic pitch, one volume per view) through evaluate()."""
    g = torch.Generator().manual_seed(3)
    c = rc.mk("oracle", "", 4, (8, 8, 8), (fo.grid_half_extent(8),) * 3, (7, 9), 10, "tilt tilt diag", nvol=3, v2v=(0, 1, 2))
    d = rc.make_data(c)
    cam = d["cam"].double()
    feat, dens = d["feat"].double().permute(0, 4, 1, 2, 3), d["dens"].double()[:, None]
    K = torch.zeros(3, 3, 3, dtype=torch.float64)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cam[:, 12], cam[:, 13], cam[:, 14], cam[:, 15], 1.0
    want = fo.render_rays(feat, dens, cam[:, :9].view(3, 3, 3), cam[:, 9:12], K, c.Hr, c.Wr, c.S, c.zmin, c.zmax, render_depth=True)
    of, oo, od = rc.evaluate(feat, dens, cam, d["v2v"], c.Hr, c.Wr, c.S, c.zmin, c.zmax, c.half)
    assert _close(of.permute(0, 2, 3, 1), want[..., :4]) and _close(oo, want[..., 4]) and _close(od, want[..., 5])
    assert want[..., 4].abs().max().item() > 0.1


def test_gradients_vs_finite_differences():
    """The float64 gradients of a small lattice-clear case against central differences on 36 random entries of each input."""
    c, d, r = ref("r8")
    g = torch.Generator().manual_seed(0)
    feat0, dens0, cam0 = d["feat"].double().permute(0, 4, 1, 2, 3).contiguous(), d["dens"].double()[:, None].contiguous(), d["cam"].double().clone()
    gf, go, gd = d["g_feat"].double().permute(0, 3, 1, 2), d["g_opac"].double(), d["g_depth"].double()

    def loss(f, dn, cm):
        of, oo, od = rc.evaluate(f, dn, cm, d["v2v"], c.Hr, c.Wr, c.S, c.zmin, c.zmax, c.half)
        return ((of * gf).sum() + (oo * go).sum() + (od * gd).sum()).item()
    wants = (r["dfeat"].permute(0, 4, 1, 2, 3).contiguous(), r["ddens"][:, None].contiguous(), r["dcam"])
    for which, (x0, want, h, tol) in enumerate(((feat0, wants[0], 0.5, 1e-9), (dens0, wants[1], 1e-4, 1e-6), (cam0, wants[2], 1e-7, 1e-5))):
        nz = want.reshape(-1).abs().nonzero()[:, 0]
        for idx in nz[torch.randperm(len(nz), generator=g)[:36]].tolist():
            xs = []
            for sgn in (1, -1):
                x = x0.clone()
                x.view(-1)[idx] += sgn * h
                xs.append(loss(*[x if j == which else y for j, y in enumerate((feat0, dens0, cam0))]))
            fd = (xs[0] - xs[1]) / (2 * h)
            assert abs(fd - want.reshape(-1)[idx].item()) <= tol * want.abs().max().item(), (which, idx, fd, want.reshape(-1)[idx].item())


def _dets(cam, z, k):
    """det01, det02, det12 of the plane's pixel-to-voxel map, from the kernel's comment: U = z R_0 / fx k, V = z R_1 / fy k (per axis)."""
    Uv, Vv = z * cam[0:3] / cam[12] * k, z * cam[3:6] / cam[13] * k
    return torch.stack([Uv[0] * Vv[1] - Uv[1] * Vv[0], Uv[0] * Vv[2] - Uv[2] * Vv[0], Uv[1] * Vv[2] - Uv[2] * Vv[1]]).abs()


def _pairs(c, k=None):
    """the set of (view, arg-max pair) over the depth planes of a case"""
    d = rc.make_data(c)
    k = 0.5 * torch.tensor([c.W - 1, c.H - 1, c.D - 1], dtype=torch.float64) / torch.tensor(c.half, dtype=torch.float64) if k is None else k
    return {(v, int(_dets(d["cam"][v].double(), z, k).argmax())) for v in range(len(c.cams)) for z in torch.linspace(c.zmin, c.zmax, c.S, dtype=torch.float64)}


HOLDS = {
    "partial_tiles": lambda c: all(c.Hr % th for th in (4, 8, 16, 32)) and c.Wr % 8 != 0,
    "aniso_pitch": lambda c: max(2 * h / (n - 1) for h, n in zip(c.half, (c.W, c.H, c.D))) >= 2.5 * min(2 * h / (n - 1) for h, n in zip(c.half, (c.W, c.H, c.D)))
    and max(c.half) >= 2.5 * min(c.half),
    "noncubic": lambda c: len({c.D, c.H, c.W}) == 3,
    "det01": lambda c: any(p == 0 for _, p in _pairs(c)), "det02": lambda c: any(p == 1 for _, p in _pairs(c)), "det12": lambda c: any(p == 2 for _, p in _pairs(c)),
    "pitch_decides": lambda c: _pairs(c) != _pairs(c, torch.ones(3, dtype=torch.float64)),
    "beta0": lambda c: bool((rc._positions(rc.make_data(c)["cam"].double(), c.Hr, c.Wr, 2, 0.0, 1.0, torch.float64)[0].diff(dim=3) == 0).any()),
    "views70": lambda c: len(c.cams) == 70 and c.v2v.count(0) == 67 and c.v2v.count(1) == 3 and c.v2v[64] == 0 and (c.Hr, c.Wr, c.S) == (8, 8, 8),
    "unused_volume": lambda c: c.nvol == 3 and 1 not in c.v2v,
    "s2": lambda c: c.S == 2, "s_odd": lambda c: c.S % 2 == 1 and c.S > 2, "s_lds_limit": lambda c: c.S == rc.max_samples(c.C) == 78,
    "miss": lambda c: "miss" in c.cams, "inside": lambda c: "inside" in c.cams and c.zmin <= 0.01,
    "partial_z": lambda c: c.zmin > 1.5 - min(c.half) and c.zmax < 1.5 + min(c.half),
    "ones": lambda c: c.dens == "ones", "over": lambda c: c.dens == "over", "zero": lambda c: c.dens == "zero",
    "intrinsics": lambda c: "tilt" in c.cams, "nodepth": lambda c: c.nodepth,
}
for _C in (4, 8, 16, 32):
    HOLDS["c%d" % _C] = lambda c, C=_C: c.C == C
    HOLDS["cam%d" % _C] = lambda c, C=_C: c.C == C and c.cam
    HOLDS["band%d" % _C] = lambda c, C=_C: c.C == C and rc.band_order(c) and c.Wr == 8 and c.S <= 8 and c.Hr == {4: 256, 8: 128, 16: 64, 32: 32}[C]
    HOLDS["band_partial%d" % _C] = lambda c, C=_C: c.C == C and rc.band_order(c) and c.Wr == 8 and c.Hr == {4: 255, 8: 127, 16: 63, 32: 31}[C]
    HOLDS["launch%d" % _C] = lambda c, C=_C: c.C == C and not rc.band_order(c) and c.Wr == 8 and c.Hr == {4: 257, 8: 129, 16: 65, 32: 33}[C]


def test_coverage_rows():
    """Every row of the coverage table is reached by a case for which it holds, and no case claims a row that does not hold for it."""
    for c in rc.CASES:
        for r in c.rows:
            assert r in rc.ROWS and HOLDS[r](c), (c.name, r)
    for r in rc.ROWS:
        assert any(HOLDS[r](c) and (r in c.rows or r.startswith("cam")) for c in rc.CASES), r
    # what the cases are meant to be
    for c in rc.CASES:
        d = rc.make_data(c)
        ex = rc.explicit(c, d)
        if "tilt" in c.cams:
            cam = d["cam"][c.cams.index("tilt")]
            assert abs(cam[12] - cam[13]) > 0.5 and abs(cam[14] * 2 - round(cam[14].item() * 2)) > 0.005
        if "miss" in c.cams:
            assert not ex["any"][c.cams.index("miss")].any() and ex["any"][1].any()
        if "inside" in c.cams:
            assert ex["any"][:, :, :, 0].double().mean().item() > 0.9                                # the first sample of nearly every ray is inside the grid
        if "partial_z" in c.rows:
            assert ex["any"][..., 0].any() and ex["any"][..., -1].any()
        if c.dens == "ones":
            assert (ex["opac"] > 1 - 1e-12).double().mean().item() > 0.1                             # rays whose transmittance reaches zero before the last sample
            grid = rc._positions(d["cam"], c.Hr, c.Wr, c.S, c.zmin, c.zmax, torch.float32)[0] / torch.tensor(c.half)
            d32 = torch.nn.functional.grid_sample(d["dens"][:, None][d["v2v"].long()], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
            assert (torch.cumprod(1 - d32, -1)[..., :-1] == 0).any(-1).double().mean().item() > 0.1  # and in float32 it is EXACTLY zero there: the forward's break
        if c.dens == "over":
            assert (ex["opac"] > 1).any()
        assert ex["any"].double().mean().item() > 0.1 or "miss" in c.cams
    # the axis cameras take one pair each, and the gather's window on every case drops nothing (test_evaluate_vs_index_arithmetic)
    c = rc.CASE["axes"]
    assert _pairs(c) == {(0, 2), (1, 1), (2, 0)}
    assert {rc.tile_rows(c.C, c.Hr) for c in rc.CASES if any(r.startswith("band") for r in c.rows)} == {8}


@pytest.mark.parametrize("name", [c.name for c in rc.CASES if c.cam])
def test_lattice_clearance(name):
    c, d, _ = ref(name)
    margin, dist = rc.clearance(c, d)
    print("render_clearance %-8s smallest distance to a lattice plane %.3e voxel, margin over 32 u (N + 2) %.3e" % (name, dist, margin))
    assert margin > 0, (name, dist)


def _violates(m, r):
    for k in ("feat", "opac", "depth"):
        if k in m and (m[k] - r[k]).abs().max().item() > rc.fwd_bound(r[k]):
            return True
    for k in ("dfeat", "ddens"):
        if (m[k] - r[k]).abs().max().item() > rc.grad_bound(r[k]):
            return True
    return "dcam" in m and max(rc.group_errors(m["dcam"], r["dcam"])) > rc.DCAM_CAP


@pytest.mark.parametrize("name,muts", rc.MUTATION_CASES)
def test_wrong_references_violate_the_bounds(name, muts):
    c, d, r = ref(name)
    assert not _violates(rc.explicit(c, d, gather=True), r)
    for mut in muts:
        m = rc.gradients(c, d, mut=mut) if mut in rc.AUTOGRAD_MUTATIONS else rc.explicit(c, d, mut=mut)
        assert _violates(m, r), (name, mut, "a wrong reference passes: a case is missing")


def test_every_mutation_has_a_case():
    assert {m for _, ms in rc.MUTATION_CASES for m in ms} == set(rc.MUTATIONS)


def test_refusals_and_workspace(L):
    """Argument checks run before any launch: the pointers are never dereferenced."""
    f = 0x1000
    big = 1 << 40

    def bwd(C, S, ws=f, ws_bytes=big, dcam=None, V=1, Hr=8, Wr=8):
        return L.forge_render_bwd(f, f, f, f, f, f, None, f, f, dcam, V, 1, C, 8, 8, 8, Hr, Wr, S, 0.5, 2.0, 0.5, 0.5, 0.5, ws, ws_bytes, None)
    assert rc.max_samples(4) == 78
    for C in (4, 8, 16, 32):
        S = rc.max_samples(C)
        assert rc.lds_bytes(C, S) <= rc.LDS_LIMIT < rc.lds_bytes(C, S + 1)
        assert bwd(C, S + 1) == -2 and bwd(C, S + 1, dcam=f) == -2, C                       # FORGE_ESHAPE
    for c in rc.CASES:
        V = len(c.cams)
        for want_cam in (0, 1):
            need = rc.ws_bytes(c, want_cam)
            assert L.forge_render_bwd_ws_bytes(V, c.C, c.Hr, c.Wr, c.S, want_cam) == need, (c.name, want_cam)
            kw = dict(dcam=f if want_cam else None, V=V, Hr=c.Hr, Wr=c.Wr)
            assert bwd(c.C, c.S, ws_bytes=need - 1, **kw) == -1, c.name                          # one byte short: FORGE_EINVAL
            assert bwd(c.C, c.S, ws=f + 8, ws_bytes=need + 8, **kw) == -1, c.name                # misaligned
            assert bwd(c.C, c.S, ws=None, ws_bytes=need, **kw) == -1, c.name
    assert L.forge_render_bwd_ws_bytes(1, 12, 8, 8, 8, 0) == -1 and L.forge_render_bwd_ws_bytes(1, 8, 8, 8, 1, 0) == -1
    assert bwd(12, 8) == -2 and bwd(8, 1) == -1
