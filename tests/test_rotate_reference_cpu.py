"""CPU: the float64 restatement of the pose warp's contract (tests/rotate_cases.py) against independent index arithmetic, the oracle and finite
differences; the case table against the dispatch it is meant to reach; the lattice clearance of every derivative case; the wrong references against
the bounds; and the host-side refusals (nothing is launched) - before tests/test_gpu_rotate_matrix.py spends a GPU on any of it."""
import pytest
import torch

import forge_oracle as fo
import rotate_cases as rc
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
    """grid_sample + autograd against floor / 8 taps / index_add and a hand-written adjoint: 1e-12. The affine gradient is compared where the case clears
    the lattice (on a lattice plane the one-sided derivative depends on which side the last bit of the position falls)."""
    c, d, (out, dvox, dxf) = ref(name)
    ex = rc.explicit(c, d)
    assert _close(ex["out"], out) and _close(ex["dvox"], dvox), name
    if c.dxf:
        assert _close(ex["dxf"], dxf), name
    assert (dxf[d["mode"] == 0] == 0).all()
    boxed = rc.explicit(c, d, box=True)
    assert _close(boxed["dvox"], ex["dvox"], 1e-14), (name, "the gather's candidate box, as its comment states it, loses a contribution")


def test_evaluate_vs_oracle():
    """forge_oracle.rotate_world (cubic grids, camera poses) through evaluate(): xf = [T_A | T_t / e], T = P_0 P_i^-1."""
    g = torch.Generator().manual_seed(5)
    B, t, C, D = 1, 3, 4, 8
    poses = torch.eye(4, dtype=torch.float64).repeat(B, t, 1, 1)
    for i in range(t):
        poses[0, i, :3, :3] = rc._rot((torch.rand(3, generator=g) - 0.5).tolist(), 0.4 * i + 0.1)
        poses[0, i, :3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.3
    vox = torch.randn(B, t, C, D, D, D, generator=g, dtype=torch.float64)
    want = fo.rotate_world(vox, poses)
    T = poses[0, 0:1] @ torch.inverse(poses[0])
    xf = torch.cat([T[:, :3, :3], T[:, :3, 3:4] / fo.grid_half_extent(D)], dim=-1).reshape(t, 12)
    got = rc.evaluate(vox[0], xf, torch.tensor([0, 1, 1]))
    assert _close(got, want[0])


def test_gradients_vs_finite_differences():
    """The float64 gradients of the smallest multi-transform case against central differences on 36 random entries of each input."""
    c, d, (_, dvox, dxf) = ref("p8")
    g = torch.Generator().manual_seed(0)
    dout = d["dout"].double().permute(0, 4, 1, 2, 3)
    vox0, xf0 = d["vox"].double().permute(0, 4, 1, 2, 3).contiguous(), d["xf"].double().clone()
    loss = lambda v, x: (rc.evaluate(v, x, d["mode"], d["slot"]) * dout).sum().item()
    dv = dvox.permute(0, 4, 1, 2, 3).contiguous()
    for idx in torch.randint(0, vox0.numel(), (36,), generator=g).tolist():
        v1, v2 = vox0.clone(), vox0.clone()
        v1.view(-1)[idx] += 0.5
        v2.view(-1)[idx] -= 0.5
        assert abs((loss(v1, xf0) - loss(v2, xf0)) - dv.view(-1)[idx].item()) <= 1e-9 * dv.abs().max().item()          # linear in vox: exact
    warped = [i * 12 + j for i in range(len(c.views)) if d["mode"][i] for j in range(12)]
    h = 1e-7
    for idx in [warped[k] for k in torch.randperm(len(warped), generator=g)[:36].tolist()]:
        x1, x2 = xf0.clone(), xf0.clone()
        x1.view(-1)[idx] += h
        x2.view(-1)[idx] -= h
        fd = (loss(vox0, x1) - loss(vox0, x2)) / (2 * h)
        assert abs(fd - dxf.view(-1)[idx].item()) <= 1e-5 * dxf.abs().max().item(), (idx, fd, dxf.view(-1)[idx].item())


HOLDS = {
    "plain_small": lambda c: not rc.tile_order(c) and max(c.D, c.H, c.W) <= 14,
    "plain_one_side": lambda c: sum(n % 16 != 0 for n in (c.D, c.H, c.W)) == 1,
    "tile_cubic": lambda c: rc.tile_order(c) and c.D == c.H == c.W,
    "tile_noncubic": lambda c: rc.tile_order(c) and len({c.D, c.H, c.W}) == 3,
    "tile_nq4": lambda c: rc.tile_order(c) and rc.nq_gather(c.C) == 4,
    "fwd_nq1": lambda c: rc.nq_forward(c.C) == 1, "fwd_nq2": lambda c: rc.nq_forward(c.C) == 2,
    "gather_nq1": lambda c: rc.nq_gather(c.C) == 1, "gather_nq2": lambda c: rc.nq_gather(c.C) == 2, "gather_nq4": lambda c: rc.nq_gather(c.C) == 4,
    "c8": lambda c: (c.C, rc.nq_forward(c.C), rc.nq_gather(c.C)) == (8, 1, 1), "c64": lambda c: (c.C, rc.nq_forward(c.C), rc.nq_gather(c.C)) == (64, 2, 2),
    "c72": lambda c: (c.C, rc.nq_forward(c.C), rc.nq_gather(c.C)) == (72, 2, 2), "c128": lambda c: (c.C, rc.nq_forward(c.C), rc.nq_gather(c.C)) == (128, 2, 4),
    "c136": lambda c: (c.C, rc.nq_forward(c.C), rc.nq_gather(c.C)) == (136, 2, 2) and c.D * c.H * c.W <= 840,
    "mode_mix": lambda c: "copy" in c.views and len(set(c.views)) > 1,
    "slots": lambda c: c.slot is not None and sorted(c.slot) == list(range(len(c.views))) and list(c.slot) != list(range(len(c.views))),
    "slots_not_involution": lambda c: c.slot is not None and any(c.slot[c.slot[i]] != i for i in range(len(c.slot))),
    "dxf_plain": lambda c: c.dxf and not rc.tile_order(c), "dxf_tile": lambda c: c.dxf and rc.tile_order(c),
    "dxf_nq1": lambda c: c.dxf and rc.nq_gather(c.C) == 1, "dxf_nq2": lambda c: c.dxf and rc.nq_gather(c.C) == 2, "dxf_nq4": lambda c: c.dxf and rc.nq_gather(c.C) == 4,
}
HOLDS.update({k: (lambda c, k=k: k in c.views) for k in rc.KINDS if k != "copy"})


def test_coverage_rows():
    """Every row of the coverage table is reached by a case for which it holds, and no case claims a row that does not hold for it."""
    for c in rc.CASES:
        for r in c.rows:
            assert r in rc.ROWS and HOLDS[r](c), (c.name, r)
    for r in rc.ROWS:
        assert any(HOLDS[r](c) and (r in c.rows or r.startswith(("dxf_", "fwd_nq", "gather_nq"))) for c in rc.CASES), r
    assert {rc.nq_forward(c.C) for c in rc.CASES} == {1, 2} and {rc.nq_gather(c.C) for c in rc.CASES} == {1, 2, 4}
    # what the transforms are meant to be
    for c in rc.CASES:
        d = rc.make_data(c)
        A = d["xf"].double().view(-1, 3, 4)
        for i, k in enumerate(c.views):
            det = torch.linalg.det(A[i, :, :3]).item()
            if k == "reflect":
                assert det < -0.5
            if k == "s055":
                assert 0.1 < det < 0.2
            if k == "s19":
                assert det > 6
            if k in ("quarter", "quarter_lattice"):
                assert (A[i, :, 3] == 0).all()
    # the lattice case: every sample of the scaled quarter turn sits within 1e-5 of a lattice point; thrown out: no sample has a tap; clipped: about half
    c = rc.CASE["quarter"]
    p, _ = rc.explicit(c, rc.make_data(c))["pos"][1]
    assert (p - p.round()).abs().max().item() < 1e-5
    c = rc.CASE["edge"]
    pos = rc.explicit(c, rc.make_data(c))["pos"]
    assert not pos[0][1].any() and 0.3 < pos[1][1].double().mean().item() < 0.7


@pytest.mark.parametrize("name", [c.name for c in rc.CASES if c.dxf])
def test_lattice_clearance(name):
    c, d, _ = ref(name)
    margin, dist = rc.clearance(c, d)
    print("rotate_clearance %-8s smallest distance to a lattice plane %.3e voxel, margin over 32 u (N + 2) %.3e" % (name, dist, margin))
    assert margin > 0, (name, dist)


def _violates(c, d, m, want):
    out, dvox, dxf = want
    if (m["out"] - out).abs().max().item() > rc.fwd_bound(c, out) or (m["dvox"] - dvox).abs().max().item() > rc.dvox_bound(c, dvox):
        return True
    return max(rc.row_errors(m["dxf"], dxf)) > rc.DXF_CAP


@pytest.mark.parametrize("name,muts", rc.MUTATION_CASES)
def test_wrong_references_violate_the_bounds(name, muts):
    c, d, want = ref(name)
    assert not _violates(c, d, rc.explicit(c, d), want)
    for mut in muts:
        assert _violates(c, d, rc.explicit(c, d, mut=mut), want), (name, mut, "a wrong reference passes: a case is missing")


def test_every_mutation_has_a_case():
    assert {m for _, ms in rc.MUTATION_CASES for m in ms} == set(rc.MUTATIONS)


def test_refusals_and_workspace(L):
    """Argument checks run before any launch: the pointers are never dereferenced."""
    f = 0x1000
    for C, D, H, W, code in ((6, 8, 8, 8, -2), (10, 8, 8, 8, -2), (8, 1, 8, 8, -1), (8, 8, 1, 8, -1), (8, 8, 8, 1, -1), (8, 8, 0, 8, -1)):
        dims = (2, C, D, H, W)
        assert L.forge_rotate_fwd(f, f, f, f, *dims, None) == code
        assert L.forge_rotate_fwd_slots(f, f, f, f, f, *dims, None) == code
        assert L.forge_rotate_bwd(f, f, f, f, f, f, *dims, None) == code
        assert L.forge_rotate_bwd_slots(f, f, f, f, f, f, f, *dims, None) == code
        assert L.forge_rotate_bwd_det(f, f, f, f, f, f, *dims, 0, f, 1 << 20, None) == code
        assert L.forge_rotate_bwd_slots_det(f, f, f, f, f, f, f, *dims, 0, f, 1 << 20, None) == code
        assert L.forge_rotate_bwd_det_ws_bytes(*dims) == code and L.forge_rotate_bwd_slots_det_ws_bytes(*dims) == code
    for c in rc.CASES:
        n = len(c.views)
        want = n * rc.affine_blocks(c) * 12 * 4
        assert L.forge_rotate_bwd_det_ws_bytes(n, c.C, c.D, c.H, c.W) == want == L.forge_rotate_bwd_slots_det_ws_bytes(n, c.C, c.D, c.H, c.W), c.name
        # one byte short, a misaligned workspace, a misaligned dxf, accumulate = 2: refused
        dims = (n, c.C, c.D, c.H, c.W)
        assert L.forge_rotate_bwd_det(f, f, f, f, None, f, *dims, 0, f, want - 1, None) == -1
        assert L.forge_rotate_bwd_det(f, f, f, f, None, f, *dims, 0, f + 4, want, None) == -1
        assert L.forge_rotate_bwd_det(f, f, f, f, None, f + 4, *dims, 0, f, want, None) == -1
        assert L.forge_rotate_bwd_det(f, f, f, f, None, f, *dims, 2, f, want, None) == -1
    assert L.forge_rotate_bwd(f, None, f, f, None, f, 2, 8, 8, 8, 8, None) == -1          # dxf without vox
    assert L.forge_rotate_bwd(f, f, f, f, None, None, 2, 8, 8, 8, 8, None) == -1          # neither gradient
