"""The winding-number contract (include/forge_hip.h section g3c) without a GPU: the float64 restatement of tests/winding_cases.py against an
independently written second formulation and against known answers, the conditions the fixtures of tests/test_gpu_winding.py must meet, the
measurement of K that the GPU tests' tolerance rests on, the constants of volume_iou's point sequence, and what the wrappers and the C entry
refuse before any device call."""
import ctypes
import math

import numpy as np
import pytest
import torch

import geom_cases as gc
import winding_cases as wc


def test_restatement_agrees_with_a_second_formulation():
    """Van Oosterom and Strackee's atan2 against the sum of the dihedral angles minus pi (Girard), float64 both: within 1e-12 on every
    (query, candidate face) pair of every case."""
    worst = 0.0
    for im, iF in wc.GRID:
        for b in range(3):
            r = wc.restated(im, iF, b)
            if not r.cand.any() or not len(r.q):
                continue
            other = wc.second64(r.q[:, None, :], r.a[None], r.b[None], r.c[None])
            worst = max(worst, float(np.where(r.cand[None, :], np.abs(other - r.theta), 0.0).max()))
    print("winding_cpu second formulation: worst |theta - theta'| = %.3g" % worst)
    assert worst <= 1e-12


def test_known_answers():
    v, f = gc.octahedron()
    r = wc.restate(np.array([[0, 0, 0], [0.05, -0.02, 0.03], [1, 1, 1], [0.5, 0, 0]], np.float32), v, f)
    assert np.abs(r.w - [1, 1, 0, 0]).max() <= 1e-15
    assert np.abs(wc.w32(r).astype(np.float64) - [1, 1, 0, 0]).max() <= 4 * wc.U
    flipped = wc.restate(r.q.astype(np.float32), v, f[:, ::-1])
    assert np.array_equal(flipped.w, -r.w) and np.abs(wc.w32(flipped).astype(np.float64) + [1, 1, 0, 0]).max() <= 4 * wc.U
    # the first octant of the unit sphere seen from the origin: an eighth of the sphere
    tri = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    one = wc.restate(np.zeros((1, 3), np.float32), tri, np.array([[0, 1, 2]]))
    assert abs(one.w[0] - 1 / 8) <= 1e-15 and abs(float(wc.w32(one)[0]) - 1 / 8) <= 2 * wc.U
    # one of the two triangles of a cube's face seen from the centre: half of a sixth
    cube = np.array([[1, -1, -1], [1, 1, -1], [1, 1, 1], [1, -1, 1]], np.float32)
    half = wc.restate(np.zeros((1, 3), np.float32), cube, np.array([[0, 1, 2], [0, 2, 3]]))
    assert np.abs(half.theta[0] * wc.INV_2PI - 1 / 12).max() <= 1e-15 and abs(half.w[0] - 1 / 6) <= 1e-15
    assert abs(float(wc.second64(np.zeros(3), *cube[:3])) * wc.INV_2PI - 1 / 12) <= 1e-15
    # a query on a vertex: that face's term drops (atan2(0, 0) counts as 0), in both precisions
    on = wc.restate(tri[:1], tri, np.array([[0, 1, 2]]))
    assert on.w[0] == 0 and wc.w32(on)[0] == 0 and np.isnan(wc.theta32(tri[0], *tri))


def test_bad_and_flat_faces_add_nothing():
    v, f, bad = gc.with_bad_faces(*gc.octahedron())
    q = wc.queries_for(*gc.octahedron(), 300, 3)
    r, clean = wc.restate(q, v, f), wc.restate(q, *gc.octahedron())
    assert not r.cand[bad].any() and (r.theta[:, bad] == 0).all() and np.abs(r.w - clean.w).max() <= 1e-15
    only_bad = wc.restate(q, v, f[bad])
    assert (only_bad.w == 0).all() and (wc.w32(only_bad) == 0).all() and (only_bad.scale == 0).all()


def test_atan2_polynomial_is_within_4u_and_takes_every_octant():
    g = np.random.default_rng(0)
    y, x = (g.standard_normal(200_000) * np.exp(g.uniform(-8, 8, 200_000))).astype(np.float32), g.standard_normal(200_000).astype(np.float32)
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    err = np.abs(wc.atan2_32(y, x).astype(np.float64) - ref) / np.abs(ref)
    print("winding_cpu atan2: worst relative error %.3g = %.2f u" % (err.max(), err.max() / wc.U))
    assert err.max() <= 4 * wc.U
    assert wc.atan2_32(0.0, 1.0) == 0 and wc.atan2_32(1.0, 0.0) == np.float32(math.pi / 2) and wc.atan2_32(-1.0, 0.0) == np.float32(-math.pi / 2)
    assert wc.atan2_32(1.0, -1.0) == np.float32(0.75 * math.pi) and np.isnan(wc.atan2_32(0.0, 0.0))


def test_cases_cover_the_launch_space():
    for im, kind in enumerate(wc.MESHES):
        cs = [wc.case(im, iF) for iF in range(len(wc.FACES))]
        assert {c.Nq for c in cs} == set(wc.QUERIES) and {c.packed for c in cs} == {False, True} and {c.xf for c in cs} == {False, True}, kind
        assert {c.q_count is None for c in cs} == {False, True}, kind
    assert wc.FACES == (1, 7, wc.TILE - 1, wc.TILE, wc.TILE + 1, 2 * wc.TILE + 1) and wc.GROUP == 8
    from forge_amd import ops
    assert wc.TILE == ops.nn_tile_faces()


def test_k_is_measured_and_the_fixtures_meet_their_conditions():
    """measured_k: numpy float32 in the header's order, grouped sums included, against the float64 restatement, in units of u scale. With the
    device's allowance K = 4 x that: per case at most 5 % of the queries have a tolerance above 1e-3, at most 1 % lie within their tolerance
    of the threshold 0.5 - and none on the whole (closed) extracted meshes, whose w is an integer up to rounding."""
    k = wc.measured_k()
    per = {}
    for im, iF in wc.GRID:
        loose = near = total = 0
        for b in range(3):
            r = wc.restated(im, iF, b)
            per[wc.MESHES[im]] = max(per.get(wc.MESHES[im], 0.0), wc.k_of(r, wc.w32(r)))
            tol = 4 * k * wc.U * r.scale
            loose, near, total = loose + int((tol > 1e-3).sum()), near + int((np.abs(r.w - 0.5) <= tol).sum()), total + len(r.q)
        assert loose <= 0.05 * total and near <= 0.01 * total, (wc.case(im, iF).name, loose, near, total)
    for kind, kk in per.items():
        print("winding_cpu measured %-10s K %.3f" % (kind, kk))
    print("winding_cpu measured K = %.3f; the device is allowed %.3f" % (k, 4 * k))
    assert k == max(per.values()) and 0.0 < k < 64.0            # finite, and of the size rounding gives
    for kind in wc.CLOSED:
        _, _, _, r = wc.whole_closed(kind)
        tol = 4 * k * wc.U * r.scale
        assert (np.abs(r.w - 0.5) > tol).all() and np.abs(r.w - np.rint(r.w)).max() <= 1e-13 and set(np.rint(r.w)) == {0.0, 1.0}, kind
        assert wc.k_of(r, wc.w32(r)) <= k * 4


def test_r3_constants_and_first_points():
    """volume_iou's points: the R3 sequence in 32-bit wrap-around integers. The constants are round(2^32 / g^k) for the real root g of
    g^4 = g + 1; the first points are pinned, and the restatement below is the definition."""
    from forge_amd import geometry
    g = 1.2207440846057596
    assert abs(g ** 4 - g - 1) < 1e-14 and geometry.R3 == tuple(round(2 ** 32 / g ** k) for k in (1, 2, 3)) == (3518319155, 2882110345, 2360945575)
    p = geometry.r3_points(1000)
    i = np.arange(1000, dtype=np.uint64)
    ref = np.stack([(((i * np.uint64(c) + np.uint64(1 << 31)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 for c in geometry.R3], 1)
    assert p.dtype == torch.float32 and np.array_equal(p.numpy().astype(np.float64), ref) and ref.min() >= 0 and ref.max() < 1
    assert p[0].tolist() == [0.5, 0.5, 0.5]
    assert (p[1] * 2 ** 24).tolist() == [5354826.0, 2869635.0, 833835.0] and (p[2] * 2 ** 24).tolist() == [2321044.0, 14127879.0, 10056279.0]
    # low discrepancy: every cell of a 5 x 5 x 5 grid holds 1000 / 125 = 8 of the first 1000 points up to half of that (independent uniform
    # draws, at a standard deviation of 2.8 per cell, leave cells with 2 and with 16)
    cells = np.bincount((np.floor(ref * 5) @ [25, 5, 1]).astype(int), minlength=125)
    assert cells.min() >= 4 and cells.max() <= 12


def test_ops_refuse_cpu_tensors_and_wrong_shapes(monkeypatch):
    from forge_amd import _lib, geometry, ops
    q = torch.zeros(2, 8, 3)
    v, f, c = torch.zeros(2, 4, 3), torch.zeros(2, 5, 3, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.winding_number(q, v, f, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.winding_number(q, geometry.Mesh(v[0], v[0], f[0]))
    with pytest.raises(TypeError, match="must be tensors"):
        ops.winding_number(q, v.numpy(), f, c)
    with pytest.raises(ValueError, match="shape"):
        geometry.voxelize(geometry.Mesh(v[0], v[0], f[0]), (4, 4))
    # shapes and dtypes are judged before the library's launch is reached: meta tensors, and a launch that fails the test
    monkeypatch.setattr(ops, "_require_cuda", lambda *t: None)
    meta = lambda t: t.to("meta")                                                  # noqa: E731
    q, v, f, c = meta(q), meta(v), meta(f), meta(c)
    real = _lib.lib()

    class NoLaunch:
        forge_winding_workspace_bytes = real.forge_winding_workspace_bytes          # host arithmetic

        def forge_winding_number(self, *a):
            pytest.fail("the launch was reached")
    monkeypatch.setattr(_lib, "lib", lambda: NoLaunch())
    for bad in (lambda: ops.winding_number(q[0], v, f, c), lambda: ops.winding_number(meta(torch.zeros(2, 8, 2)), v, f, c),
                lambda: ops.winding_number(q, v[0], f[0], c), lambda: ops.winding_number(q, v, f, c[:1]),
                lambda: ops.winding_number(q, v, f, c, xf_mesh=meta(torch.zeros(2, 16))), lambda: ops.winding_number(q, v, f, c, q_count=meta(torch.zeros(3, dtype=torch.int32))),
                lambda: ops.winding_number(meta(torch.zeros(2, 8, 6))[..., ::2], v, f, c),
                lambda: ops.winding_number(q, v, f, c, workspace=meta(torch.zeros(2 * 5 * 48 + 15, dtype=torch.uint8)))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.winding_number(q.double(), v, f, c), lambda: ops.winding_number(q, v, f.long(), c)):
        with pytest.raises(TypeError):
            bad()


def test_c_entry_refuses_bad_arguments_before_any_device_call():
    """Section g3b's list, which g3c takes over. The pointers are never dereferenced: every check runs before the first launch."""
    from forge_amd import _lib
    L = _lib.lib()
    EINVAL, ESHAPE = -1, -2
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    need = _lib.size_query("forge_winding_workspace_bytes", 2, 5, 0)
    assert need == 2 * 5 * 48 + 16 == _lib.size_query("forge_nn_triangles_workspace_bytes", 2, 5, 0)
    assert _lib.size_query("forge_winding_workspace_bytes", 2, 5, 1) == 5 * 48 + 16
    assert L.forge_winding_workspace_bytes(0, 5, 0) == EINVAL and L.forge_winding_workspace_bytes(2, -1, 0) == EINVAL
    assert L.forge_winding_workspace_bytes(65536, 5, 0) == ESHAPE and L.forge_winding_workspace_bytes(3, 2 ** 30, 0) == ESHAPE

    def call(q=p, counts=p, vertices=p, faces=p, ws=p, w=p, B=2, Nq=8, mv=4, mf=5, nbytes=need, offsets=None):
        return L.forge_winding_number(q, None, None, vertices, faces, counts, offsets, None, B, Nq, mv, mf, ws, nbytes, w, None)
    for kw in (dict(q=None), dict(counts=None), dict(ws=None), dict(w=None), dict(vertices=None), dict(faces=None), dict(B=0), dict(Nq=0), dict(mv=-1),
               dict(mf=-1), dict(nbytes=need - 1), dict(ws=odd)):
        assert call(**kw) == EINVAL, kw
        assert L.forge_last_error().decode().startswith("forge_winding_number"), kw
    assert "aligned" in L.forge_last_error().decode()
    big = 2 ** 31 - 1
    for kw in (dict(B=65536), dict(B=3, mf=2 ** 30), dict(B=3, mv=2 ** 30), dict(Nq=big - 100), dict(B=1, mf=big - 100, nbytes=2 ** 40),
               dict(mf=big - 100, offsets=p, nbytes=2 ** 40)):
        assert call(**kw) == ESHAPE, kw
