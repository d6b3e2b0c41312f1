"""Alignment on the MI355X (forge_amd.geometry -> csrc/align.hip) against the float64 numpy restatement of its contract (tests/align_cases.py,
include/forge_hip.h section g5).

Bounds. Moments: each of the 21 sums within n 2^-53 sum |term| of math.fsum over the same terms (any summation order satisfies it; the terms are
exact products of widened fp32 values). T, SCALE, RMSE, SV and the other float64 entries of a state row: the restatement's own float64 error is
measured against the same restatement in numpy.longdouble on every case of this file (align_cases.self_error), and the device - which contracts
fmas, sums in another order and takes its SVD by Jacobi sweeps - is allowed 16 times the maximum, as |difference| / max(1, |value|). Integers are
equal. The ICP tests assert lengths: align_cases.fit_bound, the distance the fp32 roundings of xf, of its fma chain and of b can move a point."""
import math

import numpy as np
import pytest
import torch

import align_cases as ac
import mesh_cases as mc

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 255, 257, 1000)
FLOAT_COLS = list(range(ac.T, ac.T + 12)) + [ac.SCALE, ac.RMSE, ac.CUT2, ac.DELTA] + list(range(ac.SV, ac.SV + 3)) + [ac.SCORE] + list(range(ac.CQ, ac.CP + 3))
INT_COLS = [ac.N_IN, ac.N_VALID, ac.ITERATIONS]
_CACHE = {}


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dt is None else t.to(dt)


def step_with_partials(q, p, state, xf, status, idx, d2, qc, pc, with_scale, reject=0.0, reject_floor=0.0, clamp2=math.inf):
    """forge_align_step through the C entry itself, on a work space of this test's own, so that the per-workgroup moments of launch 1 can be
    looked at: [B, forge_align_blocks(), PARTIAL] float64 (zeros where a frozen pair wrote nothing). state, xf, status are updated in place."""
    from forge_amd import _lib, ops
    B, Nq, Np = q.shape[0], q.shape[1], p.shape[1]
    L = _lib.lib()
    partial = torch.zeros(int(L.forge_align_partial_doubles(B)), dtype=torch.float64, device="cuda")
    _lib.check(L.forge_align_step(_lib.ptr(q), _lib.ptr(p), _lib.ptr(qc), _lib.ptr(pc), _lib.ptr(idx), _lib.ptr(d2), B, Nq, Np, int(with_scale), 1,
                                  float(reject), float(reject_floor), 0.0, ops.ALIGN_RANK_TOL, float(clamp2), _lib.ptr(partial), _lib.ptr(state),
                                  _lib.ptr(xf), _lib.ptr(status), _lib.current_stream()), "forge_align_step")
    return partial.view(B, ops.align_blocks(), ac.PARTIAL)


def step_cases():
    """Every (N, counts, with_scale) case, built once and never modified: two device steps per case (the first from the identity with nothing
    rejected, the second after a new search, rejecting beyond 2 rms), each against the restatement started from the DEVICE's incoming state and fed
    the device's own idx and d2 - so only the step is under test. -> {key: [per step: dict]}, and the largest self error of the restatement."""
    if "steps" in _CACHE:
        return _CACHE["steps"]
    from forge_amd import ops
    out, worst_self = {}, 0.0
    for N in SIZES:
        q = np.stack([ac.shape(N, 10 + b) for b in range(3)])
        Ms = [ac.similarity(8 + 3 * b, (1, 2 - b, 3), 1.0 + 0.05 * b, ac.SHIFT) for b in range(3)]
        noise = np.random.default_rng(N).standard_normal((3, N, 3)) * 0.004
        p = np.stack([ac.apply(Ms[b], q[b].astype(np.float64) + noise[b])[::-1].copy() for b in range(3)])
        for counts in (False, True):
            qc = np.array([N, 0, (N + 1) // 2], np.int32) if counts else None
            pc = np.array([N, N, (N + 1) // 2], np.int32) if counts else None
            for with_scale in (False, True):
                tq, tp, tqc, tpc = dev(q), dev(p), None if qc is None else dev(qc), None if pc is None else dev(pc)
                state, xf, status = ops.align_state(None, 3, "cuda")
                steps = []
                for k, kw in enumerate((dict(reject=0.0), dict(reject=2.0, reject_floor=1e-3, clamp2=1e-4))):
                    d2, idx = ops.nn_points(tq, tp, tqc, tpc, xf)
                    st_in, bits_in = state.cpu().numpy().copy(), status.cpu().numpy().copy()
                    partial = step_with_partials(tq, tp, state, xf, status, idx, d2, tqc, tpc, with_scale, **kw)
                    rec = dict(st_in=st_in, bits_in=bits_in, idx=idx.cpu().numpy(), d2=d2.cpu().numpy(), state=state.cpu().numpy().copy(),
                               status=status.cpu().numpy().copy(), xf=xf.cpu().numpy().copy(), partial=partial.cpu().numpy(), kw=kw, ref=[])
                    for b in range(3):
                        args = dict(idx=rec["idx"][b], d2=rec["d2"][b], nq=None if qc is None else qc[b], np_=None if pc is None else pc[b],
                                    with_scale=with_scale, **kw)
                        rec["ref"].append(ac.step(q[b], p[b], st_in[b], int(bits_in[b]), **args))
                        worst_self = max(worst_self, ac.self_error(q[b], p[b], st_in[b], int(bits_in[b]), **args))
                    steps.append(rec)
                out[(N, counts, with_scale)] = (q, p, qc, pc, steps)
    print("align step: restatement float64 vs longdouble, largest error over %d cases: %.3g" % (len(out), worst_self))
    _CACHE["steps"] = (out, worst_self)
    return _CACHE["steps"]


def rel(got, ref):
    return abs(got - ref) / max(1.0, abs(ref))


@pytest.mark.parametrize("with_scale", [False, True], ids=["rigid", "scale"])
@pytest.mark.parametrize("counts", [False, True], ids=["full", "counts"])
@pytest.mark.parametrize("N", SIZES)
def test_step_against_the_restatement(N, counts, with_scale):
    cases, worst_self = step_cases()
    assert 0 < worst_self < 1e-12
    tol = 16 * worst_self
    q, p, qc, pc, steps = cases[(N, counts, with_scale)]
    worst = worst_m = 0.0
    for rec in steps:
        for b in range(3):
            ref, bits, xf = rec["ref"][b]
            got = rec["state"][b]
            # the moments: the partials of launch 1 added in workgroup order, as launch 2 adds them
            nq, np_ = (None, None) if qc is None else (qc[b], pc[b])
            terms = ac.row_terms(q[b], p[b], rec["idx"][b], rec["d2"][b], nq, np_, rec["st_in"][b][ac.CUT2], rec["kw"].get("clamp2", np.inf))
            exact, mag = ac.exact_moments(terms) if len(terms) else (np.zeros(ac.PARTIAL), np.zeros(ac.PARTIAL))
            m = np.zeros(ac.PARTIAL)
            for blk in rec["partial"][b]:
                m = m + blk
            bound = len(terms) * 2.0 ** -53 * mag
            assert (np.abs(m - exact) <= bound).all(), (b, m - exact, bound)
            worst_m = max(worst_m, float((np.abs(m - exact) / np.maximum(bound, 1e-300)).max()))
            # integers and flags
            # CONVERGED is `DELTA <= tol` (tol = 0 here) and DELTA carries the error of T: where the restatement's DELTA lies within the
            # tolerance of the threshold the bit is the device's to decide (a step that meets the same inliers again gives the device the
            # same T bit for bit, DELTA = 0, and the restatement a T a few 1e-16 from the device's)
            # An EMPTY row never counts as converged on either side: there every bit is compared.
            mask = ~0 if (bits & ac.EMPTY or abs(ref[ac.DELTA] - 0.0) > tol) else ~ac.CONVERGED
            assert (int(rec["status"][b]) & mask) == (bits & mask), (b, rec["status"][b], bits)
            for c in INT_COLS:
                assert got[c] == ref[c], (b, c, got[c], ref[c])
            assert np.array_equal(rec["xf"][b], got[:12].astype(np.float32))
            if bits & ac.EMPTY:
                assert np.array_equal(got[:13], rec["st_in"][b][:13]) and got[ac.DELTA] == 0          # T and SCALE are kept
                continue
            if bits & ac.RANK:
                continue                                                                             # the turn about the line is arbitrary
            for c in FLOAT_COLS:
                if np.isnan(ref[c]) or np.isinf(ref[c]):
                    assert np.array_equal(got[c], ref[c], equal_nan=True), (b, c, got[c], ref[c])
                else:
                    worst = max(worst, rel(got[c], ref[c]))
                    assert rel(got[c], ref[c]) <= tol, (b, c, got[c], ref[c], tol)
    print("align step N=%d counts=%s scale=%s: state error / tolerance = %.3f (tolerance %.3g), moment error / bound = %.3f" % (
        N, counts, with_scale, worst / tol, tol, worst_m))


# -------------------------------------------------------------------------------------------------------------- known correspondences
def test_fit_similarity_recovers_known_transforms():
    from forge_amd.geometry import fit_similarity
    a = ac.shape(1000, 3)
    M1, M2 = ac.similarity(15, (1, 2, 3), 1.1, ac.SHIFT), ac.similarity(15, (1, 2, 3), 1.0, ac.SHIFT)
    for M, with_scale in ((M1, True), (M2, False), (M2, True)):
        b = ac.apply(M, a)
        res = fit_similarity(dev(a), dev(b), with_scale=with_scale)
        bound = ac.fit_bound(a, b, M)
        T = res.transform[0].cpu().numpy()
        assert int(res.status[0]) == 0 and int(res.inliers[0]) == 1000 and int(res.start[0]) == 0 and int(res.iterations[0]) == 1
        assert np.abs(T - M).max() <= bound and abs(float(res.scale[0]) - np.linalg.norm(M[0, :3])) <= bound
        assert np.array_equal(T[3], [0, 0, 0, 1]) and float(res.rmse[0]) <= bound
        if not with_scale:
            assert float(res.scale[0]) == 1.0


def test_fit_similarity_degenerate_inputs():
    from forge_amd import ops
    from forge_amd.geometry import fit_similarity
    M = ac.similarity(15, (1, 2, 3), 1.0, ac.SHIFT)
    rng = np.random.default_rng(5)
    flat = np.concatenate([rng.random((50, 2)) - 0.5, np.zeros((50, 1))], axis=1).astype(np.float32)
    line = (np.linspace(-0.4, 0.4, 50)[:, None] * np.array([[1.0, 2.0, 3.0]]) / math.sqrt(14)).astype(np.float32)
    a = np.stack([flat, line, flat])
    b = np.stack([ac.apply(M, x) for x in a])
    res = fit_similarity(dev(a), dev(b), with_scale=False, counts=dev(np.array([50, 50, 2], np.int32)))
    status = res.status.cpu().numpy() & ~ops.ALIGN_CONVERGED
    assert status.tolist() == [0, ops.ALIGN_RANK, ops.ALIGN_EMPTY] and res.start.cpu().tolist() == [0, 0, -1]
    T = res.transform.cpu().numpy()
    assert np.abs(T[0] - M).max() <= 1e-6                                                            # a plane (sv[2] = 0) fixes the rotation
    for k in (0, 1):
        R = T[k][:3, :3]
        assert abs(np.linalg.det(R) - 1) < 1e-9 and np.abs(R @ R.T - np.eye(3)).max() < 1e-9        # proper all the same
    assert np.array_equal(T[2], np.eye(4)) and res.inliers.cpu().tolist() == [50, 50, 2]            # two points: T is kept
    # a NaN row is skipped and flagged
    bad = ac.shape(300, 4)
    good_b = ac.apply(M, bad)
    clean = fit_similarity(dev(bad[1:]), dev(good_b[1:]), with_scale=False)
    bad[0, 1] = np.nan
    res = fit_similarity(dev(bad), dev(good_b), with_scale=False)
    assert int(res.status[0]) & ops.ALIGN_NONFINITE and int(res.inliers[0]) == 299
    assert float((res.transform - clean.transform).abs().max()) <= 1e-13


# --------------------------------------------------------------------------------------------------------------------------------- ICP
def icp_inputs():
    if "icp" not in _CACHE:
        a = ac.shape(1024, 7)
        _CACHE["icp"] = (a, dev(a))
    return _CACHE["icp"]


@pytest.mark.parametrize("name,M,with_scale", ac.ICP_CASES, ids=[c[0] for c in ac.ICP_CASES])
def test_icp_same_points(name, M, with_scale):
    from forge_amd import ops
    from forge_amd.geometry import align_points
    a, ta = icp_inputs()
    b = ac.apply(M, a)
    res = align_points(ta, dev(b), iterations=40, with_scale=with_scale, tol=0.0)
    bound = ac.fit_bound(a, b, M)
    err = np.abs(res.transform[0].cpu().numpy() - M).max()
    print("icp %s: %d iterations, rmse %.3g, |T - M| %.3g, bound %.3g" % (name, int(res.iterations[0]), float(res.rmse[0]), err, bound))
    assert int(res.status[0]) == ops.ALIGN_CONVERGED and int(res.inliers[0]) == 1024 and int(res.start[0]) == 0
    assert float(res.rmse[0]) <= bound and err <= bound and int(res.iterations[0]) < 40


@pytest.mark.parametrize("floor", [0.0, 1e-3], ids=["reject=3", "reject=3 floor=1e-3"])
def test_icp_rejection_drops_the_floaters(floor):
    """The last 51 rows of a are floaters. reject=3 alone (reject_floor = 0, the default): the fit is the clean one, to the bound of the same-point
    cases, with 973 inliers. The same with a floor of 1e-3 (far above the fp32 noise the inliers end at, far below the floaters' distances), which
    keeps the threshold from following the residual down. Without rejection the floaters pull the transform away."""
    from forge_amd import ops
    from forge_amd.geometry import align_points
    a, _ = icp_inputs()
    M = ac.ICP_CASES[0][1]
    b = ac.apply(M, a)
    a = a.copy()
    a[-ac.N_FLOATERS:] = ac.floaters()
    bound = ac.fit_bound(a[:-ac.N_FLOATERS], b, M)
    res = align_points(dev(a), dev(b), iterations=40, reject=3.0, reject_floor=floor)
    plain = align_points(dev(a), dev(b), iterations=40, reject=0.0)
    err, err_plain = np.abs(res.transform[0].cpu().numpy() - M).max(), np.abs(plain.transform[0].cpu().numpy() - M).max()
    print("rejection: |T - M| %.3g with reject=3, reject_floor=%g (%d inliers, %d iterations, status %d), %.3g with reject=0; bound %.3g" % (
        err, floor, int(res.inliers[0]), int(res.iterations[0]), int(res.status[0]), err_plain, bound))
    assert err <= bound and int(res.inliers[0]) == 1024 - ac.N_FLOATERS and int(res.status[0]) == ops.ALIGN_CONVERGED
    assert int(plain.inliers[0]) == 1024 and err_plain > bound


def test_multi_start():
    from forge_amd import ops
    from forge_amd.geometry import align_points, rotation_starts
    a, ta = icp_inputs()
    b = ac.apply(ac.FAR, a)
    tb = dev(b)
    bound = ac.fit_bound(a, b, ac.FAR)
    cube = rotation_starts("cube")
    res = align_points(ta, tb, iterations=40, starts=cube)
    k, err = int(res.start[0]), np.abs(res.transform[0].cpu().numpy() - ac.FAR).max()
    print("multi-start: start %d, %d iterations, rmse %.3g, |T - M| %.3g, bound %.3g" % (k, int(res.iterations[0]), float(res.rmse[0]), err, bound))
    assert 0 < k < 24 and int(res.status[0]) == ops.ALIGN_CONVERGED and err <= bound and float(res.rmse[0]) <= bound
    alone = align_points(ta, tb, iterations=40)
    assert np.abs(alone.transform[0].cpu().numpy() - ac.FAR).max() > 1000 * bound                   # the identity alone does not reach it
    for order, want in (([k, 0, k], 0), ([0, k, k], 1)):                                             # a duplicated start: the lower index
        dup = align_points(ta, tb, iterations=40, starts=cube[order])
        assert int(dup.start[0]) == want and torch.equal(dup.transform, res.transform) and torch.equal(dup.rmse, res.rmse)


def test_select_rules_on_the_device():
    from forge_amd import ops
    state = torch.zeros(8, ops.ALIGN_STATE_DOUBLES, dtype=torch.float64, device="cuda")
    state[:, ops.ALIGN_T] = torch.arange(8, dtype=torch.float64)
    state[:, ops.ALIGN_SCORE] = torch.tensor([3.0, 1.0, 1.0, 2.0, math.nan, math.inf, 0.0, math.nan], dtype=torch.float64)
    status = torch.tensor([0, 0, 0, 0, 0, 0, ops.ALIGN_EMPTY, ops.ALIGN_RANK], dtype=torch.int32, device="cuda")
    T, xf, best, st, stat = ops.align_select(state, status, 4)
    assert best.cpu().tolist() == [1, -1] and T[:, 0, 0].cpu().tolist() == [1.0, 4.0] and xf[:, 0].cpu().tolist() == [1.0, 4.0]
    assert same([st], [state[[1, 4]]]) and stat.cpu().tolist() == [0, 0]
    assert T[:, 3].cpu().tolist() == [[0, 0, 0, 1]] * 2
    assert ops.align_select(state, status, 2)[2].cpu().tolist() == [1, 0, -1, -1]


# --------------------------------------------------------------------------------------------------------------------- reproducibility
def same(x, y):
    return all(torch.equal(torch.nan_to_num(p.double(), nan=-1.0), torch.nan_to_num(q.double(), nan=-1.0)) for p, q in zip(x, y))


def test_bits_are_reproducible_and_independent_of_the_batch_and_of_padding():
    from forge_amd.geometry import align_points
    n = 700
    a = np.stack([ac.shape(n, 20 + k) for k in range(3)])
    b = np.stack([ac.apply(ac.ICP_CASES[k][1], ac.shape(n, 30 + k)) for k in range(3)])            # resampled: never converges to delta = 0
    kw = dict(iterations=6, reject=3.0, reject_floor=1e-3)
    ta, tb = dev(a), dev(b)
    first, again = align_points(ta, tb, **kw), align_points(ta, tb, **kw)
    assert same(first, again)
    for k in range(3):
        alone = align_points(ta[k:k + 1].contiguous(), tb[k:k + 1].contiguous(), **kw)
        assert same(alone, [t[k:k + 1] for t in first]), k
    pad_a = torch.cat([ta, torch.full((3, 37, 3), 0.123, device="cuda")], dim=1).contiguous()
    pad_b = torch.cat([tb, torch.full((3, 300, 3), -0.05, device="cuda")], dim=1).contiguous()
    cnt = torch.full((3,), n, dtype=torch.int32, device="cuda")
    assert same(align_points(pad_a, pad_b, counts_a=cnt, counts_b=cnt, **kw), first)
    assert int(first.iterations[0]) == 6 and float(first.rmse[0]) > 0


# ----------------------------------------------------------------------------------------------------------------------------- capture
def blob_batch():
    from forge_amd.geometry import extract_mesh
    dens = torch.from_numpy(np.stack([mc.blob(8), mc.blob(8, (0.05, -0.03, 0.02)), mc.below(8)])[:, None]).cuda()
    other = torch.from_numpy(np.stack([mc.blob(8, (0.0, 0.04, 0.0)), mc.blob(8), mc.blob(8)])[:, None]).cuda()
    return extract_mesh(dens, max_vertices=600, max_faces=1100), extract_mesh(other, max_vertices=600, max_faces=1100)


def test_alignment_runs_in_a_captured_graph():
    """Nothing synchronises or is read back (a call that did would raise inside the capture): captured once, replayed once, the bits of the eager call."""
    from forge_amd import ops
    from forge_amd.geometry import align_points, mesh_metrics, rotation_starts
    a, ta = icp_inputs()
    tb = dev(ac.apply(ac.ICP_CASES[2][1], a))
    starts = rotation_starts("cube")[:3].cuda()
    pred, gt = blob_batch()

    def chain():
        al = align_points(ta, tb, iterations=5, starts=starts, reject=3.0)
        res = mesh_metrics(pred, gt, n=500, align={"n": 300, "iterations": 4})
        return list(al) + list(res.pop("alignment")) + [res[k] for k in sorted(res)]

    eager = [t.clone() for t in chain()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = chain()
    g.replay()
    torch.cuda.synchronize()
    assert same(out, eager)
    status = eager[7 + 6].cpu().tolist()                                                             # the hook's Alignment.status
    assert status[2] & ops.ALIGN_EMPTY and not status[0] & ops.ALIGN_EMPTY                          # the empty volume has nothing to fit


# -------------------------------------------------------------------------------------------------------------------------------- hook
def test_mesh_metrics_align_hook():
    from forge_amd.geometry import Mesh, extract_mesh, mesh_metrics
    (pred,) = extract_mesh(torch.from_numpy(mc.blob(16)[None, None]).cuda())
    M = ac.similarity(10, (1, 2, 3), 1.0, (0.04, -0.02, 0.03))
    Mt = torch.from_numpy(M).cuda()
    moved = (pred.vertices.double() @ Mt[:3, :3].T + Mt[:3, 3]).float()
    gt = Mesh(moved, (pred.normals.double() @ Mt[:3, :3].T).float(), pred.faces)
    kw = dict(n=4096, thresholds=(0.01, 0.02))
    plain = mesh_metrics(pred, gt, **kw)
    res = mesh_metrics(pred, gt, align={"n": 2048, "iterations": 12}, **kw)
    al = res.pop("alignment")
    again = mesh_metrics(pred, gt, transform=al.transform, **kw)
    assert sorted(res) == sorted(again) == sorted(plain)
    for k in res:
        assert same([res[k]], [again[k]]), k
    for k in plain:
        assert same([plain[k]], [mesh_metrics(pred, gt, align=None, **kw)[k]]), k
    print("hook: chamfer_l1 %.5f unaligned, %.5f after ICP (rmse %.3g, %d iterations)" % (float(plain["chamfer_l1"][0]), float(res["chamfer_l1"][0]),
                                                                                       float(al.rmse[0]), int(al.iterations[0])))
    # aligned, what is left is the sampling: two different draws of n points of one surface of area A lie within the sample spacing sqrt(A / n)
    # of each other on average (the bound tests/test_gpu_geometry_metrics.py takes for a mesh against itself); unaligned, the shift shows
    spacing = math.sqrt(float(pred.area()) / kw["n"])
    assert float(res["chamfer_l1"][0]) <= spacing < float(plain["chamfer_l1"][0])
    assert float((al.transform[0, :3, 3] - Mt[:3, 3]).abs().max()) < 0.01                              # the blob is a sphere about the origin: its centre moves by the shift
    with pytest.raises(ValueError, match="align"):
        mesh_metrics(pred, gt, align="umeyama")
    from forge_amd.evaluation import evaluate_geometry
    ev = evaluate_geometry(pred, gt, align={"n": 2048, "iterations": 12}, **kw)
    assert same([ev["chamfer_l1"]], [res["chamfer_l1"]]) and same(list(ev["alignment"]), list(al))
