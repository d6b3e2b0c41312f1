"""CPU: the alignment contract (include/forge_hip.h section g5) on known answers, through its float64 restatement (tests/align_cases.py), and the
argument checks of its three C entry points, which return the documented codes before anything is launched. No GPU."""
import math
import os

import numpy as np
import pytest

import align_cases as ac

SHIFT, ICP_CASES = ac.SHIFT, ac.ICP_CASES


@pytest.mark.parametrize("n", [3, 4, 257, 1000])
@pytest.mark.parametrize("scale", [1.0, 1.1, 0.5])
def test_known_correspondences_recover_the_similarity(n, scale):
    """b = fp32(M a): the fit can miss M by no more than the rounding of b moves a point (fit_bound is that plus the fp32 transform's slack)."""
    a = ac.shape(n, 3)
    M = ac.similarity(15, (1, 2, 3), scale, SHIFT)
    b = ac.apply(M, a)
    st, status, xf = ac.step(a, b, ac.new_state(), 0, with_scale=scale != 1.0)
    assert status == 0 and st[ac.N_IN] == n and st[ac.ITERATIONS] == 1
    bound = ac.fit_bound(a, b, M) * (20 if n < 5 else 1)       # 3 or 4 points: no averaging, and the lever arm of 0.1-sized triangles
    assert np.abs(ac.matrix(st) - M).max() <= bound
    assert abs(st[ac.SCALE] - scale) <= bound
    assert np.array_equal(xf, st[:12].astype(np.float32))
    R = st[:12].reshape(3, 4)[:, :3] / st[ac.SCALE]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0


def test_a_mirrored_set_yields_a_proper_rotation():
    a = ac.shape(500, 4)
    b = (a * np.array([1, 1, -1], np.float32)).astype(np.float32)
    st, status, _ = ac.step(a, b, ac.new_state(), 0)
    R = st[:12].reshape(3, 4)[:, :3]
    assert status == 0 and np.linalg.det(R) == pytest.approx(1.0, abs=1e-12) and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    ld, _ = ac.project_so3(np.diag([3.0, 2.0, -1.0]), np.longdouble)      # the Jacobi of the longdouble path agrees
    assert np.abs(ld.astype(np.float64) - np.diag([1.0, 1.0, 1.0])).max() < 1e-15


def test_planar_collinear_and_tiny_sets():
    rng = np.random.default_rng(5)
    flat = np.concatenate([rng.random((50, 2)) - 0.5, np.zeros((50, 1))], axis=1).astype(np.float32)
    M = ac.similarity(15, (1, 2, 3), 1.0, SHIFT)
    st, status, _ = ac.step(flat, ac.apply(M, flat), ac.new_state(), 0)
    assert status == 0 and st[ac.SV + 2] <= 1e-7 * st[ac.SV] and np.abs(ac.matrix(st) - M).max() <= 1e-6       # a plane fixes the rotation
    line = (np.linspace(-0.4, 0.4, 50)[:, None] * np.array([[1.0, 2.0, 3.0]]) / math.sqrt(14)).astype(np.float64)
    st, status, _ = ac.step(line.astype(np.float32), ac.apply(M, line), ac.new_state(), 0)
    assert status & ac.RANK and not status & ac.EMPTY
    R = st[:12].reshape(3, 4)[:, :3]
    assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-9)                                                     # T is written all the same
    for n in (0, 1, 2):
        st, status, _ = ac.step(flat[:n], flat[:n], ac.new_state(), 0)
        assert status == ac.EMPTY and np.array_equal(st[:12], ac.new_state()[:12]) and st[ac.N_IN] == n and st[ac.ITERATIONS] == 1
    assert ac.step(flat, flat, ac.new_state(), 0, nq=2)[1] == ac.EMPTY                                           # counts limit the rows


def test_rows_that_are_skipped():
    a = ac.shape(40, 6)
    M = ac.similarity(15, (1, 2, 3), 1.0, SHIFT)
    b = ac.apply(M, a)
    clean, _, _ = ac.step(a[3:], b[3:], ac.new_state(), 0)
    bad = a.copy()
    bad[0, 1], bad[1, 2] = np.nan, np.inf
    idx = np.arange(40)
    idx[2] = -1
    st, status, _ = ac.step(bad, b, ac.new_state(), 0, idx=idx, d2=np.zeros(40, np.float32))
    assert status == ac.NONFINITE and st[ac.N_IN] == 37 and st[ac.N_VALID] == 37
    assert np.array_equal(st[:12], clean[:12])
    idx[5] = 40                                                                                                 # past p_count: never followed
    assert ac.step(a, b, ac.new_state(), 0, idx=idx, d2=np.zeros(40, np.float32))[0][ac.N_IN] == 38


def test_rejection_uses_the_incoming_threshold_and_sets_the_next():
    a = ac.shape(100, 8)
    d2 = np.full(100, 1e-4, np.float32)
    d2[:10] = 1.0
    st, status, _ = ac.step(a, a, ac.new_state(), 0, idx=np.arange(100), d2=d2, reject=3.0, clamp2=0.25)
    mean = (90 * float(np.float32(1e-4)) + 10 * 1.0) / 100
    assert st[ac.N_IN] == 100 and st[ac.CUT2] == pytest.approx(9 * mean, rel=1e-12)                             # CUT2 comes in as +inf
    assert st[ac.SCORE] == pytest.approx((90 * float(np.float32(1e-4)) + 10 * 0.25) / 100, rel=1e-12)
    st2, _, _ = ac.step(a, a, st, status & ~ac.CONVERGED, idx=np.arange(100), d2=d2, reject=3.0, reject_floor=0.5)
    assert st2[ac.N_IN] == 90 and st2[ac.N_VALID] == 100 and st2[ac.CUT2] == 0.25 and st2[ac.RMSE] == pytest.approx(math.sqrt(float(np.float32(1e-4))))


def test_a_converged_pair_is_frozen_and_statistics_leave_the_transform():
    a = ac.shape(64, 9)
    b = ac.apply(ac.similarity(10, (0, 0, 1)), a)
    st, status, _ = ac.step(a, b, ac.new_state(), 0)
    st2, status2, _ = ac.step(a, b, st, status)
    assert status2 & ac.CONVERGED and st2[ac.DELTA] == 0 and st2[ac.ITERATIONS] == 2                            # the same inputs: the same T
    st3, status3, _ = ac.step(a[::-1].copy(), b, st2, status2)
    assert np.array_equal(st3, st2) and status3 == status2
    stat, bits, _ = ac.step(a[::-1].copy(), b, st, status, update=False, d2=np.ones(64, np.float32), idx=np.arange(64))
    assert np.array_equal(stat[:13], st[:13]) and stat[ac.ITERATIONS] == 1 and stat[ac.RMSE] == 1.0 and bits == status


def test_selection():
    def row(score):
        st = ac.new_state()
        st[ac.SCORE] = score
        return st
    assert ac.select([row(3.0), row(1.0), row(1.0), row(2.0)], [0, 0, 0, 0])[0] == 1                            # the lowest index on a tie
    assert ac.select([row(np.nan), row(5.0)], [0, 0])[0] == 1 and ac.select([row(np.nan), row(np.nan)], [0, 0])[0] == -1
    assert ac.select([row(0.0), row(5.0)], [ac.EMPTY, ac.RANK])[0] == 1 and ac.select([row(0.0)], [ac.EMPTY])[0] == -1
    assert ac.select([row(np.inf)], [0])[0] == -1


@pytest.mark.parametrize("name,M,with_scale", ICP_CASES, ids=[c[0] for c in ICP_CASES])
def test_icp_reaches_its_fixed_point(name, M, with_scale):
    a = ac.shape(1024, 7)
    b = ac.apply(M, a)
    st, status = ac.icp(a, b, 40, with_scale=with_scale)
    bound = ac.fit_bound(a, b, M)
    print("icp %s: %d iterations, rmse %.3g, |T - M| %.3g, bound %.3g" % (name, st[ac.ITERATIONS], st[ac.RMSE], np.abs(ac.matrix(st) - M).max(), bound))
    assert status == ac.CONVERGED and st[ac.DELTA] == 0 and 12 <= st[ac.ITERATIONS] <= 20
    assert st[ac.RMSE] <= bound and np.abs(ac.matrix(st) - M).max() <= bound and st[ac.N_IN] == 1024


@pytest.mark.parametrize("floor", [0.0, 1e-3], ids=["reject=3", "reject=3 floor=1e-3"])
def test_icp_rejection_drops_the_floaters(floor):
    a = ac.shape(1024, 7)
    M = ICP_CASES[0][1]
    b = ac.apply(M, a)
    a[-51:] = ac.floaters()
    bound = ac.fit_bound(a[:-51], b, M)
    st, status = ac.icp(a, b, 40, reject=3.0, reject_floor=floor)
    assert status == ac.CONVERGED and st[ac.N_IN] == 973 and np.abs(ac.matrix(st) - M).max() <= bound
    plain, _ = ac.icp(a, b, 40)
    assert plain[ac.N_IN] == 1024 and np.abs(ac.matrix(plain) - M).max() > 1000 * bound


def test_rotation_starts_are_the_24_rotations_of_the_cube():
    from forge_amd.geometry import rotation_starts
    R = rotation_starts("cube").numpy()
    assert R.shape == (24, 3, 3) and np.array_equal(R[0], np.eye(3))
    assert len({tuple(r.reshape(9)) for r in R}) == 24
    for r in R:
        assert np.linalg.det(r) == pytest.approx(1.0) and np.array_equal(np.abs(r).sum(axis=0), np.ones(3)) and np.array_equal(r @ r.T, np.eye(3))
    with pytest.raises(ValueError):
        rotation_starts("icosahedron")


def test_argument_checks_return_the_documented_codes(built_lib):
    """FORGE_EINVAL = -1, FORGE_ESHAPE = -2, on pointers that are never followed: the checks run before any launch."""
    from forge_amd import _lib, ops
    L = _lib.lib()
    f = 0x1000
    inf = math.inf

    def step(q=f, p=f, idx=f, d2=f, B=1, Nq=8, Np=8, ws=0, up=1, rej=0.0, floor=0.0, tol=0.0, rank=1e-6, clamp=inf, partial=f, state=f, xf=f, status=f):
        return L.forge_align_step(q, p, None, None, idx, d2, B, Nq, Np, ws, up, rej, floor, tol, rank, clamp, partial, state, xf, status, None)
    for bad in (dict(q=None), dict(p=None), dict(partial=None), dict(state=None), dict(xf=None), dict(status=None), dict(B=0), dict(Nq=0), dict(Np=0),
                dict(ws=2), dict(up=-1), dict(rej=-1.0), dict(rej=inf), dict(floor=math.nan), dict(tol=-1e-9), dict(tol=inf), dict(rank=1.0),
                dict(rank=-0.1), dict(clamp=-1.0), dict(clamp=math.nan), dict(partial=f + 4), dict(state=f + 4)):
        assert step(**bad) == -1, bad
    assert b"forge_align_step" in L.forge_last_error()
    for bad in (dict(B=65536), dict(Nq=0x7fffffff), dict(Np=0x7fffffff)):
        assert step(**bad) == -2, bad

    def select(state=f, status=f, B=1, K=1, T=f, xf=f, best=f, so=f, sto=f):
        return L.forge_align_select(state, status, B, K, T, xf, best, so, sto, None)
    for bad in (dict(state=None), dict(status=None), dict(T=None), dict(xf=None), dict(best=None), dict(so=None), dict(sto=None), dict(B=0), dict(K=0),
                dict(state=f + 4), dict(T=f + 4), dict(so=f + 4)):
        assert select(**bad) == -1, bad
    assert select(B=65536) == -2 and select(B=65535, K=65535) == -2
    assert L.forge_align_partial_doubles(0) == -1 and L.forge_align_partial_doubles(65536) == -1
    assert L.forge_align_partial_doubles(3) == 3 * ops.align_blocks() * ac.PARTIAL
    assert (ops.ALIGN_STATE_DOUBLES, ops.ALIGN_SCORE, ops.ALIGN_CQ, ops.ALIGN_CP) == (ac.STATE, ac.SCORE, ac.CQ, ac.CP)
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "forge_hip.h")).read()
    for name, value in (("EMPTY", ac.EMPTY), ("RANK", ac.RANK), ("NONFINITE", ac.NONFINITE), ("CONVERGED", ac.CONVERGED), ("T", ac.T), ("SCALE", ac.SCALE),
                        ("RMSE", ac.RMSE), ("N_IN", ac.N_IN), ("N_VALID", ac.N_VALID), ("CUT2", ac.CUT2), ("DELTA", ac.DELTA),
                        ("ITERATIONS", ac.ITERATIONS), ("SV", ac.SV), ("SCORE", ac.SCORE), ("CQ", ac.CQ), ("CP", ac.CP), ("STATE_DOUBLES", ac.STATE)):
        assert "#define FORGE_ALIGN_%s %d\n" % (name, value) in header, name
        assert getattr(ops, "ALIGN_" + name) == value, name
