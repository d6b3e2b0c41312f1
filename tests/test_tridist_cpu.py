"""The point-to-triangle contract (include/forge_hip.h section g3b) without a GPU: the float64 restatement of tests/tri_cases.py against an
independently written second formulation and against known answers, the conditions the fixtures of tests/test_gpu_tridist.py must meet, and
the measurement of K_lo / K_hi that the GPU tests' tolerances rest on."""
import numpy as np
import pytest

import geom_cases as gc
import tri_cases as tc

GRID = [(im, iF) for im in range(len(tc.MESHES)) for iF in range(len(tc.FACES))]


def test_tile_constant_is_the_librarys():
    from forge_amd import ops
    assert tc.TILE == ops.nn_tile_faces()


def test_restatement_agrees_with_a_second_formulation():
    """Ericson's closest point against plane-distance-or-nearest-segment, float64 both: within 1e-12 L on every (query, candidate face) pair of
    every case, L the largest corner distance from the query."""
    worst = 0.0
    for im, iF in GRID:
        for b in range(3):
            r = tc.restated(im, iF, b)
            if not r.cand.any() or not len(r.q):
                continue
            other = tc.second64(r.q[:, None, :], r.a[None], r.b[None], r.c[None])
            err = np.where(r.cand[None, :], np.abs(other - r.T) / r.L, 0.0)
            worst = max(worst, float(err.max()))
    print("tridist_cpu second formulation: worst |T - T'| / L = %.3g" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("q, region, point", [
    ((-1, -1, 0), tc.VERTEX_A, (0, 0, 0)), ((6, -1, 0), tc.VERTEX_B, (4, 0, 0)), ((-2, 5, 0), tc.VERTEX_C, (0, 2, 0)),
    ((2, -3, 4), tc.EDGE_AB, (2, 0, 0)), ((-5, 1, 0), tc.EDGE_AC, (0, 1, 0)), ((3, 3, 0), tc.EDGE_BC, (2, 1, 0)),
    ((1, 0.5, 2), tc.INTERIOR, (1, 0.5, 0))])
def test_known_answers_one_query_per_region(q, region, point):
    """a = (0,0,0), b = (4,0,0), c = (0,2,0): one query per Voronoi region, exact in float64 - every parameter of a foot point is 1/2 or 1/4 and
    the interior's denominator is |ab x ac|^2 = 64, so no operation rounds. (3,3,0) lies over the midpoint of bc: (q - b).(c - b) = 10 of 20."""
    v, f = tc.right_triangle()
    q, point = np.array(q, np.float64), np.array(point, np.float64)
    a, b, c = (v[f[0, k]].astype(np.float64) for k in range(3))
    d, p, reg = tc.closest64(q, a, b, c)
    assert int(reg) == region and np.array_equal(p, point) and float(d) == float(np.sqrt(((q - point) ** 2).sum()))
    assert float(tc.second64(q, a, b, c)) == pytest.approx(float(d), rel=1e-15)
    d2, P, reg32 = tc.closest32(q, a, b, c)                   # the fp32 order names the same region (its reciprocal of 20 rounds: not bit-exact)
    assert int(reg32) == region and np.abs(P.astype(np.float64) + q - point).max() <= 1e-6 and float(d2) == pytest.approx(float(d) ** 2, rel=1e-6)


def _coverage(im, iF):
    cov, n = np.zeros(3), 0
    for b in range(3):
        r = tc.restated(im, iF, b)
        if r.cand.any() and len(r.q):
            cov += np.bincount(tc.KIND[r.region[np.arange(len(r.q)), r.T.argmin(axis=1)]], minlength=3)
            n += len(r.q)
    return cov, n


def test_fixtures_reach_every_region():
    """A condition on the fixtures: the winning region of the restatement is a vertex, an edge and the interior at least 5 % of the time each -
    over the queries of every case with at least 7 faces and 255 queries, and over every mesh's cases together. (A single small triangle seen
    from 0.3 away is nearly always nearest at a corner: the one-face cases have the three kinds, not 5 % of each.)"""
    for im, kind in enumerate(tc.MESHES):
        pool, total = np.zeros(3), 0
        for iF, F in enumerate(tc.FACES):
            cov, n = _coverage(im, iF)
            pool, total = pool + cov, total + n
            if F >= 7 and tc.case(im, iF).Nq >= 255:
                assert (cov / n >= 0.05).all(), (kind, F, cov / n)
        print("tridist_cpu regions %-10s vertex %.3f edge %.3f interior %.3f of %d queries" % ((kind,) + tuple(pool / total) + (total,)))
        assert (pool / total >= 0.05).all(), (kind, pool / total)


def test_cases_cover_the_launch_space():
    """Every Nq, both layouts, with and without transforms and counts meet every mesh; every F meets every mesh by construction."""
    for im, kind in enumerate(tc.MESHES):
        cs = [tc.case(im, iF) for iF in range(len(tc.FACES))]
        assert {c.Nq for c in cs} == set(tc.QUERIES) and {c.packed for c in cs} == {False, True} and {c.xf for c in cs} == {False, True}, kind
        assert {c.q_count is None for c in cs} == {False, True}, kind


def test_bad_and_flat_faces_never_win():
    """The octahedron with a repeated corner, an index past the end and a negative index among its faces, and the soup's exactly collinear
    face: none is a candidate, none is ever named, and the fp32 order's NaN / garbage for them is never read."""
    v, f, bad = gc.with_bad_faces(*gc.octahedron())
    q = tc.queries_for(*gc.octahedron(), 300, 3)
    r = tc.restate(q, v, f)
    assert not r.cand[bad].any() and r.cand.sum() == len(f) - len(bad)
    val, face = tc.winner(tc.scored32(r))
    assert np.isfinite(val).all() and not np.isin(face, bad).any() and not np.isin(r.T.argmin(axis=1), bad).any()
    sv, sf = tc.soup()
    rs = tc.restate(tc.queries_for(sv, sf, 300, 4), sv, sf)
    assert not rs.cand[11] and rs.cand.sum() == len(sf) - 1 and not (tc.winner(tc.scored32(rs))[1] == 11).any()
    only_bad = tc.restate(q, v, f[bad])
    assert np.isinf(tc.winner(tc.scored32(only_bad))[0]).all() and (tc.winner(tc.scored32(only_bad))[1] == -1).all()


def test_k_is_measured_and_finite():
    """K_lo, K_hi: the fp32 expression order of the header (numpy float32, fma by fma) against the float64 restatement, over the cases of the
    GPU tests, in the form those tests assert (tri_cases.k_of_pair). The device is allowed 4 times these."""
    per = {}
    for im, iF in GRID:
        for b in range(3):
            r = tc.restated(im, iF, b)
            lo, hi = tc.k_of_pair(r, tc.scored32(r))
            k = per.setdefault(tc.MESHES[im], [0.0, 0.0])
            k[0], k[1] = max(k[0], lo), max(k[1], hi)
    for kind, (lo, hi) in per.items():
        print("tridist_cpu measured %-10s K_lo %.3f K_hi %.3f" % (kind, lo, hi))
    k_lo, k_hi = tc.measured_k()
    print("tridist_cpu measured K_lo = %.3f, K_hi = %.3f; the device is allowed %.3f and %.3f" % (k_lo, k_hi, 4 * k_lo, 4 * k_hi))
    assert (k_lo, k_hi) == (max(v[0] for v in per.values()), max(v[1] for v in per.values()))
    assert 0.0 < k_lo < 64.0 and 0.0 < k_hi < 64.0        # finite, and of the size rounding gives: a few units, not a defect of the restatement
