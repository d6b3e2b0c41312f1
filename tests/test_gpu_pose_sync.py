"""GPU (-m gpu): ops.pose_sync (forge_pose_sync) against the reference's own camera_synchronization (tests/golden/pose_sync.npz).

Conditioned cases (sigma_min / sigma_max >= 1e-2 in every view, asserted by the generator):
  - out within 2 float32 ulps of max(1, |x|) of `out_f64`, the reference fed float64 inputs: both are float64 arithmetic rounded once, and
    the float64 errors of ten squarings and a 3x3 SVD (1e-15) only matter where a value sits on a rounding boundary;
  - out within 2 max|out_f32 - out_f64| of that case + 2 ulps of `out_f32`, the reference as its callers run it;
  - status 0, and the singular values within 1e-9 (relative) of the golden's.
Degenerate cases: the rank bit is set and out stays finite. A NaN in one batch element flags that element alone and leaves its neighbours
bitwise unchanged. Two calls, and a batch against its single-element calls, are bitwise equal; a captured hipGraph replays to the eager result.
Measured on an MI355X: the largest distance from `out_f64` over all conditioned cases is 0 float32 ulps of max(1, |x|) (4.0e-15 absolute, on
entries whose exact value is 0), singular values within 9.2e-16 - profiles/r17_pose_sync_probe.txt.
"""
import numpy as np
import pytest
import torch

from forge_amd import ops
from test_pose_sync_cpu import case_inputs, ulp32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("pose_sync")


def run(g, c, dev, **kw):
    P, conf, pairs, N, squares, center = case_inputs(g, c)
    first = center == 0
    assert first or center == N // 2
    return ops.pose_sync(torch.from_numpy(P).to(dev), torch.from_numpy(conf).to(dev), pairs, N, squares=squares, center_first_camera=first, **kw)


def test_conditioned_cases_against_the_reference(dev, gold):
    worst_ulps, worst_abs, worst_sv = 0.0, 0.0, 0.0
    for c in gold["cases"]:
        out, status, sv = run(gold, c, dev, return_sv=True)
        out, status, sv = out.cpu().numpy().astype(np.float64), status.cpu().numpy(), sv.cpu().numpy()
        o64, o32 = gold[c + "__out_f64"].astype(np.float64), gold[c + "__out_f32"].astype(np.float64)
        e64 = np.abs(out - o64)
        r = (e64 / ulp32(o64)).max()
        svr = (np.abs(sv - gold[c + "__sv"]) / gold[c + "__sv"]).max()
        print("%-22s |out - out_f64| %.3e = %.2f ulps, |out_f32 - out_f64| %.3e, sv rel %.2e, status %s"
              % (c, e64.max(), r, np.abs(o32 - o64).max(), svr, status.tolist()))
        worst_ulps, worst_abs, worst_sv = max(worst_ulps, r), max(worst_abs, e64.max()), max(worst_sv, svr)
        assert r <= 2.0, (c, r)
        assert (np.abs(out - o32) <= 2 * np.abs(o32 - o64).max() + 2 * ulp32(o32)).all(), c
        assert (status == 0).all(), (c, status)
        assert svr <= 1e-9, (c, svr)
    print("worst over %d cases: %.2f float32 ulps of max(1, |x|), %.3e absolute, singular values %.2e relative"
          % (len(gold["cases"]), worst_ulps, worst_abs, worst_sv))


def test_degenerate_cases_are_flagged_and_finite(dev, gold):
    for c in gold["degenerate_cases"]:
        out, status, sv = run(gold, c, dev, return_sv=True)
        assert ((status & ops.POSE_SYNC_RANK) != 0).all(), (c, status.tolist())
        assert ((status & (ops.POSE_SYNC_MASS | ops.POSE_SYNC_NONFINITE)) == 0).all(), (c, status.tolist())
        assert torch.isfinite(out).all() and torch.isfinite(sv).all(), c
        R = out[:, :, :3, :3].double()
        assert (R @ R.transpose(-1, -2) - torch.eye(3, dtype=torch.float64, device=dev)).abs().max().item() < 1e-6      # still rotations
        assert ((sv[..., 2] / sv[..., 0]).min(dim=1).values < 1e-6).all()
        # a tolerance below the ratio accepts the same data: the bit is the comparison, nothing else
        _, loose = run(gold, c, dev, rank_tol=0.0)
        assert ((loose & ops.POSE_SYNC_RANK) == 0).all()


def test_nan_flags_its_element_alone(dev, gold):
    c = "n5_all_mid_s002"
    P, conf, pairs, N, squares, _ = case_inputs(gold, c)
    clean, st0 = ops.pose_sync(torch.from_numpy(P).to(dev), torch.from_numpy(conf).to(dev), pairs, N, squares=squares)
    bad = P.copy()
    bad[1, 3, 1, 2] = np.nan
    out, st = ops.pose_sync(torch.from_numpy(bad).to(dev), torch.from_numpy(conf).to(dev), pairs, N, squares=squares)
    assert st0.tolist() == [0, 0, 0]
    assert st[1].item() & ops.POSE_SYNC_NONFINITE and st[0].item() == 0 and st[2].item() == 0
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
    cbad = conf.copy()
    cbad[2, 0] = np.inf
    out, st = ops.pose_sync(torch.from_numpy(P).to(dev), torch.from_numpy(cbad).to(dev), pairs, N, squares=squares)
    assert st[2].item() & ops.POSE_SYNC_NONFINITE and st[0].item() == 0 and st[1].item() == 0
    assert torch.equal(out[0], clean[0]) and torch.equal(out[1], clean[1])


def test_no_mass_is_flagged(dev, gold):
    """One squaring of a five-view chain cannot carry mass from view 0 to view 4 (two steps reach view 2): the reference's assertion
    "2**squares, or the set of edges, is too small"."""
    c = "n5_chain_first_s002"
    P, conf, _, N, _, _ = case_inputs(gold, c)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4)]
    out, st = ops.pose_sync(torch.from_numpy(P[:, :4].copy()).to(dev), torch.from_numpy(conf[:, :4].copy()).to(dev), pairs, N, squares=1,
                            center_first_camera=True)
    assert ((st & ops.POSE_SYNC_MASS) != 0).all() and torch.isfinite(out).all()


def test_bitwise_reproducible_and_batch_independent(dev, gold):
    for c in ("n8_all_mid_s005", "n3_all_mid_s002", "deg_n5"):
        P, conf, pairs, N, squares, _ = case_inputs(gold, c)
        Pd, cd = torch.from_numpy(P).to(dev), torch.from_numpy(conf).to(dev)
        a = ops.pose_sync(Pd, cd, pairs, N, squares=squares, return_sv=True)
        b = ops.pose_sync(Pd, cd, pairs, N, squares=squares, return_sv=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y), c
        for i in range(P.shape[0]):
            one = ops.pose_sync(Pd[i:i + 1].contiguous(), cd[i:i + 1].contiguous(), pairs, N, squares=squares, return_sv=True)
            for x, y in zip(a, one):
                assert torch.equal(x[i:i + 1], y), (c, i)


def test_graph_capture_replays_to_the_eager_result(dev, gold):
    P, conf, pairs, N, squares, _ = case_inputs(gold, "n5_all_first_s005")
    Pd, cd = torch.from_numpy(P).to(dev), torch.from_numpy(conf).to(dev)
    eager = ops.pose_sync(Pd, cd, pairs, N, squares=squares, center_first_camera=True, return_sv=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.pose_sync(Pd, cd, pairs, N, squares=squares, center_first_camera=True, return_sv=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.pose_sync(Pd, cd, pairs, N, squares=squares, center_first_camera=True, return_sv=True)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert torch.equal(x, y)


def test_wrapper_refusals_on_the_device(dev, gold):
    P, conf, pairs, N, _, _ = case_inputs(gold, "n3_all_mid_s000")
    Pd, cd = torch.from_numpy(P).to(dev), torch.from_numpy(conf).to(dev)
    with pytest.raises(TypeError):
        ops.pose_sync(Pd.double(), cd, pairs, N)
    with pytest.raises(ValueError):
        ops.pose_sync(Pd[:, :2].contiguous(), cd, pairs, N)
    with pytest.raises(ValueError, match="pairs for"):
        ops.pose_sync(Pd[:, :2].contiguous(), cd[:, :2].contiguous(), pairs, N)
    with pytest.raises(RuntimeError, match="squares"):
        ops.pose_sync(Pd, cd, pairs, N, squares=17)
    assert ops.pose_sync_pairs(pairs, N, dev) is ops.pose_sync_pairs(list(pairs), N, dev)          # the device copy is cached per pair list
