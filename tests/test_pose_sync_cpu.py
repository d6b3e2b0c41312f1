"""CPU: the yardsticks and the host side of the camera synchronisation and of the evaluation protocol's small functions.

  - `sync_ref`, a float64 numpy restatement of utils/sync_utils.py:camera_synchronization (so3_projection, normalize_confidences), reproduces
    the reference's float64 evaluation (tests/golden/pose_sync.npz `out_f64`) within 2 float32 ulps of max(1, |x|): both sides are float64
    arithmetic rounded once to float32, so they may differ where a value sits next to a rounding boundary, and by nothing else. The GPU tests
    import it;
  - forge_pose_sync's argument codes (fake pointers: every refusal happens before any launch);
  - ops.pose_sync's pair-list checks (the reference's assertions) and its refusal of host tensors;
  - evaluation.permute_clips / compute_pose_metric against the reference's own results (tests/golden/eval_protocol.npz).
"""
import ctypes

import numpy as np
import pytest
import torch

from forge_amd import _lib, ops


def ulp32(x):
    """float32 spacing at max(1, |x|), as float64."""
    return np.spacing(np.maximum(1.0, np.abs(x)).astype(np.float32)).astype(np.float64)


def sync_ref(P, conf, pairs, N, squares=10, center=None, project=True):
    """float64 restatement: P [B, E, 4, 4], conf [B, E], pairs [(i, j)] -> (out [B, N, 4, 4] float64, sv [B, N, 3], mass [B, N])."""
    P, conf = np.asarray(P, np.float64), np.asarray(conf, np.float64)
    B = P.shape[0]
    center = N // 2 if center is None else center
    c = np.zeros((B, N, N))
    for e, (i, j) in enumerate(pairs):
        c[:, i, j] = conf[:, e]
        c[:, j, i] = conf[:, e]
        c[:, i, i] += conf[:, e] / 2
        c[:, j, j] += conf[:, e] / 2
    c = c / np.maximum(c.sum(axis=1, keepdims=True), 1e-9)
    L = np.zeros((B, 4 * N, 4 * N))
    for i in range(N):
        L[:, 4 * i:4 * i + 4, 4 * i:4 * i + 4] = c[:, i, i, None, None] * np.eye(4)
    for e, (i, j) in enumerate(pairs):
        p = P[:, e]
        inv = p.copy()
        inv[:, :3, :3] = p[:, :3, :3].transpose(0, 2, 1)
        inv[:, :3, 3:] = -inv[:, :3, :3] @ p[:, :3, 3:]
        L[:, 4 * i:4 * i + 4, 4 * j:4 * j + 4] = c[:, i, j, None, None] * inv
        L[:, 4 * j:4 * j + 4, 4 * i:4 * i + 4] = c[:, j, i, None, None] * p
    for _ in range(squares):
        L = L @ L
    L = L.reshape(B, N, 4, N, 4)[:, :, :, center, :]
    mass = L[:, :, 3, 3].copy()
    L = L / np.maximum(L[:, :, 3:, 3:], 1e-9)
    U, S, Vt = np.linalg.svd(L[:, :, :3, :3])
    if project:
        d = np.linalg.det(U @ Vt)
        U = U.copy()
        U[..., :, 2] *= d[..., None]
        L = L.copy()
        L[:, :, :3, :3] = U @ Vt
    return L, S, mass


def case_inputs(g, c):
    N, squares, first = (int(v) for v in g[c + "__meta"])
    return g[c + "__P"], g[c + "__conf"], [tuple(int(v) for v in p) for p in g[c + "__pairs"]], N, squares, (0 if first else N // 2)


def test_restatement_reproduces_the_reference_float64(golden):
    g = golden("pose_sync")
    assert len(g["cases"]) >= 18 and len(g["degenerate_cases"]) == 2
    worst = 0.0
    for c in g["cases"]:
        P, conf, pairs, N, squares, center = case_inputs(g, c)
        out, sv, mass = sync_ref(P, conf, pairs, N, squares, center)
        ref = g[c + "__out_f64"].astype(np.float64)
        got = out.astype(np.float32).astype(np.float64)                           # float64 rounded once, as the reference's result is
        r = (np.abs(got - ref) / ulp32(ref)).max()
        worst = max(worst, r)
        assert r <= 2.0, (c, r)
        assert (mass > 0).all()
        assert (np.abs(sv - g[c + "__sv"]) <= 1e-9 * g[c + "__sv"]).all(), c
        assert (sv[..., 2] / sv[..., 0]).min() >= 1e-2, c                         # what the generator asserted
        # the reference's own float32-built evaluation sits 1e-6 .. 5e-5 away: the reason float64 is the yardstick
        assert np.abs(g[c + "__out_f32"].astype(np.float64) - ref).max() < 1e-3, c
    print("restatement against out_f64: worst %.2f float32 ulps" % worst)
    for c in g["degenerate_cases"]:
        P, conf, pairs, N, squares, center = case_inputs(g, c)
        _, sv, _ = sync_ref(P, conf, pairs, N, squares, center)
        assert ((sv[..., 2] / sv[..., 0]).min(axis=1) < 1e-9).all(), c


FAKE = ctypes.c_void_p(4096)


@pytest.mark.parametrize("kw, code", [
    ({"N": 2, "E": 1}, -2), ({"N": 9, "E": 8}, -2), ({"E": 3}, -2), ({"E": 11}, -2),
    ({"squares": 0}, -1), ({"squares": 17}, -1), ({"center": 5}, -1), ({"center": -1}, -1), ({"B": 0}, -1), ({"rank_tol": -1.0}, -1),
    ({"rank_tol": float("nan")}, -1), ({"P": None}, -1), ({"pairs": None}, -1), ({"status": None}, -1),
])
def test_argument_codes(built_lib, kw, code):
    a = dict(P=FAKE, conf=FAKE, pairs=FAKE, B=1, N=5, E=10, squares=10, center=2, rank_tol=1e-6, out=FAKE, sv=None, status=FAKE)
    a.update(kw)
    lib = _lib.lib()
    rc = lib.forge_pose_sync(a["P"], a["conf"], a["pairs"], a["B"], a["N"], a["E"], a["squares"], a["center"], a["rank_tol"], a["out"], a["sv"],
                             a["status"], None)
    assert rc == code, (kw, rc, lib.forge_last_error())
    assert b"forge_pose_sync" in lib.forge_last_error()


@pytest.mark.parametrize("pairs, N, what", [
    ([(0, 1), (1, 1), (1, 2)], 3, "itself"),
    ([(0, 1), (1, 3)], 3, "outside"),
    ([(0, 1), (1, 2), (1, 0)], 3, "twice"),
    ([(0, 1), (1, 2), (0, 1)], 3, "twice"),
    ([(0, 1), (1, 2), (0, 2)], 4, "view 3"),
    ([(0, 1)], 2, "N=2"),
    ([(0, 1)], 9, "N=9"),
])
def test_pair_list_errors(pairs, N, what):
    with pytest.raises(ValueError, match=what):
        ops.pose_sync_pairs(pairs, N)


def test_pair_list_accepted_and_host_tensors_refused():
    assert ops.pose_sync_pairs([(0, 1), (2, 1)], 3) == ((0, 1), (2, 1))
    P, conf = torch.eye(4).repeat(1, 2, 1, 1), torch.ones(1, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_sync(P, conf, [(0, 1), (1, 2)], 3)


# ----------------------------------------------------------------------------------------------------------------- evaluation protocol
@pytest.fixture(scope="module")
def scene(golden):
    from make_golden_eval_protocol import eval_sample
    return eval_sample(golden("eval_protocol"))                 # the golden's own camera matrices, images from seeds


def test_permute_clips_matches_the_reference(golden, scene):
    from forge_amd import evaluation as ev
    g = golden("eval_protocol")
    clips, gt, extr = scene["images"][:, :5], scene["cam_poses_rel_cv2"][:, :5], scene["cam_extrinsics_cv2_canonicalized"]
    for k in range(5):
        perm = [int(v) for v in g["perms"][k]]
        c, p, e, pm = ev.permute_clips(clips, gt, extr, k, return_permutation=True)
        assert pm == perm == ev.permutation(k, 5)
        assert torch.equal(c, clips[:, perm]) and torch.equal(ev.permute_clips(clips, None, None, k, clips_only=True), c)
        assert p.shape == (1, 5, 4, 4) and e.shape == (1, 10, 4, 4)
        for got, name in ((p[0], "gt_poses"), (e[0], "nvs_extr")):
            r32, r64 = g[name + "32"][k], g[name + "64"][k]
            # float32 inputs: within 4 x the reference's own float32-against-float64 distance (+ 2 ulps: that distance can be 0)
            bound = 4 * np.abs(r32 - r64).max() + 2 * ulp32(r64)
            assert (np.abs(got.double().numpy() - r64) <= bound).all(), (k, name)
        # float64 inputs: float64 arithmetic against float64 arithmetic, the reference's rounded once to float32 by its float32 buffers
        _, p64, e64 = ev.permute_clips(clips.double(), gt.double(), extr.double(), k)
        for got, name in ((p64[0], "gt_poses"), (e64[0], "nvs_extr")):
            r64 = g[name + "64"][k]
            assert (np.abs(got.numpy().astype(np.float32).astype(np.float64) - r64) <= 2 * ulp32(r64)).all(), (k, name)


def test_compute_pose_metric_matches_the_reference(golden):
    from forge_amd import evaluation as ev
    g = golden("eval_protocol")
    pred, gt = torch.from_numpy(g["metric_pred"]), torch.from_numpy(g["metric_gt"])
    th64, t64, th32, t32 = g["metric_theta64"], g["metric_t64"], g["metric_theta32"], g["metric_t32"]
    th, t = ev.compute_pose_metric(pred.double(), gt.double())                       # batched, float64: the same arithmetic
    assert th.shape == (8,) and np.allclose(th.numpy()[:7], th64[:7], rtol=1e-12, atol=1e-12) and np.allclose(t.numpy(), t64, rtol=1e-12)
    th_f, t_f = ev.compute_pose_metric(pred, gt)                                     # float32: within 4 x the reference's own float32 error
    assert (np.abs(th_f.double().numpy()[:7] - th64[:7]) <= 4 * np.abs(th32[:7] - th64[:7]).max() + 1e-12).all()
    assert (np.abs(t_f.double().numpy() - t64) <= 4 * np.abs(t32 - t64).max() + 1e-12).all()
    # the documented deviation: a dot product above 1 (unnormalised quaternions) is clamped; the reference returns NaN
    assert np.isnan(th64[7]) and np.isnan(th32[7])
    assert th[7].item() == 0.0 and th_f[7].item() == 0.0
    one, _ = ev.compute_pose_metric(pred[3], gt[3])                                  # a single pair, as the reference takes it
    assert one.dim() == 0 and one.item() == th_f[3].item()
