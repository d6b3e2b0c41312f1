"""Goldens of the evaluation protocol from the reference's OWN functions (kubric_eval.py, utils/sync_utils.py, utils/eval_utils.py), CPU only.

Imports the reference through oracle/ref_import.py (unchanged) and writes

tests/golden/pose_sync.npz - utils/sync_utils.py:camera_synchronization. Per case `<c>` (N views, B = 3 scenes, edge set, noise, centre):
  <c>__meta              [N, squares, center_first_camera]
  <c>__pairs             [E, 2] (i, j)
  <c>__P, <c>__conf      float32 [B, E, 4, 4] / [B, E]: consistent pairwise extrinsics P_j P_i^-1 of random cameras, disturbed by a rotation of
                         noise x N(0, 1) rad about each axis and a translation of noise x N(0, 1); confidences uniform in [0.5, 1]
  <c>__out_f32           the reference function as called (so3_projection, normalize_confidences, double: its defaults)
  <c>__out_f64           the same function fed the same inputs as float64 (its result is float64 arithmetic rounded once to float32)
  <c>__sv                float64 [B, N, 3]: singular values of the rotation blocks of a so3_projection=False float64 run whose final
                         `.float()` is suppressed (the inputs are a Tensor subclass whose float() is the identity: float32 blocks would
                         limit the singular values to 1e-7)
  Conditioned cases: sigma_min / sigma_max >= 1e-2 for every view is ASSERTED; a seed that fails is replaced by the next one, never a case.
  Degenerate cases (`deg_*`, noise 0.5): sigma_min / sigma_max < 1e-9 for some view of every scene is asserted; inputs only.

tests/golden/eval_protocol.npz - see eval_protocol_goldens().

    python tools/make_golden_eval_protocol.py [pose_sync|eval_protocol]      (needs the reference tree; a minute on a CPU)
"""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

GOLDEN = os.path.join(ROOT, "tests", "golden")
B = 3
SQUARES = 10
NOISES = (0.0, 0.02, 0.05)


class _Keep64(torch.Tensor):
    """float64 tensor whose .float() is the identity: camera_synchronization's closing `L = L.float()` then returns its float64 result."""

    def float(self):
        return self


def _rotvec(v):
    """Rodrigues: [..., 3] rotation vectors -> [..., 3, 3], float64."""
    th = v.norm(dim=-1, keepdim=True).clamp(min=1e-300)
    k = v / th
    K = torch.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    s, c = th.sin()[..., None], th.cos()[..., None]
    return torch.eye(3, dtype=v.dtype) + s * K + (1 - c) * (K @ K)


def _se3(R, t):
    P = torch.zeros(R.shape[:-2] + (4, 4), dtype=R.dtype)
    P[..., :3, :3], P[..., :3, 3], P[..., 3, 3] = R, t, 1.0
    return P


def edge_sets(N):
    sets = {"all": list(itertools.combinations(range(N), 2))}
    if N == 5:
        sets["chain"] = [(i, i + 1) for i in range(N - 1)] + [(0, 3)]      # a spanning chain with one extra edge
    return sets


def problem(N, pairs, noise, seed):
    """float32 (P [B, E, 4, 4], conf [B, E]) of a seeded synchronisation problem."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    cams = _se3(_rotvec(rn(B, N, 3)), rn(B, N, 3))                         # world -> camera extrinsics of the N views
    P = torch.stack([cams[:, j] @ torch.linalg.inv(cams[:, i]) for i, j in pairs], dim=1)
    E = len(pairs)
    dist = _se3(_rotvec(noise * rn(B, E, 3)), noise * rn(B, E, 3)) if noise > 0 else _se3(_rotvec(torch.zeros(B, E, 3, dtype=torch.float64)),
                                                                                          torch.zeros(B, E, 3, dtype=torch.float64))
    conf = 0.5 + 0.5 * torch.rand(B, E, generator=g, dtype=torch.float64)
    return (dist @ P).float(), conf.float()


def run_reference(sync_utils, P, conf, pairs, N, center_first, so3=True):
    Ps = {p: P[:, e] for e, p in enumerate(pairs)}
    cf = {p: conf[:, e] for e, p in enumerate(pairs)}
    return sync_utils.camera_synchronization(Ps, cf, N, squares=SQUARES, so3_projection=so3, center_first_camera=center_first)


def singular_values(sync_utils, P, conf, pairs, N, center_first):
    """float64 [B, N, 3] of the unprojected rotation blocks (float64 arithmetic throughout, no closing rounding)."""
    L = run_reference(sync_utils, P.double().as_subclass(_Keep64), conf.double().as_subclass(_Keep64), pairs, N, center_first, so3=False)
    L = L.as_subclass(torch.Tensor)
    assert L.dtype == torch.float64
    return torch.linalg.svdvals(L[:, :, :3, :3])


def pose_sync_goldens(sync_utils):
    out, names, deg_names = {}, [], []
    cases = []
    for N in (3, 5, 8):
        for ename, pairs in edge_sets(N).items():
            for center_first in ((False, True) if N == 5 else (False,)):
                for noise in NOISES:
                    cases.append((N, ename, pairs, center_first, noise))
    for N, ename, pairs, center_first, noise in cases:
        name = "n%d_%s_%s_s%03d" % (N, ename, "first" if center_first else "mid", round(noise * 100))
        for seed in range(100 * N, 100 * N + 50):
            P, conf = problem(N, pairs, noise, seed)
            sv = singular_values(sync_utils, P, conf, pairs, N, center_first)
            ratio = (sv[..., 2] / sv[..., 0]).min().item()
            if ratio >= 1e-2:
                break
            print("  %s: seed %d gives sigma_min / sigma_max = %.3g, next seed" % (name, seed, ratio))
        else:
            raise AssertionError("%s: no seed gives a conditioned problem" % name)
        o32 = run_reference(sync_utils, P, conf, pairs, N, center_first)
        o64 = run_reference(sync_utils, P.double(), conf.double(), pairs, N, center_first)
        assert o32.dtype == torch.float32 and o64.dtype == torch.float32 and o32.shape == (B, N, 4, 4)
        dev = (o32.double() - o64.double()).abs().max().item()
        print("  %s: seed %d, E %d, sigma ratio %.3g, |out_f32 - out_f64| %.3g" % (name, seed, len(pairs), ratio, dev))
        names.append(name)
        out.update({name + "__meta": np.array([N, SQUARES, int(center_first)]), name + "__pairs": np.array(pairs, dtype=np.int32),
                    name + "__seed": np.array(seed), name + "__P": P.numpy(), name + "__conf": conf.numpy(), name + "__out_f32": o32.numpy(),
                    name + "__out_f64": o64.numpy(), name + "__sv": sv.numpy()})
    for N in (3, 5):
        pairs = edge_sets(N)["all"]
        name = "deg_n%d" % N
        for seed in range(1000 * N, 1000 * N + 50):
            P, conf = problem(N, pairs, 0.5, seed)
            sv = singular_values(sync_utils, P, conf, pairs, N, False)
            ratio = (sv[..., 2] / sv[..., 0]).min(dim=1).values           # per scene: its worst view
            if ratio.max().item() < 1e-9:
                break
            print("  %s: seed %d gives a worst-view ratio of %.3g in some scene, next seed" % (name, seed, ratio.max().item()))
        else:
            raise AssertionError("%s: no seed gives a degenerate problem in every scene" % name)
        print("  %s: seed %d, worst-view sigma ratios %s" % (name, seed, ratio.tolist()))
        deg_names.append(name)
        out.update({name + "__meta": np.array([N, SQUARES, 0]), name + "__pairs": np.array(pairs, dtype=np.int32), name + "__seed": np.array(seed),
                    name + "__P": P.numpy(), name + "__conf": conf.numpy()})
    out["cases"] = np.array(names)
    out["degenerate_cases"] = np.array(deg_names)
    save("pose_sync", out)


SAMPLE_SEED, DEPTH_SEED, METRIC_SEED = 12, 5, 11
POSE_NOISE = 0.02
DEPTH_EPS = 1e-3
SYNC_BEST = 2


class _Wrapped:
    """What kubric_eval.py's functions take: an object with `.module` (the reference wraps its model in DataParallel)."""

    def __init__(self, module):
        self.module = module


class _FreshSample(dict):
    """A sample whose entries are handed out as copies, as `.to(device)` hands them out when the sample lives on the host and the model on
    a GPU - the reference's setting. On one device `.to()` is the identity and the renderer's in-place halving of K
    (models/volume_render.py:50-51) would reach the sample: every later evaluate would see other intrinsics."""

    def __getitem__(self, k):
        return dict.__getitem__(self, k).clone()


# utils/eval_utils.py:53-56: permute_clips re-canonicalises the novel cameras on a canonical camera 4 units from the object, whatever
# render.camera_z says. In the stock synthetic scene (cameras 1.5 units away, rays sampled between 0.5 and 2) every novel camera it hands to
# evaluate would sit beyond max_depth and render nothing. The protocol's scene is therefore the stock scene at that distance: cameras,
# canonical camera and depth range 4 units out, where the reference's protocol is consistent with itself.
EVAL_CAMERA_Z = 4.0
EVAL_DEPTH_RANGE = (3.25, 4.75)


CAMERA_KEYS = ("cam_poses_rel_cv2", "cam_poses_cv2_canonicalized", "cam_extrinsics_cv2_canonicalized", "K_cv2")


def scene_cameras():
    """The cameras of synthetic.make_sample(1, 10, 256, EVAL_CAMERA_Z, seed=SAMPLE_SEED) (the same orbit, elevations and seeded jitter), built
    in float64 with closed-form inverses (R^T, -R^T t) and rounded once to float32. make_sample itself inverts its matrices with float32
    torch.inverse, an LU whose last bits depend on the host and which leaves 1e-8 in the last row; the protocol's goldens compare poses
    at the float32 ulp, so their cameras must not."""
    from forge_amd import synthetic as syn
    g = torch.Generator().manual_seed(SAMPLE_SEED)
    jit = ((torch.rand(10, 2, generator=g) - 0.5) * 0.2).double().numpy()          # make_sample's first draw

    def rot(axis, a):
        c, s_ = np.cos(a), np.sin(a)
        m = np.eye(4)
        if axis == "y":
            m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s_, -s_, c
        else:
            m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, -s_, s_, c
        return m

    def shift(z):
        m = np.eye(4)
        m[2, 3] = z
        return m

    def inv(m):
        o = np.eye(4)
        o[:3, :3] = m[:3, :3].T
        o[:3, 3] = -m[:3, :3].T @ m[:3, 3]
        return o
    rel = []
    for i in range(10):
        az = np.radians(72.0 * i if i < 5 else 36.0 + 72.0 * (i - 5))
        el = np.radians(10.0 * ((i % 3) - 1))
        R = rot("y", az) @ rot("x", el)
        if i > 0:
            R = R @ rot("y", float(jit[i, 0])) @ rot("x", float(jit[i, 1]))
        rel.append(shift(EVAL_CAMERA_Z) @ R @ shift(-EVAL_CAMERA_Z))
    rel[0] = np.eye(4)
    poses = [shift(-EVAL_CAMERA_Z) @ r for r in rel]
    f32 = lambda ms: torch.from_numpy(np.stack(ms)).float()[None].contiguous()
    return {"cam_poses_rel_cv2": f32(rel), "cam_poses_cv2_canonicalized": f32(poses), "cam_extrinsics_cv2_canonicalized": f32([inv(m) for m in poses]),
            "K_cv2": syn.intrinsics(256)[None, None].repeat(1, 10, 1, 1).contiguous()}


def eval_sample(cameras=None):
    """The synthetic scene of the protocol goldens: synthetic.make_sample's images and masks (10 views at 256^2, seeded), seeded depths, and
    the cameras of scene_cameras(). The golden stores those cameras (`scene__<key>`); the tests pass the loaded golden as `cameras` and get
    exactly the matrices the reference was run on, whatever their host computes."""
    from forge_amd import synthetic as syn
    s = syn.add_depths(syn.make_sample(1, 10, 256, EVAL_CAMERA_Z, seed=SAMPLE_SEED), EVAL_CAMERA_Z, seed=DEPTH_SEED)
    cams = scene_cameras() if cameras is None else {k: torch.from_numpy(np.asarray(cameras["scene__" + k])) for k in CAMERA_KEYS}
    for k in CAMERA_KEYS:
        assert cams[k].shape == s[k].shape and cams[k].dtype == torch.float32 and (cams[k] - s[k]).abs().max().item() < 1e-5, k
        s[k] = cams[k].clone()
    return s


def eval_dataset():
    from forge_amd import synthetic as syn
    return syn.SyntheticDataset(EVAL_CAMERA_Z)


def eval_config(kubric_config):
    """The joint model's config for the protocol's scene; kubric_config: forge_amd.synthetic's or oracle/ref_import's (the same keys)."""
    return kubric_config(use_gt_pose=False, parameter="joint", min_depth=EVAL_DEPTH_RANGE[0], max_depth=EVAL_DEPTH_RANGE[1])


def constructed_poses(gt_poses, mat2quat, seed):
    """Poses a trained model could have predicted: the ground-truth relative poses of every canonical choice (gt_poses [5, 5, 4, 4],
    permuted) as quaternion + translation, disturbed by POSE_NOISE x N(0, 1) per component, quaternion renormalised. float32 [5, 4, 7]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(gt_poses.shape[0]):
        p = mat2quat(gt_poses[k, 1:].double()).float() + POSE_NOISE * torch.randn(4, 7, generator=g, dtype=torch.float32)
        out.append(torch.cat([torch.nn.functional.normalize(p[:, :4]), p[:, 4:]], dim=1))
    return torch.stack(out)


def eval_protocol_goldens(mods, keval):
    """tests/golden/eval_protocol.npz - kubric_eval.py's own predict_initial, evaluate, evaluate_all and sync_pose, and utils/eval_utils.py's
    permute_clips / compute_pose_metric, on the joint model and synthetic sample that oracle/make_golden.py:joint_goldens uses (seeded, neither
    stored), in float32 (`*32`) and with model, sample and the reference's own literals in float64 (`*64`: make_golden.to_float64 and
    torch.set_default_dtype, as oracle/make_golden.py runs its float64 yardsticks):
      perms [5, 5]; gt_poses32/64 [5, 5, 4, 4], nvs_extr32/64 [5, 10, 4, 4]      permute_clips per canonical id
      poses32/64 [5, 4, 7]                                                      predict_initial's poses_cam per canonical id
      given_poses [5, 4, 7]                                                     constructed_poses: what evaluate / sync_pose are fed
      errors32/64 [5, 3]                                                        evaluate per canonical id: rot, trans, depth error
      depth_sensitivity, depth_eps                                              max change of a depth error when every component of the
                                                                                given poses moves by +-depth_eps, over depth_eps
      all32/64 [4]                                                              evaluate_all: best id, rot, trans, depth error
      sync_*                                                                    sync_pose on the same poses with best id SYNC_BEST: the
                                                                                Ps / confidences it hands to camera_synchronization, that
                                                                                function's result (sync_L) and its own (sync_out)
      metric_*                                                                  compute_pose_metric on random pose pairs (float32 / float64
                                                                                inputs) and on an unnormalised pair whose dot product is > 1
    A randomly initialised model predicts poses more than 50 degrees off: all five capped rotation errors are equal and the synchronisation
    of those poses is rank-deficient. Its predictions pin predict_initial only; evaluate, evaluate_all and sync_pose are run on
    predict_initial's dict with `poses_cam` replaced by the constructed poses. The image metrics inside evaluate (skimage, lpips: not
    installed, pinned by goldens of their own) and the plots are replaced by stubs.
    Asserted: the best and the second-best rotation error differ by at least 100 x the float32-against-float64 deviation of the predicted
    poses, and both precisions choose the same id; otherwise the next pose seed is taken."""
    import types

    import make_golden as mg
    from forge_amd import synthetic as syn
    eu, su, gu = keval.eval_utils, keval.sync_utils, mods["utils.geo_utils"]
    keval.vis_utils = types.SimpleNamespace(vis_seq=lambda **kw: None)
    eu.compute_img_metric = lambda rgb, gt: (0.0, 0.0)
    lpips_stub = lambda a, b: torch.zeros(a.shape[0])
    ds = eval_dataset()
    weight_seed = 0
    out = {"sample_seed": np.array(SAMPLE_SEED), "depth_seed": np.array(DEPTH_SEED), "weight_seed": np.array(weight_seed)}

    def scores(model, sample, dataset, rd, given, tag):
        sample = _FreshSample(sample)
        dt = rd["0"]["poses_cam"].dtype
        rows = []
        with torch.no_grad():
            for k in range(5):
                r = rd[str(k)]
                r["poses_cam"] = given[k].to(dt)
                r["nvs_extr"], r["gt_poses"] = r["nvs_extr"].to(dt), r["gt_poses"].to(dt)
                res = keval.evaluate(model, lpips_stub, sample, dataset, r["poses_cam"], r["features_raw"], r["nvs_extr"], r["gt_poses"], 0, k,
                                     "cpu", None, "before")
                rows.append([float(v) for v in res[3:]])
            best = keval.evaluate_all(model, lpips_stub, sample, dataset, rd, 0, "cpu", None)
        rows = np.array(rows)
        assert [float(best[4]), float(best[5])] == list(rows[int(best[0]), :2]) and float(best[6]) == rows[4, 2]
        print("  %s: rot %s trans %s depth %s best %s" % (tag, rows[:, 0], rows[:, 1], rows[:, 2], best[0]), flush=True)
        return rows, np.array([float(best[0]), float(best[4]), float(best[5]), float(best[6])])

    jm = mods["models.model"].FORGE(ref_import_config()).eval()
    jm.load_state_dict(syn.seeded_state_dict(jm.state_dict(), weight_seed))
    sample = eval_sample()
    out.update({"scene__" + k: sample[k].numpy() for k in CAMERA_KEYS})
    with torch.no_grad():
        rd32 = keval.predict_initial(_Wrapped(jm), _FreshSample(sample), "cpu")
    jm64, sample64 = mg.to_float64(jm, sample)
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            rd64 = keval.predict_initial(_Wrapped(jm64), _FreshSample(sample64), "cpu")
    finally:
        torch.set_default_dtype(torch.float32)
    poses32 = torch.stack([rd32[str(k)]["poses_cam"] for k in range(5)])
    poses64 = torch.stack([rd64[str(k)]["poses_cam"] for k in range(5)])
    assert poses32.dtype == torch.float32 and poses64.dtype == torch.float64
    dev = (poses32.double() - poses64).abs().max().item()
    print("  predict_initial: |poses32 - poses64| %.3g" % dev)
    out["perms"] = np.array([rd32[str(k)]["permutation"] for k in range(5)])
    for tag, rd in (("32", rd32), ("64", rd64)):
        out["gt_poses" + tag] = torch.cat([rd[str(k)]["gt_poses"] for k in range(5)]).double().numpy()
        out["nvs_extr" + tag] = torch.cat([rd[str(k)]["nvs_extr"] for k in range(5)]).double().numpy()
    gt = torch.from_numpy(out["gt_poses64"])              # float64 arithmetic: the constructed poses do not inherit a float32 run's noise
    for pose_seed in range(7, 27):
        cp = constructed_poses(gt, gu.mat2quat, pose_seed)
        # the float32 model again: to_float64 converted jm in place
        jm32 = mods["models.model"].FORGE(ref_import_config()).eval()
        jm32.load_state_dict(syn.seeded_state_dict(jm32.state_dict(), weight_seed))
        rows32, all32 = scores(_Wrapped(jm32), sample, ds, rd32, cp, "float32")
        torch.set_default_dtype(torch.float64)
        try:
            rows64, all64 = scores(_Wrapped(jm64), sample64, mg._Dataset64(ds), rd64, cp, "float64")
        finally:
            torch.set_default_dtype(torch.float32)
        assert np.ptp(rows64[:, 2]) > 1e-4, "the novel views render nothing: every depth error is the mean depth"
        rot = np.sort(rows64[:, 0])
        print("  pose seed %d: best rot %.6f, second %.6f, best id %d / %d" % (pose_seed, rot[0], rot[1], all32[0], all64[0]))
        if rot[1] - rot[0] >= 100 * dev and all32[0] == all64[0]:
            break
        print("  pose seed %d: the best canonical id is not separated by 100 x the pose deviation, next seed" % pose_seed)
    else:
        raise AssertionError("no pose seed separates the best canonical id")
    # how far a pose deviation moves the depth error: the reference's own figure at poses moved by +-DEPTH_EPS in every component
    g = torch.Generator().manual_seed(pose_seed)
    moved = cp + DEPTH_EPS * (2.0 * torch.randint(0, 2, cp.shape, generator=g) - 1.0)
    moved = torch.cat([torch.nn.functional.normalize(moved[..., :4], dim=-1), moved[..., 4:]], dim=-1)
    rows_moved, _ = scores(_Wrapped(jm32), sample, ds, rd32, moved, "float32, poses moved")
    out["depth_sensitivity"] = np.array(np.abs(rows_moved[:, 2] - rows32[:, 2]).max() / DEPTH_EPS)
    out["depth_eps"] = np.array(DEPTH_EPS)
    print("  depth error moves by %.3g per unit of pose deviation" % out["depth_sensitivity"])
    out.update({"poses32": poses32.numpy(), "poses64": poses64.numpy(), "given_poses": cp.numpy(), "pose_seed": np.array(pose_seed),
                "errors32": rows32, "errors64": rows64, "all32": all32, "all64": all64})

    # ---- sync_pose on a constructed return_dict
    seen = {}
    real = su.camera_synchronization

    def spy(Ps, confidence, **kw):
        res = real(Ps, confidence, **kw)
        seen.update({"Ps": Ps, "conf": confidence, "kw": kw, "res": res})
        return res
    keval.sync_utils = types.SimpleNamespace(camera_synchronization=spy)
    try:
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            rd = {str(k): {"poses_cam": cp[k].to(dt), "permutation": [int(v) for v in out["perms"][k]]} for k in range(5)}
            torch.set_default_dtype(dt)
            try:
                res = keval.sync_pose(rd, SYNC_BEST, "cpu")
            finally:
                torch.set_default_dtype(torch.float32)
            pairs = list(seen["Ps"].keys())
            assert seen["kw"] == {"N": 5, "squares": 10, "center_first_camera": True}
            out["sync_out" + tag] = res.double().numpy()
            out["sync_P" + tag] = torch.stack([seen["Ps"][p][0] for p in pairs]).double().numpy()
            out["sync_conf" + tag] = torch.stack([torch.as_tensor(seen["conf"][p]).reshape(()) for p in pairs]).double().numpy()
            out["sync_L" + tag] = seen["res"][0].double().numpy()
    finally:
        keval.sync_utils = su
    out.update({"sync_best": np.array(SYNC_BEST), "sync_pairs": np.array(pairs, dtype=np.int32)})
    P = torch.from_numpy(out["sync_P32"]).float()[None]
    sv = singular_values(su, P, torch.from_numpy(out["sync_conf32"]).float()[None], pairs, 5, True)
    ratio = (sv[..., 2] / sv[..., 0]).min().item()
    assert ratio >= 1e-2, "the constructed synchronisation problem is not conditioned: %.3g" % ratio
    print("  sync_pose: sigma ratio %.3g, |out32 - out64| %.3g" % (ratio, np.abs(out["sync_out32"] - out["sync_out64"]).max()))

    # ---- compute_pose_metric
    g = torch.Generator().manual_seed(METRIC_SEED)
    pred, gtq = torch.randn(8, 7, generator=g), torch.randn(8, 7, generator=g)
    pred[:, :4], gtq[:, :4] = torch.nn.functional.normalize(pred[:, :4]), torch.nn.functional.normalize(gtq[:, :4])
    pred[7], gtq[7] = torch.tensor([1.25, 0.5, 0.0, 0.0, 0.1, 0.2, 0.3]), torch.tensor([1.25, 0.5, 0.0, 0.0, 0.3, 0.2, 0.1])     # dot 1.8125 > 1
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        with np.errstate(invalid="ignore"):
            res = [eu.compute_pose_metric(pred[i].to(dt), gtq[i].to(dt)) for i in range(8)]
        out["metric_theta" + tag] = np.array([float(r[0]) for r in res])
        out["metric_t" + tag] = np.array([float(r[1]) for r in res])
    assert np.isnan(out["metric_theta64"][7]) and not np.isnan(out["metric_theta64"][:7]).any()
    out.update({"metric_pred": pred.numpy(), "metric_gt": gtq.numpy()})
    save("eval_protocol", out)


def ref_import_config():
    import ref_import
    return eval_config(ref_import.kubric_config)


def save(name, arrays):
    path = os.path.join(os.environ.get("FORGE_GOLDEN_OUT") or GOLDEN, name + ".npz")      # FORGE_GOLDEN_OUT: a scratch directory, to compare two runs
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in arrays.items()})
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    import ref_import
    which = sys.argv[1:] or ["pose_sync", "eval_protocol"]
    mods = ref_import.import_reference()
    keval = ref_import.import_reference_eval()
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS") or max(1, min(16, os.cpu_count() or 1))))
    if "pose_sync" in which:
        pose_sync_goldens(keval.sync_utils)
    if "eval_protocol" in which:
        eval_protocol_goldens(mods, keval)


if __name__ == "__main__":
    main()
