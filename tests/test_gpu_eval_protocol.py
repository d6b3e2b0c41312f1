"""GPU (-m gpu): forge_amd/evaluation.py against the reference's own kubric_eval.py functions (tests/golden/eval_protocol.npz, written by
tools/make_golden_eval_protocol.py from the joint model and the synthetic scene that the joint goldens use; both are rebuilt here from seeds).

The rule for everything that passes through the networks is test_gpu_parity.py's: within 4 x the reference's own float32-against-float64
deviation of its float64 evaluation. For predict_initial that deviation is max |poses32 - poses64|. evaluate and evaluate_all are fed the
golden's own `given_poses`, so no pose deviation enters: each of their figures (rotation, translation, depth error) is held to 4 x the
reference's float32-against-float64 deviation of that figure, the largest over the five canonical ids.
sync_pose is held to ops.pose_sync's bound: 2 x max |out32 - out64| + 2 float32 ulps, for its inputs and for its result.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from forge_amd import evaluation as ev
from forge_amd import metrics as fm
from forge_amd import ops
from forge_amd import synthetic as syn
from forge_amd.model import FORGE
from make_golden_eval_protocol import eval_config, eval_dataset, eval_sample
from test_pose_sync_cpu import ulp32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("eval_protocol")


@pytest.fixture(scope="module")
def scene(dev, gold):
    return {k: v.to(dev) for k, v in eval_sample(gold).items()}            # the golden's own camera matrices, images from seeds


@pytest.fixture(scope="module")
def ds():
    return eval_dataset()


@pytest.fixture(scope="module")
def model(dev, gold):
    m = FORGE(eval_config(syn.kubric_config))
    m.load_state_dict(syn.seeded_state_dict(m.state_dict(), int(gold["weight_seed"])))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def lp(dev):
    return fm.LPIPS(pretrained=False, seed=0).to(dev)


@pytest.fixture(scope="module")
def initial(model, scene, dev):
    return ev.predict_initial(model, scene, dev)


@pytest.fixture(scope="module")
def given(initial, gold, dev):
    """predict_initial's dict with the poses the golden's evaluate / sync_pose were fed (a plain dict, as a caller would build it)."""
    poses = torch.from_numpy(gold["given_poses"]).to(dev)
    return {k: dict(v, poses_cam=poses[int(k)]) for k, v in initial.items()}


def test_predict_initial_shares_one_encoder_pass(initial, gold):
    assert list(initial.keys()) == ["0", "1", "2", "3", "4"]
    base = initial["0"]["features_raw"]
    assert base.shape[:3] == (1, 5, 128)
    for k in range(5):
        r = initial[str(k)]
        perm = [int(v) for v in gold["perms"][k]]
        assert r["permutation"] == perm
        assert torch.equal(r["features_raw"][0], base[0][perm]), k          # bitwise: a gather of the one encoder pass
        assert r["poses_cam"].shape == (4, 7)
        for name in ("gt_poses", "nvs_extr"):
            r32, r64 = gold[name + "32"][k], gold[name + "64"][k]
            got = r[name][0].double().cpu().numpy()
            assert (np.abs(got - r64) <= 4 * np.abs(r32 - r64).max() + 2 * ulp32(r64)).all(), (k, name)


def test_predict_initial_poses_against_the_reference(initial, gold):
    p32, p64 = gold["poses32"].astype(np.float64), gold["poses64"]
    dev_ref = np.abs(p32 - p64).max()
    got = torch.stack([initial[str(k)]["poses_cam"] for k in range(5)]).double().cpu().numpy()
    err = np.abs(got - p64).max()
    print("predict_initial: |poses - poses64| %.3e, the reference's own float32 run %.3e" % (err, dev_ref))
    assert err <= 4 * dev_ref
    assert np.allclose(np.linalg.norm(got[..., :4], axis=-1), 1.0, atol=1e-6)


def test_predict_initial_against_five_sequential_passes(initial, model, scene, gold):
    """The parent's only way: one full pass per canonical choice through the same modules."""
    dev_ref = np.abs(gold["poses32"].astype(np.float64) - gold["poses64"]).max()
    clips = scene["images"][:, :5]
    with torch.no_grad():
        for k in range(5):
            c = ev.permute_clips(clips, None, None, k, clips_only=True)
            feats = model.encoder_3d.get_feat3D(c.reshape(5, *c.shape[2:]))
            feats = feats.reshape(1, 5, *feats.shape[1:])
            f = torch.cat([model.encoder_traj(feats, return_features=True), model.encoder_traj_2d(c, return_features=True)], dim=-1)
            p, _ = model.pose_head(f).split([model.encoder_traj.pose_dim, 1], dim=-1)
            p = torch.cat([F.normalize(p[:, :4]), p[:, 4:]], dim=1)
            err = (p.double() - initial[str(k)]["poses_cam"].double()).abs().max().item()
            print("canonical id %d: batched against sequential %.3e (bound %.3e)" % (k, err, 4 * dev_ref))
            assert err <= 4 * dev_ref, k


def error_bounds(gold):
    """(rot, trans, depth) bounds of the module docstring."""
    return tuple(4 * np.abs(gold["errors32"] - gold["errors64"]).max(axis=0))


def test_evaluate_all_against_the_reference(given, model, lp, scene, ds, gold, dev):
    e64 = gold["errors64"]
    res = ev.evaluate_all(model, lp, scene, ds, given, 0, dev, None, return_table=True)
    best, psnr, ssim, lpips, rot, trans, depth, table = res
    table = table.cpu().numpy()
    for col, name, bound in zip((3, 4, 5), ("rot", "trans", "depth"), error_bounds(gold)):
        err = np.abs(table[:, col] - e64[:, col - 3]).max()
        print("%-5s error: |ours - reference64| %.3e, bound %.3e (values %s)" % (name, err, bound, table[:, col]))
        assert err <= bound, name
    assert best == str(int(gold["all64"][0])) == str(int(gold["all32"][0]))                # exact
    b = int(best)
    assert [psnr, ssim, lpips, rot, trans] == table[b, :5].tolist()
    assert depth == table[4, 5]                                                           # id 4's, not the best id's: the reference's leak
    assert int(gold["all64"][0]) != 4 and gold["all64"][3] == e64[4, 2]                    # ... which the golden can tell apart


def test_evaluate_is_one_row_of_evaluate_all_and_scores_its_renders(given, model, lp, scene, ds, gold, dev):
    table = ev.evaluate_all(model, lp, scene, ds, given, 0, dev, None, return_table=True)[-1].cpu().numpy()
    e64 = gold["errors64"]
    k = int(gold["all64"][0])
    r = given[str(k)]
    psnr, ssim, lpips, rot, trans, depth, renders = ev.evaluate(model, lp, scene, ds, r["poses_cam"], r["features_raw"], r["nvs_extr"], r["gt_poses"], 0,
                                                                k, dev, None, return_renders=True)
    assert all(isinstance(v, float) for v in (psnr, ssim, lpips, rot, trans, depth))
    assert rot == table[k, 3] and trans == table[k, 4]                                    # the same float64 arithmetic on the same poses
    assert abs(depth - e64[k, 2]) <= error_bounds(gold)[2]
    gt = scene["images"][0, 5:10]
    im = fm.image_metrics(renders["imgs"][0], gt, lp)
    assert psnr == im["psnr"].mean().item() and ssim == im["ssim"].mean().item() and lpips == im["lpips"].double().mean().item()
    d = (scene["depths"][0, :5] - renders["depths"][0]).abs().mean().clamp(0.0, 2.0).item()
    assert abs(depth - d) <= 1e-6 * max(1.0, d)
    short = ev.evaluate(model, lp, scene, ds, r["poses_cam"], r["features_raw"], r["nvs_extr"], r["gt_poses"], 0, k, dev, None, eval_pose=False)
    assert short == (psnr, ssim, lpips, depth)
    # a batch of five scenes against one scene: the same kernels on other launch shapes
    assert np.abs(table[k, :3] - np.array([psnr, ssim, lpips])).max() <= 1e-3 * max(1.0, abs(psnr))


def test_evaluate_all_on_the_model_s_own_predictions(initial, model, lp, scene, ds, dev):
    """The stacked path: predict_initial's own dict, untouched."""
    best, psnr, ssim, lpips, rot, trans, depth, table = ev.evaluate_all(model, lp, scene, ds, initial, 0, dev, None, return_table=True)
    table = table.cpu().numpy()
    assert np.isfinite(table).all()
    assert rot == table[:, 3].min() == table[int(best), 3] and depth == table[4, 5]
    assert [psnr, ssim, lpips, trans] == table[int(best), [0, 1, 2, 4]].tolist()


def test_equal_errors_resolve_as_the_reference_s_sort(given, model, lp, scene, ds, dev):
    """kubric_eval.py:249-251 sorts (rot_error, id) by the error, descending and stable, and takes the last entry: among equal errors the
    HIGHEST id. Built here: every pose's quaternion is orthogonal to its ground truth (180 degrees, capped at 50), so every id scores
    4 x 50 / 5 = 40; then id 1 alone is given its ground truth, and after it id 3 too."""
    def with_poses(exact):
        d = {}
        for k, v in given.items():
            gq = ev.geo_utils.mat2quat(v["gt_poses"][0, 1:5]).float()
            w, x, y, z = gq[:, :4].unbind(dim=1)
            off = torch.cat([torch.stack([-x, w, -z, y], dim=1), gq[:, 4:]], dim=1)
            d[k] = dict(v, poses_cam=gq if int(k) in exact else off)
        return d
    best, _, _, _, rot, _, _, table = ev.evaluate_all(model, lp, scene, ds, with_poses(()), 0, dev, None, return_table=True)
    assert table[:, 3].tolist() == [40.0] * 5 and rot == 40.0                              # the premise: five equal errors
    assert best == "4"
    best, _, _, _, rot, _, _, table = ev.evaluate_all(model, lp, scene, ds, with_poses((1,)), 0, dev, None, return_table=True)
    assert best == "1" and rot == table[1, 3].item() < 1.0       # float32 quaternions against float64 ones: acos near 1
    a = with_poses((1, 3))
    a["3"] = dict(a["1"])                                                                  # the same entry twice: bitwise equal errors
    best, _, _, _, rot, _, _, table = ev.evaluate_all(model, lp, scene, ds, a, 0, dev, None, return_table=True)
    assert table[1, 3].item() == table[3, 3].item() == rot and best == "3"


def test_sync_pose_against_the_reference(given, gold, dev):
    best = int(gold["sync_best"])
    P, conf, pairs = ev.sync_inputs(given, best, dev)
    assert pairs == [tuple(int(v) for v in p) for p in gold["sync_pairs"]]
    for got, name in ((P[0], "sync_P"), (conf[0], "sync_conf")):
        r32, r64 = gold[name + "32"], gold[name + "64"]
        err = np.abs(got.double().cpu().numpy() - r64)
        print("%s: |ours - reference64| %.3e, the reference's float32 run %.3e" % (name, err.max(), np.abs(r32 - r64).max()))
        assert (err <= 2 * np.abs(r32 - r64).max() + 2 * ulp32(r64)).all(), name
    out, status = ev.sync_pose(given, best, dev)
    assert status.tolist() == [0]
    r32, r64 = gold["sync_out32"], gold["sync_out64"]
    err = np.abs(out.double().cpu().numpy() - r64)
    print("sync_pose: |ours - reference64| %.3e, the reference's float32 run %.3e" % (err.max(), np.abs(r32 - r64).max()))
    assert (err <= 2 * np.abs(r32 - r64).max() + 2 * ulp32(r64)).all()
    assert not torch.equal(out, given[str(best)]["poses_cam"])


def test_sync_pose_hands_back_undetermined_problems(initial, dev):
    """The model's own predictions disagree by radians: the synchronised rotations are not determined by them (the reference returns an
    arbitrary rotation without noticing). The poses that went in come back, with the reason."""
    for best in (0, 3):
        out, status = ev.sync_pose(initial, best, dev)
        assert status.item() & ops.POSE_SYNC_RANK
        assert torch.equal(out, initial[str(best)]["poses_cam"])
