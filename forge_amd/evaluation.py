"""The evaluation protocol of kubric_eval.py on the device: what joins the predicted-pose forward, the refinement loop, the 360-degree
synthesis and the image metrics into the reference's "before / after" result line (kubric_eval.py:36-93).

    permute_clips(clips, gt_poses, nvs_extr, canonical_id, ...)      utils/eval_utils.py:30-63
    compute_pose_metric(pred, gt)                                    utils/eval_utils.py:14-27, batched, on tensors
    predict_initial(model, sample, device)                           kubric_eval.py:371-409
    evaluate(model, lpips_vgg, sample, dataset, poses_cam, ...)      kubric_eval.py:258-367 (no plotting)
    evaluate_all(model, lpips_vgg, sample, dataset, return_dict, ..) kubric_eval.py:235-255
    sync_pose(return_dict, best_canonical_id, device)                kubric_eval.py:95-145 on ops.pose_sync (forge_pose_sync)

Same names, argument orders and return orders as the reference, so its run_optimization can call them unchanged
(`from forge_amd.evaluation import ...`); `model` may be the module or a wrapper with `.module` (the reference wraps it in DataParallel).
Like the reference, the protocol scores ONE scene per call (batch 1) of five input views and five novel views.

What is different, on purpose:
  - predict_initial runs the encoder once on the five images; the five canonical choices are gathers of its output, and both pose
    estimators and the pose head run once on the five permuted clips as a batch of five (the reference: five full passes);
  - evaluate_all pushes the five choices through rotate / fuse / heads / render / metrics as one batch of five scenes;
  - nothing is read back before the single final read-out of a call (the reference: about twenty .cpu() round trips);
  - affine inverses are closed-form (geo_utils.inverse_affine), not LU;
  - compute_pose_metric clamps the quaternion dot product to <= 1 (the reference returns NaN there);
  - sync_pose returns (poses, status) and never raises on bad data: when forge_pose_sync flags the problem (ops.POSE_SYNC_* bits) the
    unsynchronised poses of the best canonical id come back, which is what the bare `except:` around the reference's caller amounts to.
"""
import math

import torch
import torch.nn.functional as F

from . import geo_utils, metrics, ops
from .staging import stage_sample

N_INPUT = 5                     # input views, and novel views scored (kubric_eval.py:238, 274-275, 302)
ROT_ERROR_CAP = 50.0            # kubric_eval.py:362


def _module(model):
    return getattr(model, "module", model)


def permutation(canonical_id, t):
    """utils/eval_utils.py:36-41: the canonical view first, the others in their order (all three branches of the reference give this)."""
    canonical_id = int(canonical_id)
    return [canonical_id] + [i for i in range(t) if i != canonical_id]


def permute_clips(clips, gt_poses, nvs_extr, canonical_id, clips_only=False, return_permutation=False):
    """utils/eval_utils.py:30-63. clips [1, t, c, h, w]; gt_poses [1, t, 4, 4] relative poses; nvs_extr [1, V, 4, 4] canonicalised extrinsics.
    Returns the clips with view `canonical_id` first, the poses relative to that view in the same order [1, t, 4, 4], and the extrinsics
    re-canonicalised on it [1, V, 4, 4] (unpermuted, as in the reference) - on the inputs' device, with closed-form affine inverses."""
    t = clips.shape[1]
    canonical_id = int(canonical_id)
    permute = permutation(canonical_id, t)
    clips = clips[:, permute]
    if clips_only:
        return clips
    gt_poses = gt_poses.reshape(-1, 4, 4)
    nvs_poses = geo_utils.inverse_affine(nvs_extr.reshape(-1, 4, 4))
    gt_poses = geo_utils.get_relative_pose(gt_poses[canonical_id], gt_poses)[permute].unsqueeze(0)
    shift = torch.eye(4, dtype=nvs_poses.dtype, device=nvs_poses.device)
    shift[2, 3] = -4.0                                      # inverse of the translation by (0, 0, 4) (utils/eval_utils.py:53-56)
    nvs_poses = geo_utils.canonicalize_poses(shift, geo_utils.get_relative_pose(nvs_poses[canonical_id], nvs_poses))
    nvs_extr = geo_utils.inverse_affine(nvs_poses).unsqueeze(0)
    if return_permutation:
        return clips, gt_poses, nvs_extr, permute
    return clips, gt_poses, nvs_extr


def compute_pose_metric(pred, gt):
    """utils/eval_utils.py:14-27 on tensors of any device, batched: pred, gt [..., 7] (quaternion w x y z, translation) ->
    (theta [...] in degrees = 2 acos(|<q_pred, q_gt>|), t_error [...] = |t_pred - t_gt|). The quaternions are NOT normalised, as in the
    reference. The one deviation: the dot product is clamped to <= 1, where the reference returns NaN."""
    d = (pred[..., :4] * gt[..., :4]).sum(dim=-1).abs().clamp(max=1.0)
    theta = 2.0 * torch.acos(d) * (180.0 / math.pi)
    return theta, (pred[..., 4:] - gt[..., 4:]).norm(dim=-1)


class ReturnDict(dict):
    """predict_initial's result: the reference's dict {'0'..'4': {...}} (sync_pose counts its keys, so it holds nothing else). `stacked`
    keeps the five entries as single tensors for evaluate_all; the per-id entries are views of them."""
    stacked = None


def predict_initial(model, sample, device):
    """kubric_eval.py:371-409: for every canonical choice k of the five input views, the predicted relative poses of the other four and
    the permuted feature volumes: {str(k): {'permutation', 'poses_cam' [4, 7], 'features_raw' [1, 5, C, D, H, W], 'nvs_extr' [1, V, 4, 4],
    'gt_poses' [1, 5, 4, 4] (float64)}}, tensors on `device`. get_feat3D runs once; the five permutations are gathers of its output and go through
    the pose estimators and the pose head as one batch of five."""
    m = _module(model)
    s = stage_sample(sample, device)
    clips = s["images"][:, :N_INPUT]
    b, t, c, h, w = clips.shape
    if b != 1:
        raise ValueError("predict_initial: the protocol scores one scene per call (kubric_eval.py:54), got a batch of %d" % b)
    perms = [permutation(k, t) for k in range(t)]
    idx = torch.tensor(perms, device=clips.device)
    with torch.no_grad():
        clips_all = clips[0][idx]                                                    # [t, t, c, h, w]: clip k has view k first
        f2d, join2d = m._pose2d_features(clips_all)
        feats = m.encoder_3d.get_feat3D(clips.reshape(t, c, h, w))                   # once: a permuted clip has the same five images
        feats_all = feats[idx]                                                       # [t, t, C, D, H, W]
        f3d = m.encoder_traj(feats_all, return_features=True)                        # [t (t-1), 1024]
        join2d()
        pred = m.pose_head(torch.cat([f3d, f2d], dim=-1))
        poses, _ = pred.split([m.encoder_traj.pose_dim, 1], dim=-1)
        poses = torch.cat([F.normalize(poses[:, :4]), poses[:, 4:]], dim=1).reshape(t, t - 1, -1)
        # 15 small matrices: float64 costs nothing; the ground-truth poses stay float64 (evaluate takes its pose errors in float64)
        gt_in, extr_in = s["cam_poses_rel_cv2"][:, :N_INPUT].double(), s["cam_extrinsics_cv2_canonicalized"].double()
        gts, extrs = [], []
        for k in range(t):
            _, g, e = permute_clips(clips[:, :, :0], gt_in, extr_in, k)
            gts.append(g)
            extrs.append(e)
        gts, extrs = torch.cat(gts), torch.cat(extrs).float()
    out = ReturnDict()
    for k in range(t):
        out[str(k)] = {"permutation": perms[k], "poses_cam": poses[k], "features_raw": feats_all[k:k + 1], "nvs_extr": extrs[k:k + 1],
                       "gt_poses": gts[k:k + 1]}
    out.stacked = {"poses_cam": poses, "features_raw": feats_all, "nvs_extr": extrs, "gt_poses": gts}
    return out


def _score(m, lpips_vgg, sample, dataset, poses_cam, features, nvs_extr, gt_poses, device, eval_pose=True):
    """evaluate for S scenes that share the sample's images, intrinsics and depths: poses_cam [S, t-1, 7], features [S, t, C, D, H, W],
    nvs_extr [S, V, 4, 4], gt_poses [S, t, 4, 4] -> float64 [S, 6] on the device (psnr, ssim, lpips, rot, trans, depth) and the renders.
    No host synchronisation."""
    S, t, C, D, H, W = features.shape
    f32 = lambda x: x.to(device=device, dtype=torch.float32, non_blocking=True)
    poses_cam = f32(poses_cam).reshape(S * (t - 1), -1)
    can_p, can_e = geo_utils.canonical_cameras(m, dataset, device)
    rel = m.encoder_traj.toSE3(poses_cam)
    cam_poses = torch.cat([can_p.reshape(1, 1, 4, 4).expand(S, 1, 4, 4), (can_p[None] @ rel).reshape(S, t - 1, 4, 4)], dim=1)
    clips_nvs = f32(sample["images"])[:, N_INPUT:2 * N_INPUT]
    depths_nvs = f32(sample["depths"])[:, :N_INPUT]              # the reference scores the NOVEL renders against the INPUT views' depths
    V = clips_nvs.shape[1]
    _, _, c, h, w = clips_nvs.shape
    # rotate, with the view ordering of sequence_from_distance / chose_selected fused into its store
    fused = m.encoder_3d.fuse(m.rotate(voxels=features, camPoses_cv2=cam_poses, grid_size=D, order="distance"))
    features_mv, densities_mv = m.encoder_3d.heads(fused)
    extr = f32(nvs_extr)[:, N_INPUT:2 * N_INPUT].reshape(S * V, 4, 4)
    K = f32(sample["K_cv2"])[:, N_INPUT:2 * N_INPUT].expand(S, V, 3, 3).reshape(S * V, 3, 3)
    cameras = {"R": extr[:, :3, :3], "T": extr[:, :3, 3], "K": K}
    imgs, masks, depths = m.render(cameras, features_mv, densities_mv, render_depth=True, view2vol=m._view2vol(S, V, features.device))
    gt_imgs = clips_nvs.expand(S, V, c, h, w).reshape(S * V, c, h, w)
    im = metrics.image_metrics(imgs, gt_imgs, lpips_vgg)
    per_scene = lambda x: x.to(torch.float64).reshape(S, V).mean(dim=1)
    nan = torch.full((S,), float("nan"), dtype=torch.float64, device=features.device)
    depth_err = (depths_nvs.reshape(1, V, 1, h, w) - depths.reshape(S, V, 1, h, w)).abs().mean(dim=(1, 2, 3, 4)).clamp(min=0.0, max=2.0)
    rot, trans = nan, nan
    if eval_pose:
        # 4 S poses: float64 costs nothing, and the angle of nearly aligned quaternions (acos near 1) loses half its digits in float32
        gq = geo_utils.mat2quat(gt_poses.to(device=device, dtype=torch.float64, non_blocking=True)[:, 1:N_INPUT].reshape(S * (t - 1), 4, 4))
        theta, terr = compute_pose_metric(poses_cam.double(), gq)
        theta = torch.where(theta < ROT_ERROR_CAP, theta, torch.full_like(theta, ROT_ERROR_CAP))      # NaN is capped too, as `x if x < 50 else 50`
        rot = theta.reshape(S, t - 1).sum(dim=1) / 5.0                           # four errors over 5.0 (kubric_eval.py:364-365)
        trans = terr.reshape(S, t - 1).sum(dim=1) / 5.0
    table = torch.stack([per_scene(im["psnr"]), per_scene(im["ssim"]), per_scene(im["lpips"]) if "lpips" in im else nan, rot, trans,
                         depth_err.to(torch.float64)], dim=1)
    return table, {"imgs": imgs.reshape(S, V, c, h, w), "masks": masks.reshape(S, V, 1, h, w), "depths": depths.reshape(S, V, 1, h, w)}


def evaluate(model, lpips_vgg, sample, dataset, poses_cam, features, nvs_extr, gt_poses, batch_idx=0, canonical_id=0, device=None,
             output_dir=None, name="before", eval_pose=True, return_renders=False):
    """kubric_eval.py:258-367 without its plotting: rotate -> view ordering -> fuse -> heads -> render of the five novel views with depth ->
    PSNR / SSIM / LPIPS (metrics.image_metrics), pose errors, depth error. Returns Python floats (psnr, ssim, lpips, rot_error, trans_error,
    depth_error), or (psnr, ssim, lpips, depth_error) with eval_pose=False; lpips is NaN when lpips_vgg is None. One read-out at the end, no
    host synchronisation before it. return_renders (not in the reference) appends {'imgs', 'masks', 'depths'} of the novel views.
    Quirks of the reference that are kept: rotation and translation errors are summed over the FOUR predicted poses and divided by 5.0; each
    rotation error is capped at 50 degrees; depth_error compares the renders of the NOVEL views with sample['depths'][:, :5], the depths of
    the INPUT views, and is clamped to [0, 2]. batch_idx, canonical_id, output_dir and name only label the reference's plots and are unused."""
    m = _module(model)
    device = features.device if device is None else device
    with torch.no_grad():
        table, renders = _score(m, lpips_vgg, sample, dataset, poses_cam[None], features, nvs_extr, gt_poses, device, eval_pose)
    psnr, ssim, lp, rot, trans, depth = table[0].cpu().tolist()                  # the read-out
    res = (psnr, ssim, lp, rot, trans, depth) if eval_pose else (psnr, ssim, lp, depth)
    return res + (renders,) if return_renders else res


def evaluate_all(model, lpips_vgg, sample, dataset, return_dict, batch_idx=0, device=None, output_dir=None, name="before", eval_pose=True,
                 return_table=False):
    """kubric_eval.py:235-255: evaluate for each of the five canonical choices, as ONE batch of five scenes, then the best choice.
    Returns (best_canonical_id, psnr, ssim, lpips, rot_error, trans_error, depth_error); best_canonical_id is the dict key (a str), as in the
    reference. The best id has the smallest rotation error; the choice is made by the reference's own expression (a stable descending sort
    whose last entry is taken), so equal errors resolve exactly as they do there. Kept quirk: depth_error is that of canonical id 4, not of
    the best id (the reference leaks its loop variable). return_table (not in the reference) appends the float64 [5, 6] table of all ids
    (psnr, ssim, lpips, rot, trans, depth)."""
    m = _module(model)
    keys = [str(k) for k in range(N_INPUT)]
    st = getattr(return_dict, "stacked", None)
    same = lambda f: all(return_dict[k][f].data_ptr() == st[f][i].data_ptr() for i, k in enumerate(keys))
    if st is None or not all(same(f) for f in ("poses_cam", "features_raw", "nvs_extr", "gt_poses")):     # a plain dict, or an entry replaced
        col = lambda f: [return_dict[k][f] for k in keys]
        st = {"poses_cam": torch.stack(col("poses_cam")), "features_raw": torch.cat(col("features_raw")), "nvs_extr": torch.cat(col("nvs_extr")),
              "gt_poses": torch.cat(col("gt_poses"))}
    device = st["features_raw"].device if device is None else device
    with torch.no_grad():
        table, _ = _score(m, lpips_vgg, sample, dataset, st["poses_cam"], st["features_raw"], st["nvs_extr"], st["gt_poses"], device, True)
    rows = table.cpu().tolist()                                                  # the read-out
    eval_results = {k: dict(zip(("psnr", "ssim", "lpips", "rot_error", "trans_error", "depths_error"), rows[i])) for i, k in enumerate(keys)}
    rot_error_res = sorted([(eval_results[k]["rot_error"], k) for k in eval_results], key=lambda x: x[0], reverse=True)
    best_canonical_id = rot_error_res[-1][1]
    r = eval_results[best_canonical_id]
    res = (best_canonical_id, r["psnr"], r["ssim"], r["lpips"], r["rot_error"], r["trans_error"], eval_results[keys[-1]]["depths_error"])
    return res + (table,) if return_table else res


def sync_inputs(return_dict, best_canonical_id, device=None):
    """The synchronisation problem of kubric_eval.py:95-135 from predict_initial's result: (P [1, E, 4, 4] float32 pairwise extrinsics,
    conf [1, E] float32, pairs) for ops.pose_sync, all on the device. Confidences are (cos(theta) + 1) / 2 with theta the rotation angle of
    pose_ij @ pose_ji (compute_pose_metric against the identity; float64, rounded once). A pair's extrinsics are the inverse of its
    predicted pose, or the pose of the reversed pair where `best_canonical_pairs` says so - that list holds (best id, idx) with idx a
    POSITION 0..t-2 in the permuted clip, not a view id, as in the reference."""
    keys = list(return_dict.keys())
    t = len(keys)
    best = int(best_canonical_id)
    poses = torch.stack([return_dict[k]["poses_cam"] for k in keys])              # [t, t-1, 7]
    device = poses.device if device is None else device
    poses = poses.to(device=device, dtype=torch.float32)
    mats = geo_utils.quat2mat(poses.reshape(t * (t - 1), -1)).reshape(t, t - 1, 4, 4)
    rows, cols = [], []
    for k in keys:
        perm = return_dict[k]["permutation"]
        assert k == str(perm[0])
        rows += [int(k)] * (t - 1)
        cols += [int(perm[i + 1]) for i in range(t - 1)]
    table = torch.eye(4, dtype=torch.float32, device=device).repeat(t, t, 1, 1)
    table[torch.tensor(rows, device=device), torch.tensor(cols, device=device)] = mats.reshape(t * (t - 1), 4, 4)     # pose_dict[(it, view)]
    best_pairs = [(best, idx) for idx in range(t - 1)]
    pairs = [(i, j) for i in range(t) for j in range(i + 1, t)]
    reverse = [(p not in best_pairs) and (p[::-1] in best_pairs) for p in pairs]
    pi = torch.tensor([p[0] for p in pairs], device=device)
    pj = torch.tensor([p[1] for p in pairs], device=device)
    fwd, bwd = table[pi, pj], table[pj, pi]
    P = torch.where(torch.tensor(reverse, device=device)[:, None, None], bwd, geo_utils.inverse_affine(fwd))
    loop = geo_utils.mat2quat(fwd.double() @ bwd.double())
    ident = torch.zeros(7, dtype=torch.float64, device=device)
    ident[0] = 1.0
    theta, _ = compute_pose_metric(loop, ident)
    conf = ((torch.cos(theta * (math.pi / 180.0)) + 1.0) / 2.0).to(torch.float32)
    return P[None].contiguous(), conf[None].contiguous(), pairs


def sync_pose(return_dict, best_canonical_id, device=None, rank_tol=1e-6):
    """kubric_eval.py:95-145 on the device: the 20 predicted relative poses of predict_initial's five canonical choices are synchronised by
    ops.pose_sync (forge_pose_sync: squares = 10, centred on view 0) and expressed relative to the best canonical view, in its clip order.
    Returns (poses_rel_quat [t-1, 7], status [1] int32). A non-zero status (ops.POSE_SYNC_* bits: no mass, a rotation the data do not
    determine, a non-finite input) means the synchronisation is not to be trusted; the poses returned are then the unsynchronised
    poses_cam of the best canonical id, selected on the device - the call never reads anything back."""
    t = len(return_dict)
    if t < 3:
        raise ValueError("sync_pose: %d views; two views are plain chaining (utils/sync_utils.py:camera_chaining), nothing to synchronise" % t)
    P, conf, pairs = sync_inputs(return_dict, best_canonical_id, device)
    out, status = ops.pose_sync(P, conf, pairs, t, squares=10, center_first_camera=True, rank_tol=rank_tol)
    best = return_dict[str(best_canonical_id)]
    poses = geo_utils.inverse_affine(out[0])[torch.tensor(best["permutation"], device=out.device)]
    synced = geo_utils.mat2quat(geo_utils.get_relative_pose(poses[0], poses[1:]))
    keep = best["poses_cam"].to(device=out.device, dtype=torch.float32)
    return torch.where(status.reshape(1, 1) != 0, keep, synced), status


def evaluate_geometry(pred_meshes, gt_meshes, transform=None, align=None, iou=False, **kw):
    """The surface metrics beside the image and pose metrics above: geometry.mesh_metrics(pred_meshes, gt_meshes, transform=transform, align=align,
    **kw) - accuracy, completeness, Chamfer, Hausdorff, F-score and normal consistency as float64 device tensors, one entry per mesh pair.
    transform maps the predictions (canonical frame of view 0) into the ground truth's frame; where nobody knows it (predicted poses, photographs,
    meshes in their own object frame), align="icp" or a dict of geometry.align_points keywords estimates it on the device first and returns it
    under 'alignment'. surface="triangles" (passed through **kw) scores each side's samples against the other side's triangles, not its
    samples: the distance to the surface, free of the sampling floor. iou=True, or a dict of geometry.volume_iou keywords (n, absolute), adds
    the volumetric intersection over union under the same transform - the one align= found, when it found one: 'iou', 'volume_pred', 'volume_gt'
    and 'iou_status' (volume_iou's 'status'); both sides must then be meshes. Not part of evaluate_all, whose outputs are the reference's."""
    from . import geometry
    res = geometry.mesh_metrics(pred_meshes, gt_meshes, transform=transform, align=align, **kw)
    if iou is not False and iou is not None:
        if not (iou is True or isinstance(iou, dict)):
            raise ValueError("evaluate_geometry: iou must be False, True or a dict of volume_iou keywords, got %r" % (iou,))
        if "alignment" in res:
            transform = res["alignment"].transform.to(torch.float32)
        vol = geometry.volume_iou(pred_meshes, gt_meshes, transform=transform, **(iou if isinstance(iou, dict) else {}))
        res.update({"iou": vol["iou"], "volume_pred": vol["volume_pred"], "volume_gt": vol["volume_gt"], "iou_status": vol["status"]})
    return res
