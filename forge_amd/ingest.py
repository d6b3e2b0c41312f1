"""Photographs to the model's input tensors, on the device (include/forge_hip.h section h, csrc/ingest.hip).

The reference turns a frame into `images` / `fg_probabilities` in Pillow, on one CPU core per image (`_load_frame` of dataset/kubric.py:410-445,
dataset/gso.py:257-290, dataset/omniobject3d.py:221-258; the image loop of demo.py:236-256): an 8-bit RGB(A) image of any size is put on a
background, resized to img_size with Image.ANTIALIAS (Lanczos, a = 3), the mask `alpha > 0` is resized with Image.NEAREST, and the result is divided
by 255. `ingest` does the same on the MI355X from the raw bytes and gives Pillow's result bit for bit: on 8-bit images Pillow's resampler is integer
arithmetic after the coefficient table (22-bit fixed point, an 8-bit image between the two passes, a clip).

Backgrounds
    "black"      dataset.mask_images = True (every shipped configuration): RGB is resized with alpha ignored, the float image is multiplied by the
                 resized mask.
    "white"      mask_images = False: every channel is first put over white, as Image.paste does it; not masked afterwards.
    "premasked"  demo.py:244-248: RGB is zeroed where alpha == 0, then resized; not masked afterwards.
With three channels there is no alpha: "white" and "premasked" resize the bytes as they are, and the mask is (R > 0) | (G > 0). Blue plays no part
in it: the third operand of np.logical_or at dataset/omniobject3d.py:228-230 is its `out=` argument. That is reproduced literally.

Out of scope: train.normalize_img (False in every configuration), the depth TIFFs of the Kubric loader (read and resized with OpenCV there), and file
decoding - `ingest` starts from decoded 8-bit frames.
"""
import ctypes

import numpy as np
import torch

from . import _lib

BACKGROUNDS = {"black": 0, "white": 1, "premasked": 2}
PRECISION_BITS = 22

_COEFFS = {}


class Coeffs:
    """One axis' resampling table: first [n_out], count [n_out], k [n_out, K] (Pillow's, from forge_resample_coeffs), nearest [n_out] as int32 numpy
    arrays on the host; device(dev) the packed int32 table forge_ingest_rgba8 reads (a copy when the sizes agree, as Pillow skips that pass)."""

    def __init__(self, n_in, n_out):
        L = _lib.lib()
        K = L.forge_resample_taps(int(n_in), int(n_out))
        _lib.check(min(K, 0), "forge_resample_taps")
        self.n_in, self.n_out, self.K = int(n_in), int(n_out), K
        self.first, self.count, self.nearest = (np.zeros(n_out, np.int32) for _ in range(3))
        self.k = np.zeros((n_out, K), np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _lib.check(L.forge_resample_coeffs(self.n_in, self.n_out, p(self.first), p(self.count), p(self.k)), "forge_resample_coeffs")
        _lib.check(L.forge_resample_nearest(self.n_in, self.n_out, p(self.nearest)), "forge_resample_nearest")
        self._device = {}

    def packed(self):
        """(int32 numpy table first | count | nearest | k tap-major, its K)."""
        if self.n_in == self.n_out:
            i = np.arange(self.n_out, dtype=np.int32)
            return np.concatenate([i, np.ones_like(i), i, np.full_like(i, 1 << PRECISION_BITS)]), 1
        return np.concatenate([self.first, self.count, self.nearest, np.ascontiguousarray(self.k.T).reshape(-1)]), self.K

    def device(self, dev):
        key = str(dev)
        if key not in self._device:
            tab, K = self.packed()
            self._device[key] = (torch.from_numpy(tab).to(dev), K)
        return self._device[key]


def resample_coeffs(n_in, n_out):
    """The table of one axis, computed once per (n_in, n_out) by the library's host code and kept, with its device copies."""
    key = (int(n_in), int(n_out))
    if key not in _COEFFS:
        _COEFFS[key] = Coeffs(*key)
    return _COEFFS[key]


def _size(img_size):
    Ho, Wo = (img_size, img_size) if isinstance(img_size, int) else img_size
    return int(Ho), int(Wo)


def ingest_rgba8(src, Ho, Wo, background, table_x, Kx, table_y, Ky, return_bytes=False):
    """forge_ingest_rgba8 on a uint8 device tensor [N, H, W, C] with unit channel stride and packed pixels (any image and row stride): allocates the
    outputs and the workspace, launches on the current stream. Every argument is checked by the library before a launch."""
    N, H, W, C = src.shape
    dev = src.device
    images = torch.empty(N, 3, Ho, Wo, device=dev)
    masks = torch.empty(N, 1, Ho, Wo, device=dev)
    out = torch.empty(N, Ho, Wo, 3, dtype=torch.uint8, device=dev) if return_bytes else None
    ws = torch.empty(max(N * H * Wo, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().forge_ingest_rgba8(_lib.ptr(src), N, H, W, C, src.stride(0), src.stride(1), _lib.ptr(table_x), Kx, _lib.ptr(table_y), Ky, Ho, Wo,
                                                 background, _lib.ptr(ws), ws.numel() * 4, _lib.ptr(images), _lib.ptr(masks), _lib.ptr(out),
                                                 _lib.current_stream()), "forge_ingest_rgba8")
    return images, masks, out


def _ingest_batch(src, Ho, Wo, mode, return_bytes):
    if src.dim() != 4 or src.dtype != torch.uint8:
        raise RuntimeError("forge_amd: ingest takes uint8 frames [N, H, W, C], got %s %s" % (src.dtype, tuple(src.shape)))
    N, H, W, C = src.shape
    if N > 1 and src.stride(0) < (H - 1) * src.stride(1) + W * C or src.stride(3) != 1 or src.stride(2) != C or src.stride(1) < W * C:
        src = src.contiguous()                       # anything but packed pixels in non-overlapping rows: one copy; a strided view goes by its strides
    tx, Kx = resample_coeffs(W, Wo).device(src.device)
    ty, Ky = resample_coeffs(H, Ho).device(src.device)
    return ingest_rgba8(src, Ho, Wo, mode, tx, Kx, ty, Ky, return_bytes)


def ingest(frames, img_size, background="black", return_bytes=False, device=None):
    """frames: a uint8 tensor or array [N, H, W, C] (C = 3 or 4), or a list of [H, W, C] arrays / tensors of any sizes. Host frames are copied to the
    device as bytes (a quarter of their float size); a device tensor with unit channel stride is read through its strides, not copied. One pair of
    launches per tensor, or per group of equally shaped frames of a list.
    Returns (images [N, 3, S, S] float32, masks [N, 1, S, S] float32) on the device, and the resized bytes [N, S, S, 3] uint8 - Pillow's own - as a
    third entry with return_bytes. img_size: S or (height, width). There is no host path: without the MI355X this raises."""
    if background not in BACKGROUNDS:
        raise RuntimeError("forge_amd: ingest: unknown background %r (one of %s)" % (background, ", ".join(BACKGROUNDS)))
    mode = BACKGROUNDS[background]
    Ho, Wo = _size(img_size)
    if device is None:
        first = frames[0] if isinstance(frames, (list, tuple)) and len(frames) else frames
        device = first.device if torch.is_tensor(first) and first.is_cuda else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None:
        raise RuntimeError("forge_amd: ingest runs only on the MI355X HIP kernels; there is no CPU path")
    up = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device)          # uint8 in, uint8 over the bus
    if not isinstance(frames, (list, tuple)):
        out = _ingest_batch(up(frames), Ho, Wo, mode, return_bytes)
        return out if return_bytes else out[:2]
    if not frames:
        raise RuntimeError("forge_amd: ingest: an empty list of frames")
    groups = {}
    for i, f in enumerate(frames):
        groups.setdefault(tuple(f.shape), []).append(i)
    n = len(frames)
    images, masks = torch.empty(n, 3, Ho, Wo, device=device), torch.empty(n, 1, Ho, Wo, device=device)
    out = torch.empty(n, Ho, Wo, 3, dtype=torch.uint8, device=device) if return_bytes else None
    for idx in groups.values():
        members = [frames[i] for i in idx]
        if all(torch.is_tensor(f) for f in members):
            batch = torch.stack([f.to(device) for f in members]) if len(members) > 1 else members[0].to(device)[None]
        else:
            batch = up(np.stack([f.cpu().numpy() if torch.is_tensor(f) else np.asarray(f) for f in members]))      # one upload per group
        im, ma, by = _ingest_batch(batch, Ho, Wo, mode, return_bytes)
        where = torch.tensor(idx, device=device)
        images[where], masks[where] = im, ma
        if return_bytes:
            out[where] = by
    return (images, masks, out) if return_bytes else (images, masks)


def photos_to_sample(frames, config, t=None, background=None):
    """The image entries of the sample schema (synthetic.make_sample, dataset/kubric.py) from t photographs of one scene: 'images' [1, t, 3, S, S],
    'fg_probabilities' [1, t, 1, S, S], 'K_cv2' [1, t, 3, 3] = synthetic.intrinsics(S) (demo.py:39-41), S = config.dataset.img_size, on the device.
    background: default "black" where config.dataset.mask_images is True or absent (every shipped configuration), else "white"."""
    from . import synthetic
    S = int(config.dataset.img_size)
    if background is None:
        background = "black" if dict(config.dataset).get("mask_images", True) else "white"
    images, masks = ingest(frames, S, background)
    if t is not None and images.shape[0] != t:
        raise ValueError("photos_to_sample: %d frames for t = %d" % (images.shape[0], t))
    t = images.shape[0]
    return {"images": images[None], "fg_probabilities": masks[None], "K_cv2": synthetic.intrinsics(S).to(images.device)[None, None].repeat(1, t, 1, 1)}


def _module(model):
    return model.module if hasattr(model, "module") else model


def reconstruct_clips(model, model_gt, config, dataset, clips, iter_num=500, n_views=28, mesh=False, use_graph=True):
    """run_demo of demo.py:30-112 on clips [b, t, 3, S, S] already on the device. `model` (the jointly trained one) lifts the clips, predicts the
    relative poses with both estimators and the pose head, and refines them against the clips themselves (refine.refine_poses, mask R > 0.05 as
    demo.py:119); `model_gt` (trained with ground-truth poses) warps, orders, fuses, runs the heads and renders the 360-degree views with the density
    clamped at 1 (demo.py:94). mesh=True adds geometry.colored_mesh on the fused volume, coloured from the clips at the refined cameras.
    Returns a dict: 'images' [b, n_views, 3, S, S], 'masks' [b, n_views, 1, S, S], 'poses_cam' [b (t-1), 7], 'cam_poses_cv2' / 'cam_extrinsics_cv2'
    [b, t, 4, 4], 'clips', and with mesh 'meshes' (what colored_mesh returns)."""
    from . import geo_utils, geometry, nvs, refine, synthetic
    m, g = _module(model), _module(model_gt)
    m.eval(), g.eval()
    b, t, c, h, w = clips.shape
    dev = clips.device
    K = synthetic.intrinsics(h).to(dev)
    with torch.no_grad():
        feats = m.encoder_3d.get_feat3D(clips.reshape(b * t, c, h, w))
        feats = feats.reshape(b, t, *feats.shape[1:])
        f3d = m.encoder_traj(feats, return_features=True)
        f2d = m.encoder_traj_2d(clips, return_features=True)
        pose_vec, _ = m.pose_head(torch.cat([f3d, f2d], dim=-1)).split([m.encoder_traj.pose_dim, 1], dim=-1)
        pose_vec = torch.cat([torch.nn.functional.normalize(pose_vec[:, :4]), pose_vec[:, 4:]], dim=1)
    target_masks = (clips[:, :, 0:1] > 0.05).float().reshape(b * t, 1, h, w)
    Kbt = K[None, None].repeat(b, t, 1, 1)
    poses_cam, _, _ = refine.refine_poses(m, config, dataset, feats, pose_vec, clips.reshape(b * t, c, h, w), target_masks, Kbt, dev, iter_num=iter_num,
                                          use_graph=use_graph)
    with torch.no_grad():
        can_p, can_e = geo_utils.canonical_cameras(g, dataset, dev)
        _, cam_poses, cam_extr = geo_utils.predicted_camera_chain(poses_cam, m.encoder_traj.toSE3, can_p, can_e, b, t)
        ft = g.rotate(voxels=feats, camPoses_cv2=cam_poses, grid_size=feats.shape[3], order="distance")
        fused = g.encoder_3d.fuse(ft)
        features_mv, densities_mv = g.encoder_3d.heads(fused)
        imgs, masks = nvs.render_360(g, features_mv, densities_mv, K, config.render.camera_z, n_views=n_views)[:2]
        out = {"images": imgs, "masks": masks, "poses_cam": poses_cam, "cam_poses_cv2": cam_poses, "cam_extrinsics_cv2": cam_extr, "clips": clips}
        if mesh:
            out["meshes"] = geometry.colored_mesh(g, fused, K, config.render.camera_z, photos=clips, photo_cameras=geo_utils.camera_dict(cam_extr, Kbt),
                                                  n_views=n_views)
    return out


def reconstruct_photos(model, model_gt, config, dataset, frames, iter_num=500, n_views=28, mesh=False, use_graph=True):
    """From t photographs of one object (uint8 RGBA or RGB frames of any sizes, as `ingest` takes them) to its 360-degree views and, with mesh=True,
    a coloured mesh: ingest(background="premasked") at config.dataset.img_size, then reconstruct_clips. demo.py uses t = 3 frames and 2000 refinement
    iterations."""
    clips, _ = ingest(frames, int(config.dataset.img_size), "premasked")
    return reconstruct_clips(model, model_gt, config, dataset, clips[None], iter_num=iter_num, n_views=n_views, mesh=mesh, use_graph=use_graph)
