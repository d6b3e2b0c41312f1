"""forge_amd — MI355X (gfx950) native implementation of the FORGE reconstruction hot path
(UT-Austin-RPL/FORGE: encoder lift -> voxel pose warp -> ConvGRU fusion -> volume render),
behind the reference's own nn.Module surface. See DESIGN.md / INTEGRATION.md.

    from forge_amd.model import FORGE                                   # models.model.FORGE
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    from forge_amd import metrics as lpips; lpips.LPIPS(net="vgg")      # import lpips (kubric_eval.py); metrics.psnr / ssim / image_metrics
"""
__version__ = "0.2.1"


def invalidate_packed(module):
    """Drop the packed-weight / folded-BatchNorm caches of every fused HIP inference path below `module`. Needed only after
    editing parameters through `.data` (which bypasses the version counters the caches key on); optimizer steps, load_state_dict,
    .to() and train()/eval() are tracked automatically."""
    from .convops import invalidate_packed as _inv
    _inv(module)


def set_deterministic(mode):
    """True / False / None (default: follow torch.are_deterministic_algorithms_enabled()): the bitwise-reproducible kernels for the weight
    gradients and the pose gradient (forge_amd/determinism.py)."""
    from .determinism import set_deterministic as _set
    _set(mode)


def is_deterministic():
    """The effective deterministic mode (forge_amd/determinism.py)."""
    from .determinism import is_deterministic as _is
    return _is()


def deterministic(mode=True):
    """`with forge_amd.deterministic(True): ...` - the mode inside the block, the previous setting restored on exit."""
    from .determinism import deterministic as _ctx
    return _ctx(mode)


def ingest_frames(frames, img_size, background="black", return_bytes=False, device=None):
    """8-bit photographs -> (images [N,3,S,S], masks [N,1,S,S]) on the device, Pillow's Lanczos resize bit for bit: forge_amd.ingest.ingest
    (the name `forge_amd.ingest` itself is the module)."""
    from .ingest import ingest as _ingest
    return _ingest(frames, img_size, background=background, return_bytes=return_bytes, device=device)


def photos_to_sample(frames, config, t=None, background=None):
    """The images / fg_probabilities / K_cv2 entries of the sample schema from t photographs (forge_amd/ingest.py)."""
    from .ingest import photos_to_sample as _p2s
    return _p2s(frames, config, t=t, background=background)


def reconstruct_photos(model, model_gt, config, dataset, frames, **kw):
    """demo.py's run_demo from photographs: ingest, poses, refinement, fusion, 360-degree views, optionally a coloured mesh (forge_amd/ingest.py)."""
    from .ingest import reconstruct_photos as _rp
    return _rp(model, model_gt, config, dataset, frames, **kw)


def sample_surface(meshes, n):
    """Deterministic, area-proportional surface samples of extracted meshes (forge_amd/geometry.py)."""
    from .geometry import sample_surface as _ss
    return _ss(meshes, n)


def point_metrics(a, b, **kw):
    """Accuracy, completeness, Chamfer, Hausdorff, F-score and normal consistency between two point sets on the device (forge_amd/geometry.py)."""
    from .geometry import point_metrics as _pm
    return _pm(a, b, **kw)


def mesh_metrics(pred, gt, **kw):
    """The same metrics between surfaces: meshes sampled on the device, a ground-truth mesh or point cloud (forge_amd/geometry.py)."""
    from .geometry import mesh_metrics as _mm
    return _mm(pred, gt, **kw)


def point_mesh_distance(points, meshes, **kw):
    """Exact point-to-triangle distances from points to the surface of meshes, on the device (forge_amd/geometry.py)."""
    from .geometry import point_mesh_distance as _pmd
    return _pmd(points, meshes, **kw)


def install_reference_aliases():
    """Make `from models.model import FORGE` (the import lines of kubric_train_*.py, demo.py,
    kubric_eval.py) and `from models.perceptual_loss import VGGPerceptualLoss` resolve to this package: registers forge_amd's modules under the reference's
    `models.*` names in sys.modules. Call once before importing the reference's entry scripts."""
    import importlib
    import sys
    import types
    pkg = types.ModuleType("models")
    pkg.__path__ = []
    sys.modules["models"] = pkg
    for name in ("model", "model_single_pose_estimator", "encoder", "fusion", "rotate", "volume_render",
                 "pose_estimator_3d", "pose_estimator_2d", "perceptual_loss"):
        mod = importlib.import_module("forge_amd." + ("perceptual" if name == "perceptual_loss" else name))
        sys.modules["models." + name] = mod
        setattr(pkg, name, mod)
