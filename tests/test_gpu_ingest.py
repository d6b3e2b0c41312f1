"""The photograph ingest on the MI355X (forge_amd.ingest -> csrc/ingest.hip) against Pillow's own output (tests/golden/ingest_pillow.npz, written by
tools/make_golden_ingest.py) and the numpy restatement of the contract (tests/ingest_cases.py). Everything is compared bit for bit: the contract
is integer arithmetic after the coefficient table, and the table is pinned on the CPU (tests/test_ingest_cpu.py)."""
import numpy as np
import pytest
import torch

import ingest_cases as ic

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def gold(golden):
    return golden("ingest_pillow")


def source(name):
    """The case's RGBA source (uint8 numpy) and its restatement per (channels, background), computed once and never modified."""
    if name not in _CACHE:
        _, H, W, Ho, Wo = next(c for c in ic.CASES if c[0] == name)
        rgba = ic.source(name, H, W)
        _CACHE[name] = (rgba, {(ch, bg): ic.ingest(np.ascontiguousarray(rgba[:, :, :ch]), Ho, Wo, bg) for ch in (3, 4) for bg in ic.BACKGROUNDS})
    return _CACHE[name]


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def same(got, want):
    """device (images, masks, bytes) rows against the restatement's (bytes, images, mask) of one frame"""
    images, masks, by = got
    rb, rf, rm = want
    assert images.dtype == torch.float32 and masks.dtype == torch.float32 and by.dtype == torch.uint8
    assert int((by.cpu().numpy() != rb).sum()) == 0
    assert np.array_equal(bits(images), rf.view(np.int32)) and np.array_equal(bits(masks), rm.view(np.int32))


@pytest.mark.parametrize("background", ic.BACKGROUNDS)
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("case", ic.CASES, ids=[c[0] for c in ic.CASES])
def test_every_golden_case(gold, case, channels, background):
    from forge_amd.ingest import ingest
    name, H, W, Ho, Wo = case
    rgba, ref = source(name)
    frame = np.ascontiguousarray(rgba[:, :, :channels])
    images, masks, by = ingest(frame[None], (Ho, Wo), background, return_bytes=True)
    assert tuple(images.shape) == (1, 3, Ho, Wo) and tuple(masks.shape) == (1, 1, Ho, Wo) and tuple(by.shape) == (1, Ho, Wo, 3) and images.is_cuda
    want = gold[ic.key(name, channels, background) + "/bytes"]
    differing = int((by[0].cpu().numpy() != want).sum())
    assert differing == 0, "%d bytes differ from Pillow's" % differing
    assert np.array_equal(masks[0, 0].cpu().numpy(), gold[ic.key(name, channels, background) + "/mask"].astype(np.float32))
    same((images[0], masks[0], by[0]), ref[(channels, background)])


def test_all_bytes_through_the_float_rule():
    from forge_amd.ingest import ingest
    b = np.arange(256, dtype=np.uint8).reshape(16, 16)
    frame = np.dstack([b, b[::-1], b.T, np.full_like(b, 255)])
    images, masks = ingest(frame[None], 16, "black")
    want = (frame[:, :, :3].astype(np.float64) / 255.0).astype(np.float32).transpose(2, 0, 1)
    assert np.array_equal(bits(images[0]), want.view(np.int32)) and bool((masks == 1).all())


def test_strided_batch_is_read_in_place(monkeypatch):
    """Three equally shaped frames as a window of a wider buffer (odd byte offsets, rows of 3-channel pixels that are not 4-byte aligned): passed by
    its strides - torch.Tensor.contiguous is never called on it - and every frame equals its own restatement."""
    from forge_amd import ingest as ig
    H, W, Ho, Wo = 37, 61, 16, 24
    for ch in (3, 4):
        rng = np.random.default_rng(5 + ch)
        wide = rng.integers(0, 256, size=(3, H + 2, W + 9, ch), dtype=np.uint8)
        wide[..., -1][wide[..., -1] < 90] = 0
        dev = torch.from_numpy(wide).cuda()
        view = dev[:, 1:1 + H, 5:5 + W]
        assert not view.is_contiguous()
        monkeypatch.setattr(torch.Tensor, "contiguous", lambda self, *a, **k: pytest.fail("the strided view was copied"))
        images, masks, by = ig.ingest(view, (Ho, Wo), "premasked", return_bytes=True)
        monkeypatch.undo()
        for n in range(3):
            same((images[n], masks[n], by[n]), ic.ingest(np.ascontiguousarray(wide[n, 1:1 + H, 5:5 + W]), Ho, Wo, "premasked"))
    # a channel-strided view cannot be read in place: one copy, the same result
    planar = torch.from_numpy(np.ascontiguousarray(wide[0].transpose(2, 0, 1))).cuda().permute(1, 2, 0)
    got = ig.ingest(planar[None], (Ho, Wo), "white", return_bytes=True)
    same(tuple(t[0] for t in got), ic.ingest(wide[0], Ho, Wo, "white"))


def test_list_of_differing_shapes():
    from forge_amd.ingest import ingest
    names = ("h13w29_8", "h64w100_32", "h5w9_16", "h64w100_32")                  # the second and fourth share a shape: one group, two frames
    frames = [source(n)[0] for n in names]
    frames[3] = np.ascontiguousarray(frames[3][::-1])
    frames[2] = torch.from_numpy(frames[2]).cuda()                                # host arrays and a device tensor in one list
    images, masks, by = ingest(frames, 12, "black", return_bytes=True)
    assert tuple(images.shape) == (4, 3, 12, 12) and tuple(masks.shape) == (4, 1, 12, 12) and tuple(by.shape) == (4, 12, 12, 3)
    for n, f in enumerate(frames):
        same((images[n], masks[n], by[n]), ic.ingest(f.cpu().numpy() if torch.is_tensor(f) else f, 12, 12, "black"))


def test_replay_from_a_captured_graph():
    from forge_amd import ingest as ig
    rgba = source("h301w257_32")[0]
    static = torch.from_numpy(rgba[None]).cuda()
    eager = ig.ingest(static, 32, "white", return_bytes=True)                    # also builds the tables' device copies before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ig.ingest(static, 32, "white", return_bytes=True)
    static.copy_(torch.from_numpy(np.ascontiguousarray(rgba[::-1])[None]))       # new pixels in the captured buffer: the replay must see them
    g.replay()
    torch.cuda.synchronize()
    flipped = ic.ingest(np.ascontiguousarray(rgba[::-1]), 32, 32, "white")
    same(tuple(t[0] for t in out), flipped)
    assert not torch.equal(out[2], eager[2])
    static.copy_(torch.from_numpy(rgba[None]))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


def test_photos_to_sample_schema():
    import forge_amd
    from forge_amd import synthetic as syn
    cfg = syn.kubric_config(img_size=64)
    frames = ic.photo_frames()
    s = forge_amd.photos_to_sample(frames, cfg, t=3)
    assert set(s) == {"images", "fg_probabilities", "K_cv2"}
    assert tuple(s["images"].shape) == (1, 3, 3, 64, 64) and tuple(s["fg_probabilities"].shape) == (1, 3, 1, 64, 64) and tuple(s["K_cv2"].shape) == (1, 3, 3, 3)
    assert all(v.dtype == torch.float32 and v.is_cuda for v in s.values())
    assert torch.equal(s["K_cv2"][0, 2].cpu(), syn.intrinsics(64))
    for n, f in enumerate(frames):                                                # every shipped configuration masks its images: "black"
        _, rf, rm = ic.ingest(f, 64, 64, "black")
        assert np.array_equal(bits(s["images"][0, n]), rf.view(np.int32)) and np.array_equal(bits(s["fg_probabilities"][0, n]), rm.view(np.int32))
    cfg.dataset.mask_images = False
    white = forge_amd.photos_to_sample(frames, cfg)
    assert np.array_equal(bits(white["images"][0, 0]), ic.ingest(frames[0], 64, 64, "white")[1].view(np.int32))
    with pytest.raises(ValueError):
        forge_amd.photos_to_sample(frames, cfg, t=5)


def test_refusals_raise_before_any_launch(monkeypatch):
    from forge_amd import _lib, ingest as ig
    frame = torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device="cuda")
    tx, Kx = ig.resample_coeffs(8, 4).device(frame.device)
    torch.cuda.synchronize()
    real = _lib.lib()

    class NoLaunch:
        """the library with the launch counted: a refusal must come back before hipLaunchKernel, which shows as the documented negative code"""
        codes = []

        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "forge_ingest_rgba8":
                return fn

            def wrapped(*a):
                rc = fn(*a)
                NoLaunch.codes.append(rc)
                return rc
            return wrapped
    monkeypatch.setattr(_lib, "lib", lambda: NoLaunch())
    with pytest.raises(RuntimeError, match="unknown background"):
        ig.ingest(frame, 4, "grey")
    assert NoLaunch.codes == []
    for bad, match in ((torch.zeros(1, 8, 8, 5, dtype=torch.uint8, device="cuda"), "3 or 4 channels"),
                       (torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device="cuda"), "3 or 4 channels")):
        with pytest.raises(RuntimeError, match=match):
            ig.ingest(bad, 4)
    with pytest.raises(RuntimeError, match="non-positive"):
        ig.ingest_rgba8(frame, 0, 4, 0, tx, Kx, tx, Kx)
    with pytest.raises(RuntimeError, match="unknown background mode"):
        ig.ingest_rgba8(frame, 4, 4, 7, tx, Kx, tx, Kx)
    with pytest.raises(RuntimeError, match="uint8"):
        ig.ingest(frame.float(), 4)
    assert NoLaunch.codes == [-1, -1, -1, -1]                                     # FORGE_EINVAL each time: returned by the argument checks
    with pytest.raises(RuntimeError, match="no CPU path"):
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
        ig.ingest(np.zeros((1, 8, 8, 4), np.uint8), 4)


def test_reconstruct_photos_is_the_composition_on_pillow_clips(gold):
    """reconstruct_photos on three RGBA frames of differing sizes (seeded weights, 2 refinement iterations, 4 views, deterministic mode so that
    the refinement's gradients are reproducible): finite outputs of the documented shapes, and bit for bit what reconstruct_clips gives on the
    clips Pillow made of the same frames (demo.py:236-256)."""
    import forge_amd
    from forge_amd import ingest as ig, synthetic as syn
    from forge_amd.model import FORGE
    dev = torch.device("cuda")
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    ds = syn.SyntheticDataset(1.5)
    frames = ic.photo_frames()
    t = len(frames)
    pillow = torch.from_numpy((gold["photos/premasked/bytes"].astype(np.float64) / 255.0).astype(np.float32).transpose(0, 3, 1, 2).copy()).to(dev)
    with forge_amd.deterministic(True):
        got = forge_amd.reconstruct_photos(model, model, cfg, ds, frames, iter_num=2, n_views=4, mesh=True)
        want = ig.reconstruct_clips(model, model, cfg, ds, pillow[None], iter_num=2, n_views=4, mesh=True)
    assert torch.equal(got["clips"], want["clips"]) and tuple(got["clips"].shape) == (1, t, 3, 256, 256)
    assert tuple(got["images"].shape) == (1, 4, 3, 256, 256) and tuple(got["masks"].shape) == (1, 4, 1, 256, 256)
    assert tuple(got["poses_cam"].shape) == (t - 1, 7) and tuple(got["cam_poses_cv2"].shape) == (1, t, 4, 4) == tuple(got["cam_extrinsics_cv2"].shape)
    for k in ("images", "masks", "poses_cam", "cam_poses_cv2", "cam_extrinsics_cv2"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    (meshes, extras), (wmeshes, _) = got["meshes"], want["meshes"]
    assert len(meshes) == len(extras) == 1
    assert torch.equal(meshes[0].vertices, wmeshes[0].vertices) and torch.equal(meshes[0].faces, wmeshes[0].faces)
    assert meshes[0].colors is None or torch.equal(meshes[0].colors.view(torch.int32), wmeshes[0].colors.view(torch.int32))
    assert all(p.requires_grad for p in model.parameters())
