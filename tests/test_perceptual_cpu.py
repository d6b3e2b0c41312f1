"""CPU: the VGG-16 perceptual loss's surface - the reference import alias, the reference's state_dict layout, both weight layouts, the seeded
initialisation against the golden's checksums, the no-download weight lookup, and the argument checks of the new C entries."""
import os

import numpy as np
import pytest
import torch

from forge_amd import _lib
from forge_amd import perceptual as fp


def test_reference_import_resolves_to_forge_amd():
    import forge_amd
    forge_amd.install_reference_aliases()
    from models.perceptual_loss import VGGPerceptualLoss
    assert VGGPerceptualLoss is fp.VGGPerceptualLoss
    from models.model import FORGE                                 # the existing aliases stay
    from forge_amd.model import FORGE as F2
    assert FORGE is F2


def test_state_dict_matches_reference(golden):
    g = golden("perceptual_vgg")
    m = fp.VGGPerceptualLoss(pretrained=False)
    mine = [(k, str(tuple(v.shape))) for k, v in m.state_dict().items()]
    assert mine == list(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert m.resize and not any(p.requires_grad for p in m.blocks.parameters())
    assert m.mean.requires_grad and m.std.requires_grad


def test_both_weight_layouts_load_identically():
    tv = fp.seeded_vgg16_state_dict(3)
    tv.update({"classifier.0.weight": torch.zeros(4, 4), "classifier.0.bias": torch.zeros(4)})       # ignored
    a = fp.VGGPerceptualLoss(weights=tv)
    b = fp.VGGPerceptualLoss(weights=a.state_dict())
    c = fp.VGGPerceptualLoss(pretrained=False, seed=3)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) and torch.equal(v, c.state_dict()[k]), k
    d = fp.VGGPerceptualLoss(pretrained=False, seed=4)
    d.load_state_dict(a.state_dict(), strict=True)                   # a reference-layout state_dict loads strictly
    assert torch.equal(getattr(d.blocks[3], "21").weight, getattr(a.blocks[3], "21").weight)
    with pytest.raises(KeyError):
        fp.VGGPerceptualLoss(weights={k: v for k, v in tv.items() if k != "features.12.weight"})


def test_weights_from_a_file(tmp_path, monkeypatch):
    p = tmp_path / "vgg.pth"
    torch.save(fp.seeded_vgg16_state_dict(5), str(p))
    monkeypatch.setenv("FORGE_VGG16_WEIGHTS", str(p))
    a = fp.VGGPerceptualLoss()
    b = fp.VGGPerceptualLoss(pretrained=False, seed=5)
    assert torch.equal(a.blocks[0][0].weight, b.blocks[0][0].weight)
    monkeypatch.delenv("FORGE_VGG16_WEIGHTS")
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    os.makedirs(tmp_path / "hub" / "checkpoints")
    os.replace(str(p), str(tmp_path / "hub" / "checkpoints" / fp.WEIGHTS_FILE))
    c = fp.VGGPerceptualLoss()
    assert torch.equal(getattr(c.blocks[2], "14").bias, getattr(b.blocks[2], "14").bias)


def test_seeded_init_matches_golden_checksums(golden):
    g = golden("perceptual_vgg")
    sd = fp.seeded_vgg16_state_dict(int(g["seed"]))
    for k, s, q in zip(g["wkeys"].tolist(), g["wsum"], g["wsq"]):
        w = sd[k].double()
        assert abs(w.sum().item() - s) <= 1e-9 * max(1.0, abs(s)) and abs(w.square().sum().item() - q) <= 1e-9 * q, k


def test_pretrained_without_a_file_raises_and_opens_no_connection(tmp_path, monkeypatch):
    import socket
    monkeypatch.delenv("FORGE_VGG16_WEIGHTS", raising=False)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))

    def no_net(*a, **kw):
        raise AssertionError("VGGPerceptualLoss tried to open a network connection")
    monkeypatch.setattr(socket, "create_connection", no_net)
    monkeypatch.setattr(socket.socket, "connect", no_net)
    with pytest.raises(FileNotFoundError) as e:
        fp.VGGPerceptualLoss()
    assert "FORGE_VGG16_WEIGHTS" in str(e.value) and os.path.join(str(tmp_path), "hub", "checkpoints", fp.WEIGHTS_FILE) in str(e.value)


def test_host_tensors_and_bad_shapes_raise():
    m = fp.VGGPerceptualLoss(pretrained=False)
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x)


def test_new_entries_reject_bad_arguments(built_lib):
    l = _lib.lib()
    fake = 0x1000   # never dereferenced: argument checks run before any launch
    assert l.forge_vgg_prep_fwd(None, 1, 1, 1, 1, None, 1, 1, 1, 1, None, None, None, 1, 3, 8, 8, 224, 224, 1, None) == -1
    assert b"null pointer" in l.forge_last_error()
    assert l.forge_vgg_prep_fwd(fake, 1, 1, 1, 1, None, 1, 1, 1, 1, fake, fake, fake, 1, 2, 8, 8, 224, 224, 1, None) == -2      # C = 2
    assert l.forge_vgg_prep_fwd(fake, 1, 1, 1, 1, None, 1, 1, 1, 1, fake, fake, fake, 1, 3, 8, 8, 224, 224, 0, None) == -2      # no resize, sizes differ
    assert l.forge_vgg_prep_fwd(fake, 1, 1, 1, 1, None, 1, 1, 1, 1, fake, fake, fake, 0, 3, 8, 8, 224, 224, 1, None) == -1      # N = 0
    assert l.forge_vgg_prep_bwd(None, 4, fake, fake, 1, 1, 1, 1, 1, 3, 8, 8, 224, 224, 1, None) == -1
    assert l.forge_vgg_prep_bwd(fake, 4, fake, fake, 1, 1, 1, 1, 1, 4, 8, 8, 224, 224, 1, None) == -2                              # C = 4
    assert l.forge_vgg_prep_bwd(fake, 2, fake, fake, 1, 1, 1, 1, 1, 3, 8, 8, 224, 224, 1, None) == -1                              # ldg < 3
    assert l.forge_l1_partial_blocks() > 0
    assert l.forge_l1_partial(None, fake, 16, fake, None) == -1
    assert l.forge_l1_partial(fake, fake, 0, fake, None) == -1
    assert l.forge_l1_partial(fake + 4, fake, 16, fake, None) == -2                                                                 # misaligned
    assert l.forge_vgg_tap_bwd(fake, None, None, fake, fake, 1, 4, 4, 8, None) == -1                                               # coef without y
    assert l.forge_vgg_tap_bwd(None, fake, None, None, fake, 1, 4, 4, 8, None) == -1
    assert l.forge_vgg_tap_bwd(fake, fake, fake, None, fake, 1, 1, 4, 8, None) == -2                                               # pool needs H >= 2
    with pytest.raises(RuntimeError, match="forge_vgg_tap_bwd"):
        _lib.check(l.forge_vgg_tap_bwd(None, None, None, None, None, 1, 4, 4, 8, None), "forge_vgg_tap_bwd")


def test_golden_cases_are_complete(golden):
    from make_golden_perceptual import images
    g = golden("perceptual_vgg")
    for c in "abcde":
        pairs, C, H, W = (int(v) for v in g[c + "_meta"][:4])
        step = int(g[c + "_rowstep"])
        assert g[c + "_grad"].shape == (pairs, C, (H + step - 1) // step, W) and np.isfinite(g[c + "_loss"]) and g[c + "_gscale"] > 0
        inp, tgt = images(c, pairs, C, H, W)                          # the images are regenerated, not stored: they must not drift
        assert [int(inp.astype(np.int64).sum()), int(tgt.astype(np.int64).sum())] == g[c + "_codesum"].tolist()
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "perceptual_vgg.npz")) < 300_000
