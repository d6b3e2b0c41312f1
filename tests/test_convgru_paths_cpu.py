"""The coverage table of the ConvGRU fusion matrix (tests/convgru_cases.py) through the host predicates of convops alone: each shape case
reaches the launch path and point-product form it was chosen for. A rule change that moves a case off its path fails here, naming it,
without a GPU. Also: the float64 reference of the matrix is the oracle's fusion."""
import pytest
import torch

import convgru_cases as cc
import forge_oracle as fo
from forge_amd import synthetic as syn


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_reaches_its_path_and_form(built_lib, monkeypatch, name):
    from forge_amd import convops as co
    case = cc.CASE[name]
    if case.small_limit:
        monkeypatch.setattr(co, "MAX_OPERAND_BYTES", cc.operand_limit(case))
    assert cc.paths(co, case) == case.expect, name


def test_direct_kernel_switch_moves_every_case_off_winograd(built_lib):
    """Under convops.winograd(False) no case keeps a Winograd launch: the fallback the S5 matrix row measures there."""
    from forge_amd import convops as co
    with co.winograd(False):
        for case in cc.CASES:
            p = cc.paths(co, case)
            assert p["chunks"] == () and not (p["fc_wino"] or any(p["wgrad_wino"]) or p["frozen_wino"] or p["node"]), case.name


def test_reference_is_the_oracle_fusion():
    """ref_fuse (eval and train mode, float64) is bitwise forge_oracle.fuse; its wrong variants differ from it."""
    from forge_amd.fusion import ConvGRU_3D
    C = 32
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=C, hidden_size=C)
    w = {k: v.double() for k, v in syn.seeded_state_dict(gru.state_dict(), 9).items()}
    x = torch.randn(1, 3, C, 4, 4, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    pre = "encoder_3d.fusion_feature."
    for training in (False, True):
        ref = fo.fuse(x, {pre + k: v for k, v in w.items()}, training=training)
        assert torch.equal(cc.ref_fuse(x, w, training), ref)
        for kw in (dict(swap=True), dict(slope=0.02), dict(mean_div=2)):
            if training and "mean_div" in kw:
                continue                         # batch statistics normalise the scale of the view mean away
            assert (cc.ref_fuse(x, w, training, **kw) - ref).abs().max().item() > 1e-3, (training, kw)


def test_running_statistics_follow_torch_batchnorm():
    """running_after: one momentum update per batch, unbiased variance, in order - as nn.BatchNorm3d in train mode."""
    bn = torch.nn.BatchNorm3d(4).double().train()
    w = {"n.running_mean": bn.running_mean.clone(), "n.running_var": bn.running_var.clone()}
    seq = []
    for s in range(3):
        v = torch.randn(2, 4, 3, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(s))
        bn(v)
        seq.append(("n", v.mean(dim=(0, 2, 3, 4)), v.var(dim=(0, 2, 3, 4), unbiased=True)))
    rm, rv = cc.running_after(w, seq)["n"]
    assert torch.allclose(rm, bn.running_mean, rtol=0, atol=1e-15) and torch.allclose(rv, bn.running_var, rtol=0, atol=1e-15)


def test_pinned_shifts_leave_a_margin_around_zero():
    """pin_lrelu_signs moves the fusion_conv BatchNorm shifts by a tiny fraction of the scale and leaves every LeakyReLU pre-activation of
    the references (eval and train, every group) well away from zero."""
    from forge_amd.fusion import ConvGRU_3D
    C = 32
    gru = ConvGRU_3D(syn.kubric_config(), n_layers=1, input_size=C, hidden_size=C)
    w = syn.seeded_state_dict(gru.state_dict(), 9)
    x = torch.randn(1, cc.T, C, 4, 8, 8, generator=torch.Generator().manual_seed(2)) * 0.5
    moved = cc.pin_lrelu_signs(x, w, cc.ALL_GROUPS)
    assert moved < 2e-3
    wd, xd = {k: v.double() for k, v in w.items()}, x.double()
    for g in cc.ALL_GROUPS:
        for training in (False, True):
            log = {}
            cc.ref_fuse(xd[:, list(g)], wd, training, log=log)
            assert cc.lrelu_margin(log) > 1e-5, (g, training)
