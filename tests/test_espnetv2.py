"""CPU: ESPNetV2 on EESPNet (segmentron/models/espnetv2.py) served by the registry — the
reference's state_dict schema and `exclusive` list (tests/golden/espnetv2_state_keys.json,
tools/gen_golden_espnetv2.py), the drop-in overlay, conv_bn's refusal of grouped 3x3, and the
test-side restatement (tests/_espnetv2_oracle.py) against the reference's own runs."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _zoo as Z
from _zoo import ESPNETV2 as SPEC
from oracle import synth

O = SPEC.O


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = Z.cfg_for(SPEC)
        assert cfg.MODEL.MODEL_NAME == "ESPNetV2" and cfg.MODEL.BACKBONE == "eespnet"
        assert tuple(cfg.TRAIN.CROP_SIZE) == (512, 1024) and cfg.TRAIN.BATCH_SIZE == 4
        assert cfg.SOLVER.AUX is False
    finally:
        reset_cfg()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params  # 640 / 2163324
    assert ref["exclusive"] == ["proj_L4_C", "pspMod", "project_l3", "act_l3", "project_l2",
                                "project_l1"]
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.espnetv2"
        assert type(model.encoder).__module__ == "segmentron_amd.models.backbones.eespnet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert sum(1 for _ in model.parameters()) == 397
        assert model.exclusive == ref["exclusive"] and not hasattr(model, "decoder")
        assert model.aux is False
        model.load_state_dict(O.state(keys), strict=True)
        # the geometry the restatement assumes: four branches, these dilations, groups = 4
        from segmentron_amd.modules import EESP
        units = {n: m for n, m in model.named_modules() if isinstance(m, EESP)}
        reached = {n: m for n, m in units.items() if not O.unused(n + ".")}
        assert len(reached) == 14 and len(units) == 14 + 1 + 7
        for name, m in reached.items():
            assert [c.dilation[0] for c in m.spp_dw] == O.dilations(O._r_lim(name)), name
            assert all(c.padding == c.dilation for c in m.spp_dw)
            assert m.proj_1x1.conv.groups == m.conv_1x1_exp.conv.groups == O.K
        assert O.dilations(9) == [1, 2, 3, 4] and O.dilations(7) == [1, 1, 2, 3]
        assert tuple(model.pspMod[0].proj_1x1.conv.weight.shape) == (32, 64, 1, 1)
        assert tuple(model.encoder.level2_0.eesp.proj_1x1.conv.weight.shape) == (8, 8, 1, 1)
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    Z.check_resolves_through_the_overlay(SPEC)


@pytest.mark.parametrize("kw", [dict(kernel_size=3, padding=1, groups=4),
                                dict(kernel_size=1, stride=2, groups=4),
                                dict(kernel_size=1, padding=1, groups=4),
                                dict(kernel_size=1, groups=4, bias=True)])
def test_conv_bn_refuses_other_grouped_geometry(kw):
    """Grouped convolutions are served as 1x1 / stride 1 / unpadded / bias-free only (the
    block-diagonal packing).  (Raised before any tensor is touched: runs on the CPU.)"""
    from segmentron_amd import functional as F
    kw.setdefault("bias", False)
    conv = nn.Conv2d(32, 32, **kw)
    with pytest.raises(NotImplementedError, match="groups=4"):
        F.conv_bn(F.Act(torch.zeros(1, 8, 8, 32)), conv)


def test_block_diagonal_packing_round_trips():
    """The dense weight of a grouped 1x1 computes the grouped convolution, and the diagonal blocks
    of a dense gradient come back in the parameter's layout."""
    from segmentron_amd import functional as F
    g = torch.Generator().manual_seed(0)
    for C, O_ in ((32, 8), (256, 32), (128, 128)):
        w = torch.randn((O_, C // 4, 1, 1), generator=g, dtype=torch.float64)
        x = torch.randn((2, C, 5, 7), generator=g, dtype=torch.float64)
        dense = F.block_diag_weight(w, 4)
        assert tuple(dense.shape) == (O_, C, 1, 1)
        assert torch.allclose(torch.nn.functional.conv2d(x, dense),
                              torch.nn.functional.conv2d(x, w, groups=4), rtol=0, atol=1e-12)
        assert int((dense != 0).sum()) == w.numel()
        assert torch.equal(F.block_diag_grad(dense.reshape(O_, C), 4), w)


def test_pyramid_contract_and_routing():
    from segmentron_amd import functional as F
    assert F.eesp_pyramid_in_contract(32, (1, 2, 3, 4), 1)
    assert F.eesp_pyramid_in_contract(64, (1, 1, 2, 3), 2)
    for n, dils, s in ((12, (1, 2, 3, 4), 1), (8, (1, 2, 3, 5), 1), (8, (1, 3, 2, 4), 1),
                       (8, (1, 2, 3), 1), (8, (1, 2, 3, 4), 3), (0, (1, 2, 3, 4), 1)):
        assert not F.eesp_pyramid_in_contract(n, dils, s)
        assert not F.eesp_pyramid_routed(torch.bfloat16, n, dils, s)


def test_oracle_reproduces_reference_eval_fixture():
    sd, g = Z.check_oracle_eval_fixture(SPEC)
    second = O.evaluate(sd, synth.synth_images(1, O.H2, O.W2, seed=0))
    assert tuple(second[0].shape) == (1, 19, O.H2, O.W2)
    assert torch.allclose(second[0][..., ::2, ::2], torch.from_numpy(g["logits0_second"]),
                          rtol=1e-4, atol=1e-4)


def test_oracle_reproduces_reference_train_fixture():
    names, t = Z.check_oracle_train_fixture(SPEC)
    assert int(t["seed"]) == O.TRAIN_SEED
    # the parameters with a gradient are the reference's, 256 of 397: level5*, fc (and the
    # module_act a DownSampler's EESP unit returns before) have none
    assert not any(k.startswith(O.UNUSED) for k in names)
    assert not any(O.unused(k) for k in names)


def test_oracle_reproduces_reference_small_train_fixture():
    Z.check_oracle_small_train_fixture(SPEC)


def test_parameters_with_a_gradient_are_the_references():
    """The model's own parameter names split the way the reference's gradients do."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    t = np.load(SPEC.file("train.npz"))
    with_grad = {k[len("gnorm::"):] for k in t.files if k.startswith("gnorm::")}
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        names = {k for k, _ in model.named_parameters()}
        assert with_grad <= names
        assert {k for k in names if not O.unused(k)} == with_grad
        assert any(k.startswith("encoder.level5.") for k in names - with_grad)
        assert "encoder.fc.weight" in names - with_grad
    finally:
        reset_cfg()
