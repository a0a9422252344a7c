"""CPU: FPENet (segmentron/models/fpenet.py) served by the registry — the reference's config and
state_dict schema (tests/golden/fpenet_state_keys.json, tools/gen_golden_fpenet.py), its
initialisation, the drop-in overlay, the refusal of GroupNorm, the host-side contracts of the FPE
stage and MEU wrappers, and the test-side restatement (tests/_fpenet_oracle.py) against the
reference's own runs."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _zoo as Z
from _fpenet_spec import FPENET as SPEC

O = SPEC.O


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = Z.cfg_for(SPEC)
        assert cfg.MODEL.MODEL_NAME == "FPENet"
        assert cfg.TRAIN.CROP_SIZE == 768 and cfg.TRAIN.BATCH_SIZE == 4
    finally:
        reset_cfg()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params  # 516 / 115125
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.fpenet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert model.encoder is None
        model.load_state_dict(O.state(keys), strict=True)
        # the layout the restatement assumes, and the quarters the issue's table lists
        from segmentron_amd.models.fpenet import FPEBlock, MEUModule, SEModule  # noqa: F401
        quarters = {"layer1.0": 4, "layer2.0": 16, "layer2.1": 8, "layer2.2": 8, "layer3.0": 32}
        blocks = dict(model.named_modules())
        assert len(O.BLOCKS) == 13
        for p, stride, down in O.BLOCKS:
            b = blocks[p]
            assert isinstance(b, FPEBlock) and b.se is None
            assert tuple(b.conv1.stride) == (stride, stride) and (b.downsample is not None) == down
            assert [c.dilation[0] for c in b.conv2] == list(O.DILATION)
            assert [c.padding[0] for c in b.conv2] == list(O.DILATION)
            assert b.conv2[0].in_channels == b.conv2[0].groups == quarters.get(p, 16)
        assert isinstance(model.meu1, MEUModule) and model.project_layer.bias is not None
    finally:
        reset_cfg()


def test_weights_init_is_the_references():
    """kaiming_normal_(fan_out, relu) on every convolution — std sqrt(2 / (out_channels * k * k)),
    torch's fan_out does not divide by the groups — ones and zeros on the norms (fpenet.py:47-52)."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC)
    try:
        torch.manual_seed(0)
        model = segmentron_amd.get_segmentation_model()
        z = []
        for m in model.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                z.append(m.weight.flatten() / (2.0 / fan_out) ** 0.5)
        z = torch.cat(z)  # 111 985 standard normal draws
        assert abs(z.mean().item()) < 2e-2 and abs(z.std().item() - 1.0) < 2e-2
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                assert bool((m.weight == 1).all()) and not m.bias.any()
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    Z.check_resolves_through_the_overlay(SPEC)


def test_group_norm_is_refused():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC, "MODEL.BN_TYPE", "GN")
    try:
        with pytest.raises(NotImplementedError, match="BN_TYPE"):
            segmentron_amd.get_segmentation_model()
    finally:
        reset_cfg()


def test_odd_size_on_the_cpu_raises_before_any_launch():
    """The forward has no size restriction (65 x 97 gives 66 x 98 on the device, as the fixture
    records from the reference); a CPU tensor is refused by the first op, before any launch."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    assert tuple(np.load(SPEC.file("eval.npz"))["shape_odd"]) == (1, 19, 66, 98)
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        with pytest.raises(RuntimeError, match="HIP device tensors"):
            model(torch.zeros(1, 3, O.H_ODD, O.W_ODD))
    finally:
        reset_cfg()


@pytest.mark.parametrize("n,dil", [(6, 1), (8, 0), (8, 9), (68, 1)],
                         ids=["n6", "dil0", "dil9", "n68"])
def test_stage_contract_raises_before_a_tensor_is_touched(n, dil):
    """(CPU tensors: anything past the contract check would raise a RuntimeError instead)"""
    from segmentron_amd import hip_ops as K
    a = torch.zeros(1, 3, 3, n)
    v = torch.ones(n)
    w = torch.zeros(n, 1, 3, 3)
    with pytest.raises(ValueError, match="fpe_stage"):
        K.fpe_stage_fwd(a, v, v, w, dil)
    with pytest.raises(ValueError, match="fpe_stage"):
        K.fpe_stage_bwd(a, a, v, v, w, dil)
    with pytest.raises(ValueError, match="fpe_stage"):
        K.fpe_stage_check(n, dil)


def test_stage_contract_accepts_the_models_classes():
    from segmentron_amd import hip_ops as K
    for n in (4, 8, 16, 32, 64):
        for dil in (1, 2, 4, 8):
            K.fpe_stage_check(n, dil)


@pytest.mark.parametrize("C,hw,hw2", [(12, (4, 4), (2, 2)), (4, (4, 4), (2, 2)),
                                      (136, (4, 4), (2, 2)), (8, (4, 4), (5, 2))],
                         ids=["C12", "C4", "C136", "high_taller"])
def test_meu_contract_raises_before_a_tensor_is_touched(C, hw, hw2):
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    L, Hr = torch.zeros((1,) + hw + (C,)), torch.zeros((1,) + hw2 + (C,))
    a, w = torch.zeros(1, C), torch.ones(1)
    with pytest.raises(ValueError, match="meu"):
        K.meu_fwd(L, None, Hr, None, a, w)
    with pytest.raises(ValueError, match="meu"):
        K.meu_bwd_low(L, L, None, Hr, None, a, w, torch.zeros((1,) + hw))
    with pytest.raises(ValueError, match="meu"):
        K.meu_bwd_high(L, torch.zeros((1,) + hw), Hr)
    with pytest.raises(ValueError, match="meu"):
        F.meu_fuse(F.Act(L), F.Act(Hr), nn.Conv2d(C, C, 1, bias=False),
                   nn.Conv2d(1, 1, 1, bias=False))


def test_fpe_pyramid_refuses_what_it_does_not_serve():
    from segmentron_amd import functional as F
    convs = [nn.Conv2d(8, 8, 3, 1, d, d, groups=8, bias=False) for d in (1, 2, 4, 8)]
    bns = [nn.BatchNorm2d(8) for _ in range(4)]
    with pytest.raises(NotImplementedError, match="fpe_pyramid"):  # no pending BatchNorm
        F.fpe_pyramid(F.Act(torch.zeros(1, 3, 3, 32)), convs, bns)
    state = F.BNState(None, None, None, None, torch.ones(32), torch.zeros(32), 9, False)
    act = F.Act(torch.zeros(1, 3, 3, 32), state)
    wide = [nn.Conv2d(8, 8, 3, 1, d, d, groups=8, bias=False) for d in (1, 2, 4, 16)]
    with pytest.raises(ValueError, match="dilation"):
        F.fpe_pyramid(act, wide, bns)
    with pytest.raises(NotImplementedError, match="fpe_pyramid"):
        F.fpe_pyramid(act, convs[:3], bns[:3])


def test_oracle_reproduces_reference_eval_fixture():
    _, g = Z.check_oracle_eval_fixture(SPEC)
    x = Z.synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0)
    assert tuple(O.evaluate(O.state(Z.fixture_keys(SPEC)[1]), x)[0].shape) == tuple(g["shape_odd"])


def test_oracle_reproduces_reference_train_fixture():
    names, t = Z.check_oracle_train_fixture(SPEC)  # (261 gradients: every parameter carries one)
    assert len(names) == SPEC.n_grads


def test_oracle_reproduces_reference_small_train_fixture():
    Z.check_oracle_small_train_fixture(SPEC)
