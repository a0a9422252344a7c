"""CPU: EDANet (segmentron/models/edanet.py) served by the registry — the reference's state_dict
schema (tests/golden/edanet_state_keys.json, tools/gen_golden_edanet.py), the drop-in overlay, the
refusal of sizes the reference cannot run, what line_conv_bn accepts and refuses, and the test-side
restatement (tests/_edanet_oracle.py) against the reference's own runs."""
import pytest
import torch
import torch.nn as nn

import _zoo as Z
from _edanet_spec import EDANET as SPEC

O = SPEC.O


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = Z.cfg_for(SPEC)
        assert cfg.MODEL.MODEL_NAME == "EDANet"
        assert cfg.TRAIN.CROP_SIZE == 768 and cfg.TRAIN.BATCH_SIZE == 4
    finally:
        reset_cfg()


def test_fixture_yaml_is_the_repository_config():
    import os
    from conftest import GOLDEN
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "cityscapes_edanet.yaml")) as a, \
            open(os.path.join(GOLDEN, "cityscapes_edanet.yaml")) as b:
        assert a.read() == b.read()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params  # 348 / 689485
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.edanet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert not hasattr(model, "decoder") and model.encoder is None
        model.load_state_dict(O.state(keys), strict=True)
        # the layout the restatement assumes
        from segmentron_amd.models.edanet import DownsamplerBlock, EDABlock
        assert len(model.layers) == len(O.LAYERS) == 16
        for layer, spec in zip(model.layers, O.LAYERS):
            if spec[0] == "down":
                assert isinstance(layer, DownsamplerBlock)
                assert (layer.ninput, layer.noutput) == spec[1:]
                assert tuple(layer.conv.stride) == (2, 2) and layer.conv.bias is not None
            else:
                assert isinstance(layer, EDABlock)
                assert layer.conv1x1.in_channels == spec[1] and layer.conv1x1.out_channels == 40
                assert tuple(layer.conv3x1_2.dilation) == (spec[2], spec[2])  # (one int)
                assert tuple(layer.conv3x1_2.padding) == (spec[2], 0)
                assert tuple(layer.conv1x3_2.padding) == (0, spec[2])
                assert layer.conv3x1_1.bias is not None and layer.dropout.p == 0.02
    finally:
        reset_cfg()


def test_weights_init_is_the_references():
    """normal(0, 0.02) convolution weights, normal(1, 0.02) BatchNorm weights, zero BatchNorm
    biases (edanet.py:44-51); the convolution biases keep nn.Conv2d's own initialisation."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC)
    try:
        torch.manual_seed(0)
        model = segmentron_amd.get_segmentation_model()
        w = torch.cat([m.weight.flatten() for m in model.modules() if isinstance(m, nn.Conv2d)])
        assert abs(w.mean().item()) < 1e-3 and abs(w.std().item() - 0.02) < 1e-3
        g = torch.cat([m.weight for m in model.modules() if isinstance(m, nn.BatchNorm2d)])
        assert abs(g.mean().item() - 1.0) < 5e-3 and abs(g.std().item() - 0.02) < 5e-3
        assert all(not m.bias.any() for m in model.modules() if isinstance(m, nn.BatchNorm2d))
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    Z.check_resolves_through_the_overlay(SPEC)


@pytest.mark.parametrize("hw", [(65, 96), (64, 97), (68, 96), (64, 100)])
def test_input_not_divisible_by_8_raises_before_any_launch(hw):
    """The reference raises in torch.cat for such sizes (the generator asserts it); here the
    forward says why, before it touches the device (the input is a CPU tensor: any launch would
    raise a RuntimeError instead)."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        with pytest.raises(ValueError, match="not divisible by 8"):
            model(torch.zeros(1, 3, *hw))
    finally:
        reset_cfg()


def test_group_norm_is_refused():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC, "MODEL.BN_TYPE", "GN")
    try:
        with pytest.raises(NotImplementedError, match="BN_TYPE"):
            segmentron_amd.get_segmentation_model()
    finally:
        reset_cfg()


def test_line_geometry_accepts_a_bias():
    """(raised, or not, before any tensor is touched: runs on the CPU)"""
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    for kw, want in ((dict(kernel_size=(3, 1), padding=(1, 0)), (K.AXIS_H, 1)),
                     (dict(kernel_size=(1, 3), padding=(0, 16), dilation=(1, 16)), (K.AXIS_W, 16)),
                     (dict(kernel_size=(3, 1), padding=(2, 0), dilation=2), (K.AXIS_H, 2))):
        for bias in (True, False):
            assert F._line_geometry(nn.Conv2d(40, 40, bias=bias, **kw)) == want


@pytest.mark.parametrize("kw", [dict(in_channels=40, out_channels=32, kernel_size=(3, 1),
                                     padding=(1, 0)),
                                dict(in_channels=40, out_channels=40, kernel_size=(1, 3),
                                     padding=(0, 1), stride=2),
                                dict(in_channels=40, out_channels=40, kernel_size=(1, 3),
                                     padding=(0, 1), stride=(1, 2)),
                                dict(in_channels=40, out_channels=40, kernel_size=(3, 1),
                                     padding=(2, 0)),
                                dict(in_channels=40, out_channels=40, kernel_size=(3, 1),
                                     padding=(1, 0), groups=40)])
def test_line_geometry_still_refuses_what_the_kernel_cannot_do(kw):
    from segmentron_amd import functional as F
    with pytest.raises(NotImplementedError, match="3-tap convolution"):
        F._line_geometry(nn.Conv2d(**kw))


def test_oracle_reproduces_reference_eval_fixture():
    _, g = Z.check_oracle_eval_fixture(SPEC)
    assert "shape_odd" not in g.files  # (the reference has no output for such a size)


def test_oracle_reproduces_reference_train_fixture():
    names, t = Z.check_oracle_train_fixture(SPEC)  # (222 gradients: every parameter carries one)
    assert len(names) == SPEC.n_grads


def test_oracle_reproduces_reference_small_train_fixture():
    Z.check_oracle_small_train_fixture(SPEC)
