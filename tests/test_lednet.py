"""CPU: LEDNet (segmentron/models/lednet.py) served by the registry — the reference's state_dict
schema and decoder list (tests/golden/lednet_state_keys.json, tools/gen_golden_lednet.py), the
drop-in overlay, conv_bn's refusal of per-axis geometry, and the test-side restatement
(tests/_lednet_oracle.py) against the reference's own runs."""
import pytest
import torch
import torch.nn as nn

import _zoo as Z
from _zoo import LEDNET as SPEC
from oracle import synth

O = SPEC.O


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = Z.cfg_for(SPEC)
        assert cfg.MODEL.MODEL_NAME == "LEDNet"
        assert cfg.TRAIN.CROP_SIZE == 768 and cfg.TRAIN.BATCH_SIZE == 4
    finally:
        reset_cfg()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params  # 418 / 2325022
    assert ref["decoder"] == ["head"]
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.lednet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert model.decoder == ref["decoder"]
        model.load_state_dict(O.state(keys), strict=True)
        # the encoder layout the restatement assumes
        from segmentron_amd.models.lednet import Downsampling, SSnbt
        assert len(model.encoder) == len(O.ENCODER)
        for layer, spec in zip(model.encoder, O.ENCODER):
            if spec[0] == "down":
                assert isinstance(layer, Downsampling) and tuple(layer.conv1.padding) == (2, 2)
            else:
                assert isinstance(layer, SSnbt)
                assert tuple(layer.branch1[5].dilation) == (spec[1], 1)
                assert tuple(layer.branch2[5].padding) == (0, spec[1])
        assert isinstance(model.head.level5[1].bn, nn.BatchNorm2d)
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    Z.check_resolves_through_the_overlay(SPEC)


@pytest.mark.parametrize("kw", [dict(kernel_size=(3, 1), padding=(1, 0)),
                                dict(kernel_size=(1, 3), padding=(0, 2), dilation=(1, 2)),
                                dict(kernel_size=3, padding=(1, 2), dilation=(1, 2)),
                                dict(kernel_size=3, padding=(1, 0))])
def test_conv_bn_refuses_per_axis_geometry(kw):
    """The implicit GEMM has one pad / dilation for both axes: conv_bn must not read index 0 of
    a convolution whose axes differ.  (Raised before any tensor is touched: runs on the CPU.)"""
    from segmentron_amd import functional as F
    conv = nn.Conv2d(16, 16, bias=False, **kw)
    with pytest.raises(NotImplementedError, match="differ between the axes"):
        F.conv_bn(F.Act(torch.zeros(1, 8, 8, 16)), conv)


def test_oracle_reproduces_reference_eval_fixture():
    sd, g = Z.check_oracle_eval_fixture(SPEC)
    odd = O.evaluate(sd, synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    assert tuple(odd[0].shape) == tuple(g["shape_odd"]) == (1, 19, 65, 97)


def test_oracle_reproduces_reference_train_fixture():
    Z.check_oracle_train_fixture(SPEC)  # (238 gradients: every parameter carries one)


def test_oracle_reproduces_reference_small_train_fixture():
    Z.check_oracle_small_train_fixture(SPEC)
