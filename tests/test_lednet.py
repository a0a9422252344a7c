"""CPU: LEDNet (segmentron/models/lednet.py) served by the registry — the reference's state_dict
schema and decoder list (tests/golden/lednet_state_keys.json, tools/gen_golden_lednet.py), the
drop-in overlay, conv_bn's refusal of per-axis geometry, and the test-side restatement
(tests/_lednet_oracle.py) against the reference's own runs."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _lednet_oracle as O
from conftest import GOLDEN
from oracle import synth
from test_dropin import _run

YAML = os.path.join(GOLDEN, "cityscapes_lednet.yaml")


def lednet_cfg(*overrides):
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(YAML)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"] + list(overrides))
    cfg.PHASE = "test"
    cfg.check_and_freeze()
    return cfg


def fixture_keys():
    ref = json.load(open(os.path.join(GOLDEN, "lednet_state_keys.json")))
    return ref, [(k, tuple(s)) for k, s in ref["keys"]]


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = lednet_cfg()
        assert cfg.MODEL.MODEL_NAME == "LEDNet"
        assert cfg.TRAIN.CROP_SIZE == 768 and cfg.TRAIN.BATCH_SIZE == 4
    finally:
        reset_cfg()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = fixture_keys()
    assert len(keys) == 418 and ref["n_params"] == 2325022
    assert ref["decoder"] == ["head"]
    lednet_cfg()
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
    out = _run("""
        import sys
        sys.path = [p for p in sys.path if 'reference' not in p]
        sys.argv = ['x']
        import segmentron, segmentron_amd
        from segmentron.config import cfg
        from segmentron.models.model_zoo import get_segmentation_model, MODEL_REGISTRY
        assert 'LEDNet' in MODEL_REGISTRY.get_list()
        cfg.update_from_file(%r)
        cfg.update_from_list(['TRAIN.BACKBONE_PRETRAINED', 'False'])
        cfg.PHASE = 'test'
        cfg.check_and_freeze()
        model = get_segmentation_model()
        assert type(model).__module__ == 'segmentron_amd.models.lednet', type(model).__module__
        print('LEDNET_OK')
    """ % YAML, env_extra={"SEGMENTRON_REFERENCE_ROOT": ""})
    assert "LEDNET_OK" in out


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
    _, keys = fixture_keys()
    sd = O.state(keys)
    outs = O.evaluate(sd, synth.synth_images(O.B, O.H, O.W, seed=0))
    g = np.load(os.path.join(GOLDEN, "lednet_eval.npz"))
    assert len(outs) == int(g["n_outputs"]) == 1
    assert torch.allclose(outs[0][..., ::2, ::2], torch.from_numpy(g["logits0"]), rtol=1e-4,
                          atol=1e-4)
    odd = O.evaluate(sd, synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    assert tuple(odd[0].shape) == tuple(g["shape_odd"]) == (1, 19, 65, 97)


def _check_train(t, logits_ref, loss, outs, grads, after):
    assert abs(loss - float(t["loss"])) < 1e-5
    assert torch.allclose(outs[0][..., ::2, ::2], logits_ref, rtol=1e-4, atol=1e-4)
    names = [k[len("gnorm::"):] for k in t.files if k.startswith("gnorm::")]
    assert set(names) == set(grads)
    for k in names:
        n = float(t["gnorm::" + k])
        assert abs(float(grads[k].double().norm()) - n) <= 1e-3 * max(n, 1e-6) + 1e-9, k
    stats = [k[len("stat::"):] for k in t.files if k.startswith("stat::")]
    assert stats
    for k in stats:
        ref = torch.from_numpy(t["stat::" + k])
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(ref) == 1, k
        else:
            assert (after[k] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6, k
    return names


def train_fixture_logits():
    return torch.cat([torch.from_numpy(np.load(os.path.join(GOLDEN, f))["logits0"])
                      for f in ("lednet_train_logits_a.npz", "lednet_train_logits_b.npz")])


def test_oracle_reproduces_reference_train_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    x = synth.synth_images(O.TB, O.TH, O.TW, seed=O.TRAIN_SEED)
    y = synth.synth_targets(O.TB, O.TH, O.TW, seed=O.TRAIN_SEED)
    t = np.load(os.path.join(GOLDEN, "lednet_train.npz"))
    names = _check_train(t, train_fixture_logits(), *O.train(sd, x, y))
    assert len(names) == 238  # every parameter carries a gradient
    # what the reference's own arithmetic costs on this fixture: the yardsticks of the GPU bars
    assert 0 < float(t["cpu::grad_global"]) <= 1e-4
    assert 0 < float(t["cpu::bf16_loss_rel"]) < 1e-2 and 0.99 < float(t["cpu::bf16_grad_cos"]) < 1


def test_oracle_reproduces_reference_small_train_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    x = synth.synth_images(O.B, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B, O.H, O.W, seed=0)
    t = np.load(os.path.join(GOLDEN, "lednet_small_train.npz"))
    _check_train(t, torch.from_numpy(t["logits0"]), *O.train(sd, x, y))
