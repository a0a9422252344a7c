"""CPU: CGNet (segmentron/models/cgnet.py) served by the registry — the reference's state_dict
schema and decoder list (tests/golden/cgnet_state_keys.json, tools/gen_golden_cgnet.py), the
block-count options, the drop-in overlay, and the test-side restatement (tests/_cgnet_oracle.py)
against the reference's own runs."""
import json
import os

import numpy as np
import torch

import _cgnet_oracle as O
from conftest import GOLDEN
from oracle import synth
from test_dropin import _run

YAML = os.path.join(GOLDEN, "cityscapes_cgnet.yaml")


def cgnet_cfg(*overrides):
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(YAML)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"] + list(overrides))
    cfg.PHASE = "test"
    cfg.check_and_freeze()
    return cfg


def fixture_keys():
    ref = json.load(open(os.path.join(GOLDEN, "cgnet_state_keys.json")))
    return ref, [(k, tuple(s)) for k, s in ref["keys"]]


def small_keys():
    """The schema of the STAGE2_BLOCK_NUM 2 / STAGE3_BLOCK_NUM 2 model: the full one without the
    blocks stage2.1 and stage3.1 .. stage3.19."""
    _, keys = fixture_keys()
    return [(k, s) for k, s in keys
            if not (k.startswith(("stage2.", "stage3.")) and int(k.split(".")[1]) >= 1)]


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = cgnet_cfg()
        assert cfg.MODEL.MODEL_NAME == "CGNet"
        assert (cfg.MODEL.CGNET.STAGE2_BLOCK_NUM, cfg.MODEL.CGNET.STAGE3_BLOCK_NUM) == (3, 21)
        assert cfg.TRAIN.CROP_SIZE == 768 and cfg.TRAIN.BATCH_SIZE == 4
    finally:
        reset_cfg()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = fixture_keys()
    assert len(keys) == 499 and ref["n_params"] == 496325
    assert ref["decoder"] == ["stage1_0", "stage1_1", "stage1_2", "sample1", "sample2", "bn_prelu1",
                              "stage2_0", "stage2", "bn_prelu2", "stage3_0", "stage3", "bn_prelu3",
                              "head"]
    cgnet_cfg()
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.cgnet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert model.decoder == ref["decoder"]
        model.load_state_dict(O.state(keys), strict=True)
        assert len(model.stage2) == 2 and len(model.stage3) == 20
        blk = model.stage3[0]
        assert tuple(blk.f_sur.conv.dilation) == (4, 4) and tuple(blk.f_sur.conv.padding) == (4, 4)
        assert tuple(blk.f_glo.fc[0].weight.shape) == (8, 128)
        assert tuple(model.bn_prelu2.prelu.weight.shape) == (131,)
    finally:
        reset_cfg()


def test_block_count_options_shape_the_model():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    cgnet_cfg(*O.SMALL_OVERRIDES)
    try:
        model = segmentron_amd.get_segmentation_model()
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == small_keys()
        model.load_state_dict(O.state(small_keys()), strict=True)
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
        assert 'CGNet' in MODEL_REGISTRY.get_list()
        cfg.update_from_file(%r)
        cfg.update_from_list(['TRAIN.BACKBONE_PRETRAINED', 'False'])
        cfg.PHASE = 'test'
        cfg.check_and_freeze()
        model = get_segmentation_model()
        assert type(model).__module__ == 'segmentron_amd.models.cgnet', type(model).__module__
        from segmentron.modules import _ConvBNPReLU, _BNPReLU, _ConvBN
        assert _BNPReLU.__module__ == 'segmentron_amd.modules.basic'
        print('CGNET_OK')
    """ % YAML, env_extra={"SEGMENTRON_REFERENCE_ROOT": ""})
    assert "CGNET_OK" in out


def test_oracle_prelu_slopes_are_spread():
    _, keys = fixture_keys()
    sd = O.state(keys)
    alphas = torch.cat([v for k, v in sd.items() if k.endswith("prelu.weight")])
    assert alphas.numel() > 3000
    assert 0.05 <= alphas.min().item() < 0.06 and 0.44 < alphas.max().item() <= 0.45


def test_oracle_reproduces_reference_eval_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    outs = O.evaluate(sd, synth.synth_images(O.B, O.H, O.W, seed=0))
    g = np.load(os.path.join(GOLDEN, "cgnet_eval.npz"))
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
                      for f in ("cgnet_train_logits_a.npz", "cgnet_train_logits_b.npz")])


def test_oracle_reproduces_reference_train_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    x = synth.synth_images(O.TB, O.TH, O.TW, seed=0)
    y = synth.synth_targets(O.TB, O.TH, O.TW, seed=0)
    t = np.load(os.path.join(GOLDEN, "cgnet_train.npz"))
    names = _check_train(t, train_fixture_logits(), *O.train(sd, x, y))
    assert len(names) == 337  # every parameter carries a gradient
    # what the reference's own arithmetic costs on this fixture: the yardsticks of the GPU bars
    assert 0 < float(t["cpu::grad_global"]) <= 1e-4
    assert 0 < float(t["cpu::bf16_loss_rel"]) < 1e-2 and 0.99 < float(t["cpu::bf16_grad_cos"]) < 1


def test_oracle_reproduces_reference_small_train_fixture():
    sd = O.state(small_keys())
    x = synth.synth_images(O.B, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B, O.H, O.W, seed=0)
    t = np.load(os.path.join(GOLDEN, "cgnet_small_train.npz"))
    _check_train(t, torch.from_numpy(t["logits0"]), *O.train(sd, x, y))
